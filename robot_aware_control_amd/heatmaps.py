"""End-effector heatmaps for `--model_use_heatmap`, made on the device (`rac_eef_heatmaps`).

The reference makes them per video on the host (robonet_dataset.py:482-544 `create_heatmaps`: denormalise the states,
add the robot's gripper offset, project with the viewpoint's camera, cast to integers, evaluate a 48x64 Gaussian per
time step in numpy) and uploads the result (trainer.py:234-246, locobot_model.py:179-193).  Here the host's share is one
small record per video -- the fp64 projection `K @ wTc[:3]`, the two scale factors and the fp32 z offset, computed in
numpy exactly as the reference does -- and one launch writes the heatmaps of every frame of a batch.

Divergence, on purpose: the reference casts the projected coordinates with `astype(np.uint8)`, which is exact truncation
inside (-1, 256) and undefined outside (numpy 2 wraps: -3.2 -> 253, 300.7 -> 44), so a point far outside the image can
wrap back into it.  Here a frame is valid iff its truncated coordinates lie inside the image; everything else,
non-finite coordinates included, gives an all-zero heatmap.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

# robot -> (fp32 z offset, intrinsics key, original (width, height)); robonet_dataset.py:497-516
ROBOTS = {
    "sawyer": (-0.15, "logitech_c420", (320, 240)),
    "baxter": (0.0, "logitech_c420", (320, 240)),
    "widowx": (0.05, "logitech_c420", (320, 240)),   # mounted upside down: positive z
    "locobot": (0.0, "intel_realsense_d435", (640, 480)),
}
VIEW = np.dtype([("proj", "<f8", (12,)), ("scale_x", "<f8"), ("scale_y", "<f8"), ("z_offset", "<f4"), ("reserved", "<i4")])
assert VIEW.itemsize == ctypes.sizeof(_lib.HeatmapView) == 120
VIEW_ROW = 17  # a view as plain float64 numbers, the form a dataset item carries: proj, scale_x, scale_y, z_offset, H, W


def view_key(robot: str, viewpoint: str) -> str:
    """The key of `world_to_camera_dict` for a robot's viewpoint; an unknown robot is a ValueError, as in the reference."""
    if robot not in ROBOTS:
        raise ValueError(f"create_heatmaps: unknown robot {robot!r} (one of {sorted(ROBOTS)})")
    return "locobot_c0" if robot == "locobot" else f"{robot}_{viewpoint}"


class CameraTable:
    """`world_to_camera` (4, 4) and `intrinsics` (3, 3) float64 arrays by key: the part of the reference's
    src/utils/camera_calibration.py the heatmaps need."""

    def __init__(self, world_to_camera: dict, intrinsics: dict):
        self.world_to_camera = {k: np.asarray(v, dtype=np.float64).reshape(4, 4) for k, v in world_to_camera.items()}
        self.intrinsics = {k: np.asarray(v, dtype=np.float64).reshape(3, 3) for k, v in intrinsics.items()}
        self._rows = {}

    @classmethod
    def from_reference(cls):
        """From `src.utils.camera_calibration` of a reference checkout on the path (the route data._camera_dicts takes)."""
        from src.utils.camera_calibration import cam_intrinsics_dict, world_to_camera_dict
        return cls(world_to_camera_dict, cam_intrinsics_dict)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls({k[4:]: z[k] for k in z.files if k.startswith("w2c_")},
                       {k[2:]: z[k] for k in z.files if k.startswith("K_")})

    def save(self, path):
        arrays = {f"w2c_{k}": v for k, v in self.world_to_camera.items()}
        arrays.update({f"K_{k}": v for k, v in self.intrinsics.items()})
        with open(path, "wb") as f:  # (a file object: np.savez would append ".npz" to a bare name)
            np.savez(f, **arrays)

    @classmethod
    def from_config(cls, config):
        """`--camera_calibration FILE` when given, else the reference import; the error names both when neither works."""
        path = getattr(config, "camera_calibration", None)
        if path:
            return cls.load(path)
        try:
            return cls.from_reference()
        except ImportError as e:
            raise ImportError(
                "model_use_heatmap needs the camera calibration: pass --camera_calibration FILE (an .npz written by "
                "tools/export_camera_calibration.py / CameraTable.save), or put a reference checkout with "
                f"src/utils/camera_calibration.py on the path ({e})") from e

    def view_row(self, robot: str, viewpoint: str, height: int, width: int) -> np.ndarray:
        """One video's view as VIEW_ROW float64 numbers, in the reference's arithmetic (get_2d_eef_pos)."""
        key = (robot, viewpoint, int(height), int(width))
        row = self._rows.get(key)
        if row is None:
            name = view_key(robot, viewpoint)
            z_offset, camera, (orig_w, orig_h) = ROBOTS[robot]
            if name not in self.world_to_camera or camera not in self.intrinsics:
                raise KeyError(f"camera table has no entry {name!r} / {camera!r}")
            proj = self.intrinsics[camera] @ self.world_to_camera[name][:3]
            row = np.concatenate([proj.reshape(12), [width / orig_w, height / orig_h, float(np.float32(z_offset)),
                                                     float(height), float(width)]])
            self._rows[key] = row
        return row

    def view_rows(self, robots, folders, height: int, width: int) -> np.ndarray:
        return np.stack([self.view_row(str(r), str(f), height, width) for r, f in zip(robots, folders)])


def pack_views(rows) -> np.ndarray:
    """(B, VIEW_ROW) float64 rows -> B `rac_heatmap_view` records."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, VIEW_ROW)
    views = np.zeros(len(rows), dtype=VIEW)
    views["proj"], views["scale_x"], views["scale_y"] = rows[:, :12], rows[:, 12], rows[:, 13]
    views["z_offset"] = rows[:, 14].astype(np.float32)
    return views


def heatmaps_from_views(states, low, high, rows, height: int, width: int, out=None, first_row: int = 0,
                        time_first: bool = True, centres: bool = False, keep=None):
    """One `rac_eef_heatmaps` launch on the current stream.  `states` (T, B, S >= 3) on the GPU, or (B, T, S) with
    `time_first=False`: read in place through their strides.  `low` / `high` (B, >= 3), `rows` (B, VIEW_ROW).  Writes rows
    `first_row .. first_row + T` of `out` (a time-first (T', B, 1, H, W) fp32 tensor; a fresh (T, B, 1, H, W) one when
    None) and returns `out`, or `(out, centres)` with the int32 (T, B, 3) = (mx, my, valid).  `keep`: a list that receives
    the launch's device inputs, for a caller that must hold them until a side stream has run."""
    if not (torch.is_tensor(states) and states.is_cuda):
        raise _lib.RacError("heatmaps are made on the GPU (rac_eef_heatmaps; no CPU fallback)")
    dev = states.device
    if states.dim() != 3 or states.shape[-1] < 3:
        raise _lib.RacError(f"heatmaps: states (T, B, S >= 3), got {tuple(states.shape)}")
    if not time_first:
        states = states.transpose(0, 1)
    if states.dtype != torch.float32 or states.stride(2) != 1:
        states = states.to(torch.float32).contiguous()
    T, B = int(states.shape[0]), int(states.shape[1])
    H, W = int(height), int(width)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, VIEW_ROW)
    if len(rows) != B:
        raise _lib.RacError(f"heatmaps: {len(rows)} views for {B} videos")
    bounds = [torch.as_tensor(b).to(dev, torch.float32).reshape(B, -1).contiguous() for b in (low, high)]
    if bounds[0].shape != bounds[1].shape or bounds[0].shape[1] < 3:
        raise _lib.RacError(f"heatmaps: low / high (B, >= 3), got {tuple(bounds[0].shape)} and {tuple(bounds[1].shape)}")
    if out is None:
        out, first_row = torch.empty((T, B, 1, H, W), device=dev, dtype=torch.float32), 0
    if (out.dim() != 5 or out.dtype != torch.float32 or out.device != dev or tuple(out.shape[1:]) != (B, 1, H, W)
            or first_row < 0 or first_row + T > out.shape[0] or (out.numel() and not out[0, 0].is_contiguous())):
        raise _lib.RacError(f"heatmaps: out must be fp32 (>= {first_row + T}, {B}, 1, {H}, {W}) with dense frames on "
                            f"{dev}, got {tuple(out.shape)} {out.dtype} on {out.device}")
    cen = torch.empty((T, B, 3), device=dev, dtype=torch.int32) if centres else None
    if T:
        views = torch.from_numpy(pack_views(rows).view(np.uint8).reshape(B, VIEW.itemsize)).to(dev)
        with torch.cuda.device(dev):
            _lib.call("rac_eef_heatmaps", _lib.ptr(states), states.stride(0), states.stride(1), _lib.ptr(bounds[0]),
                      _lib.ptr(bounds[1]), bounds[0].stride(0), _lib.ptr(views), _lib.ptr(out[first_row]), out.stride(0),
                      out.stride(1), _lib.ptr(cen), T, B, H, W, _lib.stream_ptr())
        if keep is not None:
            keep.extend([states, bounds[0], bounds[1], views])
    return (out, cen) if centres else out


def batch_heatmaps(states, low, high, robots, folders, table: CameraTable, height: int, width: int, out=None,
                   first_row: int = 0):
    """Heatmaps (T, B, 1, H, W) of a time-first batch of normalised world-frame states (T, B, S), on the states' device,
    in one launch: video b with its own `low[b]` / `high[b]`, `robots[b]` and viewpoint `folders[b]`.  With `out`, rows
    `first_row .. first_row + T` of that tensor are written and the rest is left alone (the robot models keep row 0)."""
    return heatmaps_from_views(states, low, high, table.view_rows(robots, folders, height, width), height, width, out,
                               first_row)


_TABLE = None


def use_camera_table(table):
    """The table `create_heatmaps` projects with (None: back to the reference import on next use)."""
    global _TABLE
    _TABLE = table


def create_heatmaps(states, low, high, robot, viewpoint):
    """The reference's `create_heatmaps` (robonet_dataset.py:482-544): states (T, S) normalised, low / high the bounds,
    -> numpy (T, 1, 48, 64) float32 -- through the kernel, so CPU tensors are moved to the current device and a machine
    without one raises RacError.  The calibration is the reference's own module (`CameraTable.from_reference`)."""
    global _TABLE
    view_key(robot, viewpoint)
    if not torch.cuda.is_available():
        raise _lib.RacError("create_heatmaps runs on the GPU (rac_eef_heatmaps; no CPU fallback)")
    if _TABLE is None:
        _TABLE = CameraTable.from_config(None)
    s = torch.as_tensor(states)
    s = s if s.is_cuda else s.to(torch.device("cuda", torch.cuda.current_device()))
    out = batch_heatmaps(s.unsqueeze(1), torch.as_tensor(low).reshape(1, -1), torch.as_tensor(high).reshape(1, -1),
                         [robot], [viewpoint], _TABLE, 48, 64)
    return out[:, 0].cpu().numpy()
