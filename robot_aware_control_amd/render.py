"""Robot masks from joint positions, rendered on the device (`rac_render_masks`).

`MjcfMaskRenderer` has the contract of the reference's MuJoCo mask environments (src/env/robotics/masks/base_mask_env.py:
`set_opencv_camera_pose`, `generate_masks(list_of_qpos, width, height) -> bool (n, H, W)`), so it drops into
`LearnedRobotModel(renderers={viewpoint: ...})` and `RobotPredictionTrainer.plot`; and it has `render(qpos)` for joint
positions that are already on the GPU: (P, J) -> (P, 1, h, w) fp32 with no host copy, the route
`LearnedRobotModel.predict_batch` takes.  The model comes from `mjcf.load_mjcf`; its tables are uploaded once.  There is
no CPU fallback: off the GPU every render raises RacError.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib, mjcf

LINK = np.dtype([("local", "<f4", (12,)), ("axis", "<f4", (3,)), ("anchor", "<f4", (3,)), ("parent", "<i4"),
                 ("joint", "<i4"), ("qcol", "<i4"), ("reserved", "<i4")])
assert LINK.itemsize == ctypes.sizeof(_lib.RenderLink) == 88


def _affine(pos, quat) -> np.ndarray:
    """T(pos) R(quat) as the 12 numbers of a row-major 3x4."""
    return np.concatenate([mjcf.quat_to_mat(quat), np.asarray(pos, dtype=np.float64).reshape(3, 1)], axis=1).reshape(12)


class MjcfMaskRenderer:
    """Masks of `model` (an `mjcf.MjcfModel`, or the path of an MJCF file `mjcf.load_mjcf` knows by name) seen from its
    camera `camera`.  `_img_height` / `_img_width` are the native render size, as in the reference environments."""

    def __init__(self, model, camera="main_cam", device=None):
        if isinstance(model, (str, os.PathLike)):
            model = mjcf.load_mjcf(model)
        if camera not in model.cameras:
            raise ValueError(f"model {model.name!r} has no camera {camera!r} (it has {sorted(model.cameras)})")
        if len(model.tri) == 0:
            raise ValueError(f"model {model.name!r} has no geometry to render")
        self.model, self._camera_name = model, camera
        self._img_height, self._img_width = model.native_hw
        self._poses = {name: (cam.pos.copy(), cam.quat.copy()) for name, cam in model.cameras.items()}
        self._device = None if device is None else torch.device(device)
        self._tables = None

    @property
    def joints(self):
        return self.model.joints

    def set_opencv_camera_pose(self, cam_name, camera_extrinsics, offset=(0, 0, 0)):
        """The reference's call (base_mask_env.py:8-22): afterwards `cam_name` sees the OpenCV pinhole image of the
        camera-to-world `camera_extrinsics` (x right, y down, z forward, fx = fy = f, cx = W / 2, cy = H / 2)."""
        if cam_name not in self._poses:
            raise ValueError(f"model {self.model.name!r} has no camera {cam_name!r}")
        self._poses[cam_name] = mjcf.opencv_camera_pose(camera_extrinsics, offset)

    def _upload(self, dev):
        m = self.model
        links = np.zeros(m.n_links, dtype=LINK)
        for l in range(m.n_links):
            links["local"][l] = _affine(m.link_pos[l], m.link_quat[l])
        links["axis"], links["anchor"] = m.joint_axis, m.joint_anchor
        links["parent"], links["joint"], links["qcol"] = m.link_parent, m.joint_type, m.joint_col
        if not all(-1 <= int(p) < l for l, p in enumerate(m.link_parent)) or int(m.tri_link.max()) >= m.n_links:
            raise ValueError(f"model {m.name!r}: links must list parents first and triangles must name a link")
        n = len(m.tri)
        stride = (n + 63) // 64 * 64
        soa = np.zeros((9, stride), dtype=np.float32)
        soa[:, :n] = m.tri.reshape(n, 9).T
        meta = (m.tri_link.astype(np.int32) | (m.tri_robot.astype(np.int32) << 8)).astype(np.int32)
        self._tables = dict(
            dev=dev, links=torch.from_numpy(links.view(np.uint8).reshape(m.n_links, LINK.itemsize).copy()).to(dev),
            tri=torch.from_numpy(soa).to(dev), meta=torch.from_numpy(meta).to(dev), n=n, stride=stride,
            other=int(not bool(m.tri_robot.all())))

    def render(self, qpos, out_hw=None, render_hw=None, out=None, extras=None):
        """qpos (P, J) on the GPU -> (P, 1, h, w) fp32 masks (0 or 1) on the same device, in one launch on the current
        stream.  `render_hw`: the size rendered at (the native one by default); `out_hw`: the size written, by the
        resize rule of `robot_model.resize_masks` (the render size by default).  `out`: a dense fp32 (P, 1, h, w) tensor
        to write.  `extras`: a dict that receives `native` (P, 1, H, W), the render before the resize, and `link_xpos`
        (P, L, 3), the links' world positions."""
        if not (torch.is_tensor(qpos) and qpos.is_cuda):
            raise _lib.RacError("MjcfMaskRenderer renders on the GPU only (rac_render_masks; no CPU fallback)")
        dev = qpos.device
        if self._device is not None and self._device.type == "cuda" and self._device.index not in (None, dev.index):
            raise _lib.RacError(f"MjcfMaskRenderer was built for {self._device}, qpos is on {dev}")
        J = len(self.model.joints)
        if qpos.dim() != 2 or qpos.shape[1] != J:
            raise ValueError(f"qpos must be (P, {J}) for joints {list(self.model.joints)}, got {tuple(qpos.shape)}")
        H, W = (int(x) for x in (render_hw or (self._img_height, self._img_width)))
        h, w = (int(x) for x in (out_hw or (H, W)))
        if H < 1 or W < 1 or H * W > _lib.RENDER_MAX_PIXELS:
            raise ValueError(f"render size {H} x {W}: at most {_lib.RENDER_MAX_PIXELS} pixels are rendered "
                             f"(two depth buffers of H W must fit the workgroup's LDS)")
        if not (1 <= h <= 4096 and 1 <= w <= 4096):
            raise ValueError(f"output size {h} x {w} outside 1..4096")
        if qpos.dtype != torch.float32 or qpos.stride(1) != 1:
            qpos = qpos.to(torch.float32).contiguous()
        P = int(qpos.shape[0])
        if out is None:
            out = torch.empty((P, 1, h, w), device=dev, dtype=torch.float32)
        elif (out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (P, 1, h, w)
              or not out.is_contiguous()):
            raise ValueError(f"out must be a dense fp32 ({P}, 1, {h}, {w}) tensor on {dev}, got {tuple(out.shape)} "
                             f"{out.dtype} on {out.device}")
        native = xpos = None
        if extras is not None:
            native = extras["native"] = torch.empty((P, 1, H, W), device=dev, dtype=torch.float32)
            xpos = extras["link_xpos"] = torch.empty((P, self.model.n_links, 3), device=dev, dtype=torch.float32)
        if P == 0:
            return out
        if self._tables is None or self._tables["dev"] != dev:
            self._upload(dev)
        t = self._tables
        cam = self.model.cameras[self._camera_name]
        pos, quat = self._poses[self._camera_name]
        cam_local = (ctypes.c_float * 12)(*_affine(pos, quat))
        with torch.cuda.device(dev):
            _lib.call("rac_render_masks", _lib.ptr(qpos), qpos.stride(0), P, J, _lib.ptr(t["links"]), self.model.n_links,
                      _lib.ptr(t["tri"]), t["stride"], _lib.ptr(t["meta"]), t["n"], t["other"],
                      ctypes.cast(cam_local, ctypes.c_void_p), cam.link, float(cam.fovy), H, W, h, w, _lib.ptr(out),
                      _lib.ptr(native), _lib.ptr(xpos), _lib.stream_ptr())
        return out

    def generate_masks(self, qpos_data, width=None, height=None):
        """The reference environments' call: a sequence of qpos rows -> numpy bool (n, H, W), rendered at the native size
        or at `height` x `width` when both are given."""
        if not torch.cuda.is_available():
            raise _lib.RacError("MjcfMaskRenderer renders on the GPU only (rac_render_masks; no CPU fallback)")
        dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
        hw = (self._img_height, self._img_width) if width is None or height is None else (int(height), int(width))
        rows = np.asarray([np.asarray(q, dtype=np.float32) for q in qpos_data], dtype=np.float32)
        rows = rows.reshape(-1, len(self.model.joints)) if rows.size == 0 else rows
        masks = self.render(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), render_hw=hw)
        return masks[:, 0].cpu().numpy() != 0
