"""The data path that feeds the train step: trajectory files -> (B, T, ...) batches -> time-first tensors on the device.

Drop-in for the reference's `src/dataset/robonet/robonet_dataset.py` (`RoboNetDataset`, `process_batch`, `get_batch`,
`normalize`, `denormalize`) and `robonet_dataloaders.py` (`create_loaders`): same constructor arguments, same item
dictionary (keys, shapes, dtypes), same window sampling, state / action / bound preprocessing and mask binarisation,
same file discovery, shuffling and train / test split.

What is different, for a trainer that consumes ~2 800 frames/s per GPU:
  * frames are resized with one batched `interpolate` call per trajectory instead of one PIL / torchvision call per
    frame (bilinear, align_corners=False, no antialias: what `tf.Resize` does to a tensor in the torchvision the
    reference pins);
  * `get_batch` runs a DEVICE PREFETCHER: the next batch's pinned host tensors are copied on a side HIP stream and
    transposed to time-first there while the current step computes (the reference transposes on the host and copies on
    the compute stream);
  * trajectory files may be HDF5 (`h5py`, imported when the first `.hdf5` file is opened) or `.npz` archives with the
    same dataset names (the format of `tools/make_synthetic_robonet.py`, used by the tests: this container has no h5py);
  * `--device_images True` (off by default) moves the image half of an item to the GPU: the dataset hands over the raw
    uint8 frames, the binary raw masks and the augmentation parameters it drew (`draw_image_params`), `collate` packs a
    batch's videos (of any raw sizes) into one flat uint8 buffer plus one `rac_image_job` per video, and one
    `rac_image_pipeline` launch on the prefetcher's stream writes the time-first fp32 `images` / `masks`;
  * `--model_use_heatmap True`: an item carries its bounds and its camera (`heatmap_view`, a row of numbers from
    heatmaps.CameraTable) and `process_batch` / the prefetcher add the time-first `heatmaps` of the whole batch with one
    `rac_eef_heatmaps` launch on the stream they already use (the reference's dataset raises under this flag);
  * `experiment_loaders` gives every `--experiment` of the reference's trainer its own split (trainer.py:899-947), and
    `--device_resident True` (off by default) keeps such a split on the GPU: `ResidentVideos` holds every stored video
    and the preprocessed numerics, the loader only draws (`ResidentDataset`), and a batch is `rac_image_pipeline` on the
    resident frames plus `rac_window_gather` for the numerics behind an upload of the jobs and the (index, start) pairs.
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
import random
import threading
from queue import Queue
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.data as data

from . import _lib

TRANSPOSE_KEYS = ("qpos", "images", "states", "actions", "masks", "heatmaps", "raw_actions", "raw_states")

# robonet_dataloaders.py:13-18
BAXTER_TRAIN_DIRS = ["left_c0"]
WIDOWX_TRAIN_DIRS = ["widowx1_c0"]
SAWYER_TRAIN_DIRS = ["sudri0_c0", "sudri0_c1", "sudri0_c2", "sudri2_c0", "sudri2_c1", "sudri2_c2", "vestri_table2_c0",
                     "vestri_table2_c1", "vestri_table2_c2"]
TRAJ_EXTENSIONS = (".hdf5", ".npz")


def denormalize(states, low, high):
    """robonet_dataset.py:470-473."""
    states = states * (high - low)
    states = states + low
    return states


def normalize(states, low, high):
    """robonet_dataset.py:476-479."""
    states = states - low
    states = states / (high - low)
    return states


# --------------------------------------------------------------------------- #
# trajectory files
# --------------------------------------------------------------------------- #
class _NpzTrajectory:
    """An `.npz` archive behind the part of the h5py.File interface the dataset uses (`in`, `[name]`, `.attrs`)."""

    def __init__(self, path):
        self._z = np.load(path, allow_pickle=False)
        self.attrs = {k[5:]: str(self._z[k]) for k in self._z.files if k.startswith("attr_")}

    def __contains__(self, k):
        return k in self._z.files

    def __getitem__(self, k):
        return self._z[k]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self._z.close()


def open_trajectory(path):
    if path.endswith(".npz"):
        return _NpzTrajectory(path)
    try:
        import h5py
    except ImportError as e:  # pragma: no cover - depends on the deployment image
        raise ImportError(f"{path}: reading HDF5 trajectories needs h5py (or convert them to .npz with the same "
                          f"dataset names)") from e
    return h5py.File(path, "r")


def _camera_dicts():
    """Camera calibration tables live in the reference tree (src/utils/camera_calibration.py: measured extrinsics of
    the authors' rigs); only the `camera_*` action preprocessing needs them."""
    from src.utils.camera_calibration import camera_to_world_dict, world_to_camera_dict
    return world_to_camera_dict, camera_to_world_dict


# --------------------------------------------------------------------------- #
# image preprocessing (robonet_dataset.py:257-300)
# --------------------------------------------------------------------------- #
def _to_tensor(x: np.ndarray) -> torch.Tensor:
    """tf.ToTensor on a stack: uint8 (T,H,W,C) -> float (T,C,H,W) / 255; float (T,H,W) -> (T,1,H,W) unscaled."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if t.dim() == 3:
        t = t.unsqueeze(-1)
    t = t.permute(0, 3, 1, 2)
    return t.float().div(255) if x.dtype == np.uint8 else t.float()


def _resize(t: torch.Tensor, h: int, w: int) -> torch.Tensor:
    if tuple(t.shape[-2:]) == (h, w):
        return t
    return F.interpolate(t, size=(h, w), mode="bilinear", align_corners=False)


def _gray(img):
    return (0.2989 * img[:, 0:1] + 0.587 * img[:, 1:2] + 0.114 * img[:, 2:3])


def _adjust_hue(img, factor):
    r, g, b = img[:, 0], img[:, 1], img[:, 2]
    maxc, minc = img.max(1).values, img.min(1).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    crd = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = (h + factor) % 1.0
    v = maxc
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p, q, t = (v * (1.0 - s)).clamp(0, 1), (v * (1.0 - s * f)).clamp(0, 1), (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    sel = torch.stack([torch.stack([v, q, p, p, t, v], 1), torch.stack([t, v, v, q, p, p], 1),
                       torch.stack([p, p, t, v, v, q], 1)], 1)  # (T, 3, 6, H, W)
    idx = i[:, None, None].expand(-1, 3, 1, -1, -1).long()
    return sel.gather(2, idx).squeeze(2)


JITTER_RANGES = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))  # brightness, contrast, saturation, hue


def draw_color_jitter(brightness, contrast, saturation, hue):
    """The random part of get_random_color_jitter (robonet_dataset.py:545-572): the four factors drawn with
    `random.uniform` in the order brightness, contrast, saturation, hue, then one `random.shuffle` of the four
    operations.  Returns (factors, order): operation order[k] runs k-th, 0 = brightness .. 3 = hue."""
    factors = tuple(random.uniform(*r) for r in (brightness, contrast, saturation, hue))
    order = [0, 1, 2, 3]
    random.shuffle(order)
    return factors, tuple(order)


def color_jitter(factors, order):
    """The function of a (T,3,H,W) clip that applies drawn jitter parameters in the drawn order (brightness, contrast and
    saturation clamped to [0, 1], the hue shift through hsv)."""
    bf, cf, sf, hf = factors
    ops = (lambda im: (im * bf).clamp(0, 1),
           lambda im: (cf * im + (1 - cf) * _gray(im).mean((1, 2, 3), keepdim=True)).clamp(0, 1),
           lambda im: (sf * im + (1 - sf) * _gray(im)).clamp(0, 1),
           lambda im: _adjust_hue(im, hf))

    def apply(im):
        for k in order:
            im = ops[k](im)
        return im
    return apply


def random_color_jitter(brightness, contrast, saturation, hue):
    """get_random_color_jitter (robonet_dataset.py:545-572): factors drawn with `random.uniform` in this order, the
    four adjustments applied in a `random.shuffle`d order; returns a function of a (T,3,H,W) clip."""
    return color_jitter(*draw_color_jitter(brightness, contrast, saturation, hue))


class ImageParams(NamedTuple):
    """What `ImagePipeline` decides at random for one trajectory, apart from its application: the crop window
    (top, left, th, tw) of the (h, w) model-size clip that is resized back to (h, w) -- the whole clip without
    augmentation -- and, when `jitter`, the colour factors (brightness, contrast, saturation, hue) and the order of the
    four operations (order[k] runs k-th; 0 = brightness, 1 = contrast, 2 = saturation, 3 = hue)."""
    h: int
    w: int
    top: int
    left: int
    th: int
    tw: int
    jitter: bool
    order: tuple
    factors: tuple


def draw_image_params(h: int, w: int, augment: bool) -> ImageParams:
    """Draws one trajectory's augmentation from the `random` and torch generators exactly as the reference's item code
    does (robonet_dataset.py:271-300): `random.randint(0, 5)` for the shrink, the crop corner from the torch generator
    (row first, only when the shrink is non-zero), then the colour jitter's draws."""
    if not augment:
        return ImageParams(h, w, 0, 0, h, w, False, (0, 1, 2, 3), (1.0, 1.0, 1.0, 0.0))
    shrink = random.randint(0, 5)
    th, tw = h - shrink, w - shrink
    top = left = 0
    if shrink:  # tf.RandomCrop.get_params draws the corner from the torch generator, row first
        top = int(torch.randint(0, h - th + 1, size=(1,)).item())
        left = int(torch.randint(0, w - tw + 1, size=(1,)).item())
    factors, order = draw_color_jitter(*JITTER_RANGES)
    return ImageParams(h, w, top, left, th, tw, True, order, factors)


def apply_image_params(frames, masks, p: ImageParams):
    """uint8 frames (T,Hs,Ws,3) and masks (T,Hs,Ws) of a window -> (T,3,h,w) images, (T,1,h,w) binary masks, on the host
    in fp32: ToTensor + one bilinear resize of the whole window, the crop resized back, the jitter.  Masks may be the
    file's float values or the device mode's uint8 `mask != 0`: raw masks are non-negative, so both are non-zero at
    the same output pixels."""
    if isinstance(masks, torch.Tensor):
        masks = masks.numpy()
    if isinstance(frames, torch.Tensor):
        frames = frames.numpy()
    video = _resize(_to_tensor(frames), p.h, p.w)
    mask = _resize(_to_tensor(masks.astype(np.float32)), p.h, p.w)
    if p.jitter or (p.th, p.tw) != (p.h, p.w):
        window = (slice(None), slice(None), slice(p.top, p.top + p.th), slice(p.left, p.left + p.tw))
        video = _resize(video[window], p.h, p.w)
        mask = _resize(mask[window], p.h, p.w)
    if p.jitter:
        video = color_jitter(p.factors, p.order)(video)
    return video, mask.type(torch.bool).type(torch.float32)


# --------------------------------------------------------------------------- #
# numeric preprocessing: one table entry per robot viewpoint, whole-trajectory array ops
# --------------------------------------------------------------------------- #
# The reference spreads this over per-item methods with per-robot branches (robonet_dataset.py:173-256,300-432).  Here
# the branches are DATA: a `Viewpoint` says where a robot's bounds come from and how its stored end-effector positions
# become metric world positions; `NumericPipeline` then maps the (T, .) arrays of a whole window at once.  The
# floating-point expressions keep the reference's order of operations in float32 (tests/golden/dataset_item.npz pins
# them bit for bit).
WORKSPACE_BOX = (np.array([0.015, -0.3, 0.1, 0, 0], dtype=np.float32),      # robonet_dataset.py:203-207: the planner's
                 np.array([0.55, 0.3, 0.4, 1, 1], dtype=np.float32))         # workspace for the authors' own robots
FRANKA_TO_LOCOBOT_XY = np.array([-0.365, -0.06103333])                       # LOCO_FRANKA_DIFF, robonet_dataset.py:21
FRANKA_PUSH_HEIGHT = 0.14


class Viewpoint:
    """What distinguishes one robot viewpoint's numeric preprocessing (robonet_dataset.py:200-208,305-322)."""
    __slots__ = ("name", "file_bounds", "stored_metric", "shift_xy", "fixed_z", "default_robot")

    def __init__(self, name: str):
        self.name = name
        own_rig = "locobot" in name or "franka" in name
        self.file_bounds = not own_rig       # RoboNet files carry low_bound / high_bound; the authors' rigs use the box
        self.stored_metric = own_rig         # RoboNet stores NORMALISED eef positions, the authors' rigs metric ones
        franka = "franka" in name and "locobot" not in name
        self.shift_xy = FRANKA_TO_LOCOBOT_XY if franka else None
        self.fixed_z = FRANKA_PUSH_HEIGHT if franka else None
        self.default_robot = "locobot" if "locobot" in name else ("franka" if "franka" in name else None)

    def bounds(self, traj):
        if self.file_bounds:
            return traj["low_bound"][:], traj["high_bound"][:]
        return WORKSPACE_BOX[0].copy(), WORKSPACE_BOX[1].copy()

    def metric_eef(self, states, low, high):
        """(T, 3) end-effector positions in the metric world frame, as a view / copy of states[:, :3]."""
        eef = states[:, :3]
        if not self.stored_metric:
            return denormalize(eef, low[:3], high[:3])
        if self.shift_xy is not None:
            eef[:, :2] += self.shift_xy
            eef[:, 2] = self.fixed_z
        return eef


def _homogeneous(points):
    """(n, 3) -> (4, n) homogeneous columns (float64, as np.ones promotes in the reference)."""
    return np.concatenate([points, np.ones((points.shape[0], 1))], 1).T


def _apply(matrix, points):
    return (matrix @ _homogeneous(points)).T[:, :3]


def fit_width(x, width):
    """Zero-pad the last axis of a (T, d) array up to `width` (robonet_dataset.py:209-229)."""
    if x.shape[-1] == width:
        return x
    assert width > x.shape[-1]
    return np.pad(x, [(0, 0), (0, width - x.shape[-1])])


def imputed_gripper_actions(actions, next_gripper, g_low, g_high):
    """`--impute_autograsp_action`: append the gripper command implied by the NEXT state's gripper reading, open / closed
    around the midpoint of its bounds (robonet_dataset.py:181-190), for all steps at once."""
    mid = (g_high + g_low) / 2.0
    cmd = np.where(next_gripper > mid, g_high, g_low).astype(np.float64)[:, None]
    return np.concatenate((actions, cmd), axis=-1)


class NumericPipeline:
    """Bounds, states and actions of one viewpoint under one `--preprocess_action` strategy, for whole windows."""

    def __init__(self, viewpoint: str, strategy: str):
        self.view = Viewpoint(viewpoint)
        self.strategy = strategy
        self.camera = "camera" in strategy
        self.w2c = self.c2w = None
        if self.camera:
            w2c, c2w = _camera_dicts()
            self.w2c, self.c2w = w2c[viewpoint], c2w[viewpoint]

    def bounds(self, raw_low, raw_high):
        """Camera strategies normalise in the camera frame: the box's 8 corners are transformed and re-boxed
        (robonet_dataset.py:231-255)."""
        low, high = raw_low.copy(), raw_high.copy()
        if self.camera:
            corners = np.array([[x, y, z] for x in (low[0], high[0]) for y in (low[1], high[1]) for z in (low[2], high[2])])
            cam = _apply(self.w2c, corners)
            low[:3], high[:3] = cam.min(0), cam.max(0)
        return low, high

    def states(self, states, low, high):
        """Stored states -> states normalised by (low, high), positions in the strategy's frame."""
        out = states.copy()
        eef = self.view.metric_eef(out, low, high)
        if self.camera:
            eef = _apply(self.w2c, eef)
        out[:, :3] = normalize(eef, low[:3], high[:3])
        out[:, 4] = normalize(out[:, 4], low[4], high[4])
        return out

    def actions(self, norm_states, actions, low, high):
        if self.strategy == "raw":
            return torch.from_numpy(actions)
        if self.strategy != "camera_raw":
            raise NotImplementedError(self.strategy)  # state_infer / camera_state_infer: as the reference
        # displacement of the eef in the camera frame.  The reference zeroes the recorded actions first
        # (robonet_dataset.py:383-384), so the "next" position equals the current one: kept, it is its arithmetic.
        out = np.zeros_like(actions)
        world = _apply(self.c2w, denormalize(norm_states[:, :3], low[:3], high[:3]))[:-1]
        out[:, :3] = _apply(self.w2c, world + out[:, :3]) - _apply(self.w2c, world)
        return torch.from_numpy(out)


class ImagePipeline:
    """uint8 frames / float masks of a window -> (T, C, h, w) tensors (robonet_dataset.py:257-300): ToTensor + bilinear
    resize of the whole window in one call; with augmentation one crop and one colour jitter per trajectory."""

    def __init__(self, height: int, width: int, augment: bool):
        self.h, self.w, self.augment = height, width, augment

    def draw(self) -> ImageParams:
        return draw_image_params(self.h, self.w, self.augment)

    def __call__(self, frames, masks):
        return apply_image_params(frames, masks, self.draw())


class RoboNetDataset(data.Dataset):
    """Trajectory files -> the reference's item dict (robonet_dataset.py:23-171): images (T,3,h,w) in [0,1], states (T,R)
    normalised, actions (T-1,A), masks (T,1,h,w) in {0,1}, qpos (T,Q), robot, folder, file_path, idx (+ low / high /
    raw_* for finetune_* experiments, high_movement with --load_movement_info; low / high / heatmap_view with
    --model_use_heatmap, from which `process_batch` makes the batch's `heatmaps` on the device).

    `device_images=True`: instead of `images` / `masks` an item carries what the device needs to make them
    (`rac_image_pipeline`, through `collate` and `process_batch` / the prefetcher): `frames` uint8 (T,Hs,Ws,3) as
    stored, `raw_masks` uint8 (T,Hs,Ws) = `mask != 0` (raw masks are non-negative, so the resized mask is non-zero
    exactly where the resized `mask != 0` is) and `image_params`, the `ImageParams` drawn for this trajectory from the
    same random streams at the same point.  Every other key, the window sampling and the `preload_ram` cache are
    unchanged; a cached item keeps its parameters as a cached host item keeps its augmented frames."""

    def __init__(self, hdf5_list, robot_list, config, augment_img=False, load_snippet=False, rng_seed=None,
                 device_images=False):
        self._traj_names, self._traj_robots = hdf5_list, robot_list
        self._config = config
        self._device_images = bool(device_images)
        self._data_root = config.data_root
        self._video_length = (config.n_past + config.n_future) if load_snippet else config.video_length
        self._action_dim = config.action_dim
        self._impute = getattr(config, "impute_autograsp_action", False)
        self._images = ImagePipeline(config.image_height, config.image_width, augment_img)
        self._pipelines = {}
        # window starts: the reference's RandomState(config.seed); data-parallel ranks pass their own seed
        self._rng = np.random.RandomState(config.seed if rng_seed is None else rng_seed)
        self._movement = self._movement_tables() if config.load_movement_info else None
        self._heatmaps = bool(getattr(config, "model_use_heatmap", False))
        self._camera_table = None  # heatmaps.CameraTable, read on the first item under --model_use_heatmap
        self._memory = {}
        if getattr(config, "preload_ram", False):
            self._memory = {i: self[i] for i in range(len(self))}

    def __len__(self):
        return len(self._traj_names)

    def _movement_tables(self):
        """folder -> {file path: high-movement flag} (obj_movement.pkl next to the trajectories, :36-48)."""
        tables = {}
        for folder_path in {os.path.dirname(n) for n in self._traj_names}:
            with open(os.path.join(folder_path, "obj_movement.pkl"), "rb") as f:
                tables[os.path.basename(folder_path)] = pickle.load(f)
        return tables

    def pipeline(self, viewpoint: str) -> NumericPipeline:
        pipe = self._pipelines.get(viewpoint)
        if pipe is None:
            pipe = self._pipelines[viewpoint] = NumericPipeline(viewpoint, self._config.preprocess_action)
        return pipe

    def camera_table(self):
        if self._camera_table is None:
            from .heatmaps import CameraTable
            self._camera_table = CameraTable.from_config(self._config)
        return self._camera_table

    def _window(self, length: int, path: str):
        assert length >= self._video_length, f"{length}, {path}"
        if length == self._video_length:
            return 0, length
        start = self._rng.randint(0, length - self._video_length + 1)
        return start, start + self._video_length

    def read_actions(self, traj, start, end, g_low, g_high):
        """(end - start, A) float32 actions of the window; files with one dimension less get the imputed gripper
        command when `--impute_autograsp_action` is set."""
        actions = traj["actions"][:].astype(np.float32)
        have = actions.shape[1]
        if have != self._action_dim:
            if not (self._impute and have + 1 == self._action_dim):
                raise ValueError(f"file adim {have}, target adim {self._action_dim}")
            actions = imputed_gripper_actions(actions, traj["states"][:][1:, -1], g_low, g_high).astype(np.float32)
        return actions[start:end]

    def stored_numerics(self, traj, pipe, s, e):
        """What the numeric half reads of frames [s, e) of an open trajectory: (raw_low, raw_high, raw_states (e - s, R),
        raw_actions (e - s - 1, A), qpos (e - s, J), robot)."""
        cf = self._config
        raw_low, raw_high = pipe.view.bounds(traj)
        raw_states = fit_width(traj["states"][s:e].astype(np.float32), cf.robot_dim)
        raw_actions = self.read_actions(traj, s, e - 1, raw_low[4], raw_high[4])
        qpos = fit_width(traj["qpos"][s:e].astype(np.float32), cf.robot_joint_dim)
        robot = traj.attrs["robot"] if "robot" in traj.attrs else pipe.view.default_robot
        robot = robot.decode() if isinstance(robot, bytes) else str(robot)
        return raw_low, raw_high, raw_states, raw_actions, qpos, robot

    def numerics(self, pipe, stored, folder, path):
        """The numeric keys of an item from `stored_numerics` of its frames: states, actions, qpos (+ low / high /
        heatmap_view, raw_*, high_movement as the flags ask).  Every step works row by row, so the rows of a window are
        the same bits whether the window or the whole video is handed in (the device-resident split relies on it)."""
        cf = self._config
        raw_low, raw_high, raw_states, raw_actions, qpos, robot = stored
        if self._heatmaps and pipe.camera:
            # the heatmap projects WORLD-frame positions; the camera strategies normalise the states in the camera frame
            # (the reference's own open TODO, robonet_dataset.py:132-135 "need to account for camera space state")
            raise NotImplementedError(f"model_use_heatmap with preprocess_action={cf.preprocess_action!r}: the states are "
                                      f"in the camera frame, the heatmap needs them in the world frame")
        low, high = pipe.bounds(raw_low, raw_high)
        states = pipe.states(raw_states, low, high)
        actions = pipe.actions(states, raw_actions, low, high)
        out = {"states": states, "actions": actions, "qpos": qpos}
        if self._heatmaps:  # what rac_eef_heatmaps needs of this video: its bounds and its camera
            out["low"], out["high"] = low, high
            out["heatmap_view"] = self.camera_table().view_row(robot, folder, cf.image_height, cf.image_width).copy()
        if "finetune" in cf.experiment:  # the robot model of finetune_* windows needs the bounds (:148-166)
            out["low"], out["high"] = low, high
            if cf.preprocess_action != "raw":
                if not pipe.camera:
                    raise NotImplementedError
                world = raw_states.copy()  # world-frame states, normalised by the file's own bounds
                world[:, :3] = normalize(world[:, :3], raw_low[:3], raw_high[:3])
                world[:, 4] = normalize(world[:, 4], raw_low[4], raw_high[4])
                out.update(raw_low=raw_low, raw_high=raw_high, raw_actions=raw_actions.copy(), raw_states=world)
        if self._movement is not None:
            out["high_movement"] = self._movement[folder][path]
        return out

    def __getitem__(self, idx):
        if idx in self._memory:
            return self._memory[idx]
        name, viewpoint = self._traj_names[idx], self._traj_robots[idx]
        path = os.path.join(self._data_root, name)
        pipe = self.pipeline(viewpoint)
        with open_trajectory(path) as traj:
            frames_key, masks_key = picture_keys(traj, path)
            s, e = self._window(traj[frames_key].shape[0], path)
            frames = traj[frames_key][s:e]
            masks = traj[masks_key][s:e]
            masks = (masks != 0).astype(np.uint8) if self._device_images else masks.astype(np.float32)
            stored = self.stored_numerics(traj, pipe, s, e)
        raw_states, raw_actions, robot = stored[2], stored[3], stored[5]
        if not len(frames) == len(raw_states) == len(raw_actions) + 1 == len(masks):
            raise AssertionError(f"{path}, {frames.shape}, {raw_states.shape}, {raw_actions.shape}, {masks.shape}")
        folder = os.path.basename(os.path.dirname(name))
        if self._heatmaps and pipe.camera:
            self.numerics(pipe, stored, folder, path)  # (raises, before anything is drawn)
        if self._device_images:
            check_raw_frames(frames, path)
            pictures = {"frames": torch.from_numpy(np.ascontiguousarray(frames))}
            mask_keys = {"raw_masks": torch.from_numpy(masks), "image_params": self._images.draw()}
        else:
            images, masks = self._images(frames, masks)
            pictures, mask_keys = {"images": images}, {"masks": masks}
        rest = self.numerics(pipe, stored, folder, path)
        return {**pictures, "states": rest.pop("states"), "actions": rest.pop("actions"), **mask_keys, "robot": robot,
                "folder": folder, "file_path": path, "idx": idx, "qpos": rest.pop("qpos"), **rest}


def picture_keys(traj, path):
    """The names of a trajectory file's frames and masks (RoboNet's `frames` / `mask`, the authors' rigs'
    `observations` / `masks`)."""
    frames_key = "observations" if "observations" in traj else "frames"
    assert frames_key in traj, path
    return frames_key, "masks" if "masks" in traj else "mask"


def check_raw_frames(frames, path):
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] != 3:
        raise ValueError(f"{path}: device_images needs uint8 (T,H,W,3) frames, got {frames.dtype} {frames.shape}")


# --------------------------------------------------------------------------- #
# loaders (robonet_dataloaders.py:21-80, 137-199)
# --------------------------------------------------------------------------- #
def _robot_files(config, subdir, train_dirs, label, keep=None):
    """`keep(folder_name, path)`: an optional predicate on the discovered files (`create_movement_loader`)."""
    files, labels = [], []
    data_path = os.path.join(config.data_root, subdir)
    if not os.path.isdir(data_path):
        return []
    for folder in os.scandir(data_path):
        if folder.is_dir() and folder.name in train_dirs:
            for d in os.scandir(folder.path):
                if (d.is_file() and d.path.lower().endswith(TRAJ_EXTENSIONS)
                        and (keep is None or keep(folder.name, d.path))):
                    files.append(d.path)
                    labels.append(f"{label}_{folder.name}")
    fl = sorted(zip(files, labels), key=lambda x: x[0])
    random.seed(config.seed)
    random.shuffle(fl)
    return fl


def split_files(config):
    """The reference's discovery + shuffle + `train_test_split` (non-stratified): (X_train, X_test, y_train, y_test)."""
    from sklearn.model_selection import train_test_split
    fl = (_robot_files(config, "baxter_views", BAXTER_TRAIN_DIRS, "baxter")
          + _robot_files(config, "widowx_views", WIDOWX_TRAIN_DIRS, "widowx")
          + _robot_files(config, "sawyer_views", SAWYER_TRAIN_DIRS, "sawyer"))
    random.seed(config.seed)
    random.shuffle(fl)
    files, labels = [x[0] for x in fl], [x[1] for x in fl]
    return train_test_split(files, labels, test_size=1 - config.train_val_split,
                            random_state=np.random.RandomState(config.seed))


RAW_IMAGE_KEYS = ("frames", "raw_masks", "image_jobs", "image_shape")  # of a collated device_images batch
IMAGE_JOB = np.dtype(_lib.ImageJob)  # struct rac_image_job as a numpy record


def collate(items):
    """Default collation of the item dicts (tensors / arrays stacked, strings listed), images already float.
    Items of a `device_images` dataset: their raw videos may differ in size (RoboNet's 240x320 next to the authors' own
    rigs), so the bytes of all `frames` go into ONE flat uint8 buffer, all `raw_masks` into another, and `image_jobs`
    (B, sizeof(rac_image_job)) uint8 holds one job per video: its byte offsets into the two buffers, its (Hs, Ws) and
    its `ImageParams`; `image_shape` = (T, h, w)."""
    if isinstance(items[0], ResidentChoice):
        return items[0].store.collate(items)
    if "frames" not in items[0]:
        return data.default_collate(items)
    out = data.default_collate([{k: v for k, v in it.items() if k not in ("frames", "raw_masks", "image_params")}
                                for it in items])
    p0, T = items[0]["image_params"], items[0]["frames"].shape[0]
    jobs = np.zeros(len(items), IMAGE_JOB)
    f_off = m_off = 0
    for job, it in zip(jobs, items):
        fr, mk, p = it["frames"], it["raw_masks"], it["image_params"]
        if fr.shape[0] != T or tuple(mk.shape) != tuple(fr.shape[:3]) or (p.h, p.w) != (p0.h, p0.w):
            raise ValueError(f"device_images batch: {tuple(fr.shape)} frames, {tuple(mk.shape)} masks, T {T}")
        job["frame_offset"], job["mask_offset"] = f_off, m_off
        job["Hs"], job["Ws"] = fr.shape[1], fr.shape[2]
        job["top"], job["left"], job["th"], job["tw"] = p.top, p.left, p.th, p.tw
        job["order"], job["factor"], job["jitter"] = p.order, p.factors, int(p.jitter)
        f_off += fr.numel()
        m_off += mk.numel()
    out["frames"] = torch.cat([it["frames"].reshape(-1) for it in items])
    out["raw_masks"] = torch.cat([it["raw_masks"].reshape(-1) for it in items])
    out["image_jobs"] = torch.from_numpy(jobs.view(np.uint8).reshape(len(items), IMAGE_JOB.itemsize))
    out["image_shape"] = torch.tensor([T, p0.h, p0.w])
    return out


def _image_jobs(batch):
    """The job records of a collated device_images batch, checked against the buffers they index."""
    jobs = batch["image_jobs"].numpy().reshape(-1).view(IMAGE_JOB)
    T, h, w = (int(v) for v in batch["image_shape"])
    store = batch.get(RESIDENT_KEY)  # (a resident batch indexes its store's buffers)
    n_frames, n_masks = ((store.frames.numel(), store.raw_masks.numel()) if store is not None
                         else (batch["frames"].numel(), batch["raw_masks"].numel()))
    for j in jobs:
        n = T * int(j["Hs"]) * int(j["Ws"])
        ok = (j["Hs"] >= 1 and j["Ws"] >= 1 and j["frame_offset"] >= 0 and j["mask_offset"] >= 0
              and j["frame_offset"] + 3 * n <= n_frames and j["mask_offset"] + n <= n_masks
              and j["th"] >= 1 and j["tw"] >= 1 and j["top"] >= 0 and j["left"] >= 0
              and j["top"] + j["th"] <= h and j["left"] + j["tw"] <= w and sorted(j["order"]) == [0, 1, 2, 3])
        if not ok:
            raise ValueError(f"device_images batch: job {j} does not fit its buffers / the {h}x{w} model size")
    return jobs, T, h, w


def host_images(batch):
    """`images` (B,T,3,h,w) / `masks` (B,T,1,h,w) of a collated device_images batch by the HOST pipeline
    (`apply_image_params` per video): what the batch would have held with device_images off, bit for bit."""
    jobs, T, h, w = _image_jobs(batch)
    frames, masks = batch["frames"].numpy(), batch["raw_masks"].numpy()
    images, out_masks = [], []
    for j in jobs:
        im, mk = apply_image_params(*job_video(j, frames, masks, T), job_params(j, h, w))
        images.append(im)
        out_masks.append(mk)
    return torch.stack(images), torch.stack(out_masks)


def job_params(j, h, w) -> ImageParams:
    """The `ImageParams` a job record was made from."""
    return ImageParams(h, w, int(j["top"]), int(j["left"]), int(j["th"]), int(j["tw"]), bool(j["jitter"]),
                       tuple(int(k) for k in j["order"]), tuple(float(f) for f in j["factor"]))


def job_video(j, frames, masks, T):
    """A job's (T,Hs,Ws,3) frames and (T,Hs,Ws) masks as views of the flat numpy buffers."""
    Hs, Ws, n = int(j["Hs"]), int(j["Ws"]), T * int(j["Hs"]) * int(j["Ws"])
    return (frames[j["frame_offset"]:j["frame_offset"] + 3 * n].reshape(T, Hs, Ws, 3),
            masks[j["mask_offset"]:j["mask_offset"] + n].reshape(T, Hs, Ws))


def _pinned(t):
    return t if t.is_pinned() else t.pin_memory()


def device_images(batch, device):
    """Time-first `images` (T,B,3,h,w) / `masks` (T,B,1,h,w) of a collated device_images batch on `device`: the raw
    buffers and the job array are uploaded and ONE `rac_image_pipeline` launch does the rest, all on the current
    stream.  Also returns the tensors that launch reads (host and device), for the caller to keep until it has run."""
    jobs, T, h, w = _image_jobs(batch)
    host = [t if t.is_pinned() else t.pin_memory() for t in (batch["frames"], batch["raw_masks"], batch["image_jobs"])]
    frames, masks, jobs_dev = (t.to(device, non_blocking=True) for t in host)
    B = len(jobs)
    images = torch.empty(T, B, 3, h, w, device=device)
    out_masks = torch.empty(T, B, 1, h, w, device=device)
    _lib.call("rac_image_pipeline", _lib.ptr(frames), _lib.ptr(masks), _lib.ptr(jobs_dev), _lib.ptr(images),
              _lib.ptr(out_masks), B, T, h, w, _lib.stream_ptr())
    return images, out_masks, host + [frames, masks, jobs_dev]


def _dist_info():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


def create_loaders(config):
    """robonet_dataloaders.py:21-80.  Under torch.distributed (one process per GPU) the TRAIN loader shards the files
    with a DistributedSampler (same seed on every rank: disjoint shards of one shuffle, reshuffled per epoch through
    `set_epoch`, which `get_batch` calls) and each rank draws its own window starts; otherwise the ranks would train
    on identical batches and the gradient all-reduce would average copies of one gradient."""
    X_train, X_test, y_train, y_test = split_files(config)
    world, rank = _dist_info()
    return _split_loaders(config, (X_train, y_train), (X_test, y_test))


def _dataset(files, labels, config, augment=False, rng_seed=None):
    """The dataset of one split under the config's flags: `RoboNetDataset` with `--device_images` honoured, behind a
    `ResidentDataset` over its device-resident store with `--device_resident True`."""
    resident = getattr(config, "device_resident", False)
    if resident and getattr(config, "preload_ram", False):
        raise ValueError("--preload_ram True and --device_resident True: the split is kept either in host memory or on the "
                         "device, not both")
    ds = RoboNetDataset(files, labels, config, augment_img=augment and getattr(config, "img_augmentation", False),
                        rng_seed=rng_seed, device_images=resident or getattr(config, "device_images", False))
    if resident:
        ds = ResidentDataset(ds, ResidentVideos(ds, config.device, getattr(config, "device_resident_max_gb", 16.0)))
    return ds


def _threads(ds, config):
    """A resident dataset only draws numbers: its loader never has workers (they would each copy the random streams)."""
    return 0 if isinstance(ds, ResidentDataset) else config.data_threads


def _split_loaders(config, train, test, test_shuffle=True):
    """(train loader, test loader) over (files, labels) pairs, by `create_loaders`' conventions: the train split
    augmented under `--img_augmentation`, sharded by a DistributedSampler under torch.distributed with a window-start
    seed per rank, both loaders shuffled by generators seeded with the config seed."""
    world, rank = _dist_info()
    train_data = _dataset(*train, config, augment=True, rng_seed=config.seed + rank if world > 1 else None)
    test_data = _dataset(*test, config)
    threads = _threads(train_data, config)
    common = dict(num_workers=threads, drop_last=False, pin_memory=True, collate_fn=collate,
                  persistent_workers=threads > 0)
    if world > 1:
        sampler = data.distributed.DistributedSampler(train_data, num_replicas=world, rank=rank, shuffle=True,
                                                      seed=config.seed)
        train = data.DataLoader(train_data, batch_size=config.batch_size, sampler=sampler, **common)
    else:
        train = data.DataLoader(train_data, batch_size=config.batch_size, shuffle=True,
                                generator=torch.Generator().manual_seed(config.seed), **common)
    test = data.DataLoader(test_data, batch_size=config.test_batch_size, shuffle=test_shuffle,
                           generator=torch.Generator().manual_seed(config.seed), **common)
    return train, test


LOCOBOT_FOLDERS = ["c0", "c1", "c2", "c3"]  # locobot_singleview_dataloader.py:11


def _locobot_files(config):
    """<data_root>/locobot_views/c{0..3}/*.hdf5 (or .npz), sorted then shuffled with the config seed; labels in discovery
    order, as the reference pairs them (locobot_singleview_dataloader.py:63-75)."""
    files, labels = [], []
    for folder in LOCOBOT_FOLDERS:
        path = os.path.join(config.data_root, "locobot_views", folder)
        if not os.path.isdir(path):
            continue
        for d in os.scandir(path):
            if d.is_file() and d.path.lower().endswith(TRAJ_EXTENSIONS):
                files.append(d.path)
                labels.append("locobot_" + folder)
    files = sorted(files)
    random.seed(config.seed)
    random.shuffle(files)
    return files, labels


def _plain_loader(ds, config, batch_size):
    threads = _threads(ds, config)
    return data.DataLoader(ds, num_workers=threads, batch_size=batch_size, shuffle=True, drop_last=False,
                           pin_memory=True, generator=torch.Generator().manual_seed(config.seed), collate_fn=collate,
                           persistent_workers=threads > 0)


MOVEMENT_FILE = "obj_movement.pkl"  # per viewpoint folder: {file path: high-movement flag}, written by movement.py


def load_movement_table(folder_path):
    """The table of one viewpoint folder; a folder that has not been scored names the command that scores it."""
    path = os.path.join(folder_path, MOVEMENT_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found: score the folder's videos first with "
                                f"`python -m src.prediction.measure_obj_movement --data_root ...`")
    with open(path, "rb") as f:
        return pickle.load(f)


def _movement_files(config, subdir, train_dirs, label):
    """`_robot_files` restricted to the files whose table entry is true (robonet_dataloaders.py:210-292)."""
    data_path = os.path.join(config.data_root, subdir)
    if not os.path.isdir(data_path):
        return []
    tables = {f.name: load_movement_table(f.path) for f in os.scandir(data_path) if f.is_dir() and f.name in train_dirs}
    return _robot_files(config, subdir, train_dirs, label, keep=lambda name, path: bool(tables[name].get(path, False)))


def movement_files(config, n_files: int = 4000):
    """(files, labels) of `create_movement_loader`: per robot the flagged files sorted by path and shuffled after
    `random.seed(config.seed)`, baxter + widowx + sawyer concatenated, reseeded and shuffled again, the first `n_files`."""
    fl = (_movement_files(config, "baxter_views", BAXTER_TRAIN_DIRS, "baxter")
          + _movement_files(config, "widowx_views", WIDOWX_TRAIN_DIRS, "widowx")
          + _movement_files(config, "sawyer_views", SAWYER_TRAIN_DIRS, "sawyer"))
    random.seed(config.seed)
    random.shuffle(fl)
    fl = fl[:n_files]
    return [x[0] for x in fl], [x[1] for x in fl]


def create_movement_loader(config, n_files: int = 4000):
    """Loader over the high-movement videos only (robonet_dataloaders.py:295-327): up to 4000 files flagged true in
    their viewpoint folder's obj_movement.pkl, no augmentation, batches of `config.batch_size`."""
    files, labels = movement_files(config, n_files)
    return _plain_loader(_dataset(files, labels, config), config, config.batch_size)


def create_transfer_loader(config, n_files: int = 400):
    """Zero-shot evaluation set of `--experiment train_robonet`: up to 400 trajectories of the unseen locobot
    (locobot_singleview_dataloader.py:59-92).  None when the data root has no locobot_views folder."""
    files, labels = _locobot_files(config)
    if not files:
        return None
    return _plain_loader(_dataset(files[:n_files], labels[:n_files], config, augment=True), config, config.batch_size)


def create_finetune_loaders(config):
    """`--experiment finetune_locobot`: finetune_num_test files for testing, the next finetune_num_train for training
    (locobot_singleview_dataloader.py:12-57)."""
    files, labels = _locobot_files(config)
    return _head_split_loaders(config, files, labels, config.finetune_num_test, config.finetune_num_train)


def _head_split_loaders(config, files, labels, n_test, n_train, test_shuffle=True):
    """The first `n_test` files test, the next `n_train` train (the finetune_* and locobot rules)."""
    return _split_loaders(config, (files[n_test:n_test + n_train], labels[n_test:n_test + n_train]),
                          (files[:n_test], labels[:n_test]), test_shuffle)


# --------------------------------------------------------------------------- #
# one pair of loaders per --experiment (the reference trainer's _setup_data, trainer.py:899-947)
# --------------------------------------------------------------------------- #
# sawyer_dataloaders.py:13-16: the multiview experiment trains on every sawyer viewpoint but one and transfers to that one
SAWYER_MULTIVIEW_TRAIN_DIRS = [d for d in SAWYER_TRAIN_DIRS if d != "sudri2_c1"]
SAWYER_UNSEEN_VIEW = "sudri2_c1"


def high_movement_files(config, subdir, view):
    """The trajectory files of <data_root>/<subdir>/<view> in which the world moves, sorted by path and shuffled after
    `random.seed(config.seed)` (sawyer_dataloaders.py:18-35, widowx_dataloaders.py:10-28).  With `--world_error_dict` the
    filter is the reference's pickle {path: [{"high_error": bool}, ...]}: a file stays if any entry is true.  Without it,
    the folder's own obj_movement.pkl decides (`load_movement_table`)."""
    folder = os.path.join(config.data_root, subdir, view)
    paths = [d.path for d in os.scandir(folder) if d.is_file() and d.path.lower().endswith(TRAJ_EXTENSIONS)]
    if getattr(config, "world_error_dict", None):
        with open(config.world_error_dict, "rb") as f:
            motion_info = pickle.load(f)
        paths = [p for p in paths if any(x["high_error"] for x in motion_info[p])]
    else:
        table = load_movement_table(folder)
        paths = [p for p in paths if bool(table.get(p, False))]
    paths = sorted(paths)
    random.seed(config.seed)
    random.shuffle(paths)
    return paths


def _view_finetune_loaders(config, subdir, view, label):
    files = high_movement_files(config, subdir, view)
    return _head_split_loaders(config, files, [label] * len(files), config.finetune_num_test, config.finetune_num_train)


def create_widowx_finetune_loaders(config):
    """`--experiment finetune_widowx` (widowx_dataloaders.py:10-63): the high-movement videos of widowx1_c0."""
    return _view_finetune_loaders(config, "widowx_views", "widowx1_c0", "widowx_widowx1_c0")


def create_sawyer_finetune_loaders(config):
    """`--experiment finetune_sawyer_view` (sawyer_dataloaders.py:18-70): the high-movement videos of the sawyer
    viewpoint the multiview experiment never trains on."""
    return _view_finetune_loaders(config, "sawyer_views", SAWYER_UNSEEN_VIEW, "sawyer_" + SAWYER_UNSEEN_VIEW)


def create_sawyer_loaders(config):
    """`--experiment train_sawyer_multiview` (sawyer_dataloaders.py:126-190): the sawyer training viewpoints, one sort
    and seeded shuffle, `train_test_split` without stratification."""
    from sklearn.model_selection import train_test_split
    fl = _robot_files(config, "sawyer_views", SAWYER_MULTIVIEW_TRAIN_DIRS, "sawyer")
    X_train, X_test, y_train, y_test = train_test_split([x[0] for x in fl], [x[1] for x in fl],
                                                        test_size=1 - config.train_val_split,
                                                        random_state=np.random.RandomState(config.seed))
    return _split_loaders(config, (X_train, y_train), (X_test, y_test))


def create_sawyer_transfer_loader(config, n_files: int = 500):
    """Zero-shot set of `train_sawyer_multiview` (sawyer_dataloaders.py:83-124): the first 500 high-movement videos of the
    unseen viewpoint, of those the train part of `train_test_split`; no augmentation, batches of `test_batch_size`."""
    from sklearn.model_selection import train_test_split
    files = high_movement_files(config, "sawyer_views", SAWYER_UNSEEN_VIEW)[:n_files]
    labels = ["sawyer_" + SAWYER_UNSEEN_VIEW] * len(files)
    X_train, _, y_train, _ = train_test_split(files, labels, test_size=1 - config.train_val_split,
                                              random_state=np.random.RandomState(config.seed))
    return _plain_loader(_dataset(X_train, y_train, config), config, config.test_batch_size)


def create_locobot_loaders(config, n_test: int = 200, n_train: int = 3000):
    """`--experiment train_locobot_singleview` (locobot_singleview_dataloader.py:97-146): 200 videos test, the next 3000
    train; the test loader walks its files in order."""
    files, labels = _locobot_files(config)
    return _head_split_loaders(config, files, labels, n_test, n_train, test_shuffle=False)


def create_locobot_table_loaders(config, n_test: int = 1000, n_train: int = 10000):
    """`--experiment train_locobot_table` (locobot_table_dataloaders.py:95-144): <data_root>/locobot_table_views/c0, 1000
    videos test, the next 10000 train."""
    folder = os.path.join(config.data_root, "locobot_table_views", "c0")
    files = sorted(d.path for d in os.scandir(folder) if d.is_file() and d.path.lower().endswith(TRAJ_EXTENSIONS))
    random.seed(config.seed)
    random.shuffle(files)
    return _head_split_loaders(config, files, ["locobot_c0"] * len(files), n_test, n_train)


EXPERIMENT_LOADERS = {  # --experiment -> (train / test loaders, transfer loader or None)
    "train_robonet": (create_loaders, create_transfer_loader),
    "train_sawyer_multiview": (create_sawyer_loaders, create_sawyer_transfer_loader),
    "finetune_sawyer_view": (create_sawyer_finetune_loaders, None),
    "finetune_widowx": (create_widowx_finetune_loaders, None),
    "train_locobot_singleview": (create_locobot_loaders, None),
    "finetune_locobot": (create_finetune_loaders, None),
    "train_locobot_table": (create_locobot_table_loaders, None),
    # the stale value of published command lines (config.py: accepted, not in the reference's parser): the RoboNet
    # split it has always run on here, without the transfer set
    "singlerobot": (create_loaders, None),
}


def experiment_loaders(config, transfer: bool = True):
    """(train loader, test loader, transfer loader or None) of `config.experiment`, chosen as the reference's trainer
    chooses them (trainer.py:899-947); `transfer=False` leaves the transfer loader unbuilt.  An experiment it has no loaders for raises NotImplementedError, as there
    (`train_locobot_pick` among them: its simulated-pick dataset is not part of this package)."""
    if config.experiment not in EXPERIMENT_LOADERS:
        raise NotImplementedError(config.experiment)
    loaders, transfer_loader = EXPERIMENT_LOADERS[config.experiment]
    train, test = loaders(config)
    return train, test, (transfer_loader(config) if transfer and transfer_loader is not None else None)


# --------------------------------------------------------------------------- #
# --device_resident True: a split that lives on the device
# --------------------------------------------------------------------------- #
RESIDENT_KEY = "resident"                                     # of a collated resident batch: its ResidentVideos
RESIDENT_BATCH_KEYS = (RESIDENT_KEY, "image_jobs", "image_shape", "index", "start")  # gone once the batch is made
WINDOW_TABLES = ("states", "actions", "qpos", "raw_states", "raw_actions")            # (V, rows, width): a window each
STEP_TABLES = ("actions", "raw_actions")                                              # (a row per step: one fewer)
VIDEO_TABLES = ("low", "high", "raw_low", "raw_high")                                 # (V, width): one row per video


class ResidentChoice(NamedTuple):
    """What is drawn at random for one item of a resident split: the video, its window start and its `ImageParams`."""
    idx: int
    start: int
    params: ImageParams
    store: "ResidentVideos"


class ResidentVideos:
    """One split of a `RoboNetDataset` on the device, built once:
      * `frames` / `raw_masks`: every file's WHOLE stored video (uint8 (L_v, Hs, Ws, 3)) and `mask != 0` back to back in
        two flat uint8 buffers; the byte offsets, `shapes` (L_v, Hs, Ws) and the strings stay on the host;
      * `tables`: the numeric keys of an item, computed once per file by the dataset's `NumericPipeline` over the whole
        video, as fp32 tables padded to the longest video: states (V, Lmax, R), actions (V, Lmax - 1, A), qpos
        (V, Lmax, J), low / high (V, 5) (+ raw_* under finetune_* with a camera strategy); `lengths` int32 (V,);
      * `host_rows`, on the host: `heatmap_view` (17 float64 numbers per video under --model_use_heatmap: the rows are
        fp64 and rac_eef_heatmaps takes records packed on the host), `high_movement` under --load_movement_info (a host
        tensor in the batch dict either way) and bounds that a file stores as float64.
    A batch is then `collate` of B `ResidentChoice`s -> `device_batch`: the job array and an (index, start) pair per
    sample are uploaded, `rac_image_pipeline` reads the frames in place and `rac_window_gather` copies the windows."""

    def __init__(self, dataset: RoboNetDataset, device, max_gb: float = 16.0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.RacError(f"--device_resident True keeps the split on a GPU, not on {self.device} (no CPU fallback)")
        self.window = dataset._video_length
        paths, shapes = [], []
        for name in dataset._traj_names:  # sizes first: nothing is allocated for a split that does not fit
            path = os.path.join(dataset._data_root, name)
            with open_trajectory(path) as traj:
                fk, mk = picture_keys(traj, path)
                shape, mshape = tuple(traj[fk].shape), tuple(traj[mk].shape)
            if len(shape) != 4 or shape[3] != 3 or mshape != shape[:3] or shape[0] < self.window:
                raise ValueError(f"{path}: frames {shape}, masks {mshape} for a window of {self.window} (T,H,W,3) frames")
            paths.append(path)
            shapes.append(shape[:3])
        if not paths:
            raise ValueError("ResidentVideos: an empty split")
        self.paths, self.shapes = paths, np.array(shapes, np.int64)
        pixels = self.shapes.prod(1)
        self.mask_offsets = np.concatenate([[0], np.cumsum(pixels)])
        self.frame_offsets = 3 * self.mask_offsets
        cf = dataset._config
        V, Lmax = len(paths), int(self.shapes[:, 0].max())
        numeric = 4 * V * Lmax * (2 * (cf.robot_dim + cf.action_dim) + cf.robot_joint_dim + 20)  # (an upper bound)
        need = 4 * int(self.mask_offsets[-1]) + numeric
        if need > max_gb * 2 ** 30:
            raise ValueError(f"the split needs {need / 2 ** 30:.2f} GB on the device, above --device_resident_max_gb "
                             f"{max_gb:g}: raise the flag or train from the loaders")
        self.frames = torch.empty(int(self.frame_offsets[-1]), dtype=torch.uint8, device=self.device)
        self.raw_masks = torch.empty(int(self.mask_offsets[-1]), dtype=torch.uint8, device=self.device)
        rows, self.robots, self.folders = [], [], []
        for i, (path, name, viewpoint) in enumerate(zip(paths, dataset._traj_names, dataset._traj_robots)):
            pipe = dataset.pipeline(viewpoint)
            folder = os.path.basename(os.path.dirname(name))
            with open_trajectory(path) as traj:
                fk, mk = picture_keys(traj, path)
                frames, masks = traj[fk][:], traj[mk][:]
                stored = dataset.stored_numerics(traj, pipe, 0, len(frames))
            check_raw_frames(frames, path)
            if not len(frames) == len(stored[2]) == len(stored[3]) + 1 == len(masks) == len(stored[4]):
                raise AssertionError(f"{path}, {frames.shape}, {stored[2].shape}, {stored[3].shape}, {masks.shape}")
            f0, m0 = int(self.frame_offsets[i]), int(self.mask_offsets[i])
            self.frames[f0:f0 + frames.size].copy_(torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)))
            self.raw_masks[m0:m0 + masks.size].copy_(torch.from_numpy((masks != 0).astype(np.uint8).reshape(-1)))
            rows.append(dataset.numerics(pipe, stored, folder, path))
            self.robots.append(stored[5])
            self.folders.append(folder)
        self.lengths_host = self.shapes[:, 0].copy()
        self.lengths = torch.from_numpy(self.lengths_host.astype(np.int32)).to(self.device)
        self.tables, self.host_rows = {}, {}
        for k in rows[0]:
            first = np.asarray(rows[0][k])
            if k in WINDOW_TABLES:
                table = np.zeros((V, Lmax - (k in STEP_TABLES), first.shape[1]), np.float32)
            elif k in VIDEO_TABLES and first.dtype == np.float32:
                table = np.zeros((V, first.shape[0]), np.float32)
            else:  # fp64 camera rows, flags, bounds a file stores as float64: collated from the host, as the loader does
                self.host_rows[k] = [r[k] for r in rows]
                continue
            for i, r in enumerate(rows):
                a = np.asarray(r[k])
                if a.dtype != np.float32 or a.shape[1 if k in WINDOW_TABLES else 0:] != table.shape[2 if k in WINDOW_TABLES else 1:]:
                    raise ValueError(f"{paths[i]}: {k} {a.dtype} {a.shape} next to {first.dtype} {first.shape}")
                if k in WINDOW_TABLES:
                    table[i, :len(a)] = a
                else:
                    table[i] = a
            self.tables[k] = torch.from_numpy(table).to(self.device)
        torch.cuda.synchronize(self.device)

    def __len__(self):
        return len(self.paths)

    def nbytes(self) -> int:
        return (self.frames.numel() + self.raw_masks.numel()
                + sum(t.numel() * t.element_size() for t in self.tables.values()))

    def check(self, index, start):
        return check_windows(index, start, self.lengths_host, self.window)

    def collate(self, choices):
        """B `ResidentChoice`s -> the batch dict: one `rac_image_job` per sample pointing at its window inside the
        store's buffers, `image_shape`, int32 `index` / `start`, the strings, `idx`, and the store itself."""
        idx = [int(c.idx) for c in choices]
        index, start = self.check(idx, [int(c.start) for c in choices])
        p0 = choices[0].params
        jobs = np.zeros(len(choices), IMAGE_JOB)
        for job, c, i, s in zip(jobs, choices, index, start):
            p = c.params
            if (p.h, p.w) != (p0.h, p0.w):
                raise ValueError(f"resident batch: model sizes {(p.h, p.w)} and {(p0.h, p0.w)} in one batch")
            _, Hs, Ws = (int(v) for v in self.shapes[i])
            job["frame_offset"] = self.frame_offsets[i] + int(s) * Hs * Ws * 3
            job["mask_offset"] = self.mask_offsets[i] + int(s) * Hs * Ws
            job["Hs"], job["Ws"] = Hs, Ws
            job["top"], job["left"], job["th"], job["tw"] = p.top, p.left, p.th, p.tw
            job["order"], job["factor"], job["jitter"] = p.order, p.factors, int(p.jitter)
        out = {RESIDENT_KEY: self, "image_jobs": torch.from_numpy(jobs.view(np.uint8).reshape(len(choices), IMAGE_JOB.itemsize)),
               "image_shape": torch.tensor([self.window, p0.h, p0.w]), "index": torch.from_numpy(index),
               "start": torch.from_numpy(start), "robot": [self.robots[i] for i in idx],
               "folder": [self.folders[i] for i in idx], "file_path": [self.paths[i] for i in idx],
               "idx": torch.tensor(idx, dtype=torch.int64)}
        for k, per_video in self.host_rows.items():
            out[k] = data.default_collate([per_video[i] for i in idx])
        return out

    def gather(self, index, start, L=None):
        """Time-first windows of every table for int32 DEVICE tensors `index` / `start` the caller has checked
        (`check`): {states (L, B, R), actions (L - 1, B, A), qpos (L, B, J), low / high (B, 5), ...}, one
        `rac_window_gather` launch per 8 tables on the current stream."""
        L = self.window if L is None else int(L)
        return window_gather([(k, t, k in VIDEO_TABLES, L - (k in STEP_TABLES))
                              for k, t in self.tables.items()], index, start, self.lengths, L)

    def device_batch(self, batch):
        """`images`, `masks` and the numeric keys of a collated resident batch, time-first on the store's device, all on
        the current stream: the job array and the (index, start) pairs are uploaded, `rac_image_pipeline` reads the
        resident frames and `rac_window_gather` the resident tables.  Also returns the tensors the launches read that
        the store does not own, for the caller to keep until they have run."""
        jobs, T, h, w = _image_jobs(batch)
        index, start = self.check(batch["index"].numpy(), batch["start"].numpy())
        if T != self.window:
            raise ValueError(f"resident batch: windows of {T} frames from a store built for {self.window}")
        host = [_pinned(batch["image_jobs"]), _pinned(torch.from_numpy(np.stack([index, start])))]
        jobs_dev, pairs = (t.to(self.device, non_blocking=True) for t in host)
        B = len(jobs)
        images = torch.empty(T, B, 3, h, w, device=self.device)
        masks = torch.empty(T, B, 1, h, w, device=self.device)
        _lib.call("rac_image_pipeline", _lib.ptr(self.frames), _lib.ptr(self.raw_masks), _lib.ptr(jobs_dev),
                  _lib.ptr(images), _lib.ptr(masks), B, T, h, w, _lib.stream_ptr())
        out = self.gather(pairs[0], pairs[1], T)
        out.update(images=images, masks=masks)
        return out, host + [jobs_dev, pairs]


def check_windows(index, start, lengths, window):
    """The (index, start) pairs of a batch as int32 arrays, refused unless every window of `window` frames lies inside
    its video of `lengths[index]` frames: `rac_window_gather` and `rac_image_pipeline` read them from device memory,
    where their entry points cannot look."""
    index, start, lengths = np.asarray(index), np.asarray(start), np.asarray(lengths)
    if (index.ndim != 1 or index.shape != start.shape or not len(index)
            or not (np.issubdtype(index.dtype, np.integer) and np.issubdtype(start.dtype, np.integer))):
        raise ValueError(f"resident batch: one integer index and start per sample, got {index.shape} and {start.shape}")
    if index.min() < 0 or index.max() >= len(lengths):
        raise ValueError(f"resident batch: video index outside [0, {len(lengths)}): {index.tolist()}")
    if start.min() < 0 or np.any(start + window > lengths[index]):
        raise ValueError(f"resident batch: a window of {window} from {start.tolist()} leaves its video "
                         f"(lengths {lengths[index].tolist()})")
    return index.astype(np.int32), start.astype(np.int32)


def window_gather(tables, index, start, lengths, L):
    """`rac_window_gather` (include/rac_hip.h): for every (name, table, per_video, rows) of `tables` -- fp32 device
    tensors (V, rows_stored, width), or (V, width) when per_video -- the time-first windows
    out[name][r][b] = table[index[b]][start[b] + r] as (rows, B, width), or table[index[b]] as (B, width).  `index`,
    `start` (B,) and `lengths` (V,) are int32 device tensors; the CALLER has checked 0 <= index < V and
    0 <= start <= length - L (the entry point cannot read them)."""
    for t in (index, start, lengths):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.RacError("window_gather: index / start / lengths live on the GPU (no CPU fallback)")
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"window_gather: expected a contiguous int32 vector, got {t.dtype} {tuple(t.shape)}")
    B, V = int(index.shape[0]), int(lengths.shape[0])
    if start.shape[0] != B:
        raise ValueError(f"window_gather: {B} indices and {start.shape[0]} starts")
    out, records = {}, []
    for name, t, per_video, rows in tables:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.RacError(f"window_gather: table {name!r} lives on the GPU (no CPU fallback)")
        if (t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != (2 if per_video else 3) or t.shape[0] != V
                or t.device != index.device):
            raise ValueError(f"window_gather: table {name!r} must be contiguous fp32 ({V}, ...) on {index.device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
        width = int(t.shape[-1])
        dst = torch.empty((B, width) if per_video else (int(rows), B, width), device=t.device)
        out[name] = dst
        records.append((t.data_ptr(), dst.data_ptr(), 1 if per_video else int(t.shape[1]), width,
                        1 if per_video else int(rows), int(bool(per_video))))
    with torch.cuda.device(index.device):
        for k in range(0, len(records), _lib.GATHER_MAX_TABLES):
            part = records[k:k + _lib.GATHER_MAX_TABLES]
            array = (_lib.GatherTable * len(part))(*part)
            _lib.call("rac_window_gather", C.cast(array, C.c_void_p), len(part), _lib.ptr(index), _lib.ptr(start),
                      _lib.ptr(lengths), V, B, int(L), _lib.stream_ptr())
    return out


class ResidentDataset(data.Dataset):
    """The dataset of a resident loader: an item is what `RoboNetDataset.__getitem__` draws at random for it -- the
    window start from the dataset's RandomState, the `ImageParams` from its image pipeline, in that order, from the same
    streams -- and nothing else: no file is opened.  `collate` makes the batch from the choices and the store."""

    def __init__(self, dataset: RoboNetDataset, store: ResidentVideos):
        self.dataset, self.store = dataset, store

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        start, _ = self.dataset._window(int(self.store.lengths_host[idx]), self.store.paths[idx])
        return ResidentChoice(int(idx), int(start), self.dataset._images.draw(), self.store)


def _start_epoch(loader, epoch: int):
    sampler = getattr(loader, "sampler", None)
    if hasattr(sampler, "set_epoch"):
        sampler.set_epoch(epoch)


# --------------------------------------------------------------------------- #
# host -> device
# --------------------------------------------------------------------------- #
def process_batch(data: dict, device) -> dict:
    """Changes tensor idx from batch-first to time-first and moves it to `device` (robonet_dataset.py:434-451).
    A `device_images` batch gets its `images` / `masks` here: from `rac_image_pipeline` on a GPU, from the host pipeline
    on the CPU (the same tensors as with device_images off)."""
    if RESIDENT_KEY in data:  # a --device_resident batch: everything but the strings is made on the store's device
        store = data[RESIDENT_KEY]
        if torch.device(device).type != "cuda" or torch.device(device).index not in (None, store.device.index):
            raise _lib.RacError(f"a --device_resident batch of {store.device} cannot be made on {device} (no CPU fallback)")
        with torch.cuda.device(store.device):
            pictures, _ = store.device_batch(data)  # (the current stream orders the small uploads' reuse)
        for k in RESIDENT_BATCH_KEYS:
            del data[k]
    elif "frames" in data:
        if torch.device(device).type == "cuda":
            with torch.cuda.device(device):
                images, masks, _ = device_images(data, device)  # (the current stream orders the buffers' reuse)
        else:
            images, masks = (t.transpose(0, 1) for t in host_images(data))
        for k in RAW_IMAGE_KEYS:
            del data[k]
        pictures = {"images": images, "masks": masks}
    else:
        pictures = {}
    for k in TRANSPOSE_KEYS:
        if k in data:
            data[k] = data[k].transpose_(1, 0).to(device, non_blocking=True)
    data.update(pictures)
    if HEATMAP_VIEW_KEY in data:
        if torch.device(device).type != "cuda":
            raise _lib.RacError("model_use_heatmap: the heatmaps are made on the GPU (rac_eef_heatmaps; no CPU fallback)")
        with torch.cuda.device(device):
            data["heatmaps"] = device_heatmaps(data)
    return data


HEATMAP_VIEW_KEY = "heatmap_view"


def device_heatmaps(batch: dict, keep=None):
    """The time-first `heatmaps` (T, B, 1, H, W) of a `--model_use_heatmap` batch whose `states` are already time-first
    on the GPU: one `rac_eef_heatmaps` launch on the current stream.  Removes the batch's `heatmap_view`."""
    from .heatmaps import heatmaps_from_views
    rows = batch.pop(HEATMAP_VIEW_KEY).numpy()
    return heatmaps_from_views(batch["states"], batch["low"], batch["high"], rows, int(rows[0, 15]), int(rows[0, 16]),
                               keep=keep)


class DevicePrefetcher:
    """Iterates a loader one batch ahead: batch k+1 is copied (pinned memory -> HBM) on a side stream and transposed to
    time-first ON THE DEVICE while step k computes; `next()` makes the compute stream wait for that stream's event
    only.  A background thread keeps the (CPU-bound) loader iterator off the trainer's critical path."""

    def __init__(self, loader, device, depth: int = 2):
        self.loader, self.device = loader, torch.device(device)
        self.stream = torch.cuda.Stream(self.device)
        self.q: Queue = Queue(maxsize=depth)
        self._raw = []  # (event, tensors): raw image buffers of uploads whose kernel may not have run yet
        self._stop = False
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _upload(self, batch):
        out = dict(batch)
        raw = None
        with torch.cuda.stream(self.stream):
            made = ()
            if RESIDENT_KEY in out:  # a resident batch: the jobs and (index, start) go up, two launches make the tensors
                tensors, raw = out[RESIDENT_KEY].device_batch(out)  # (the store's buffers outlive every launch)
                for k in RESIDENT_BATCH_KEYS:
                    del out[k]
                out.update(tensors)
                made = tuple(tensors)
            elif "frames" in out:  # a device_images batch: upload the raw bytes + jobs, one launch makes images / masks
                out["images"], out["masks"], raw = device_images(out, self.device)
                for k in RAW_IMAGE_KEYS:
                    del out[k]
                made = ("images", "masks")
            for k in TRANSPOSE_KEYS:
                if k in out and k not in made:  # (those are time-first already)
                    t = out[k]
                    t = t if t.is_pinned() else t.pin_memory()
                    out[k] = t.to(self.device, non_blocking=True).transpose(0, 1).contiguous()
            if HEATMAP_VIEW_KEY in out:  # one launch behind the states' upload, on this stream
                held = []
                out["heatmaps"] = device_heatmaps(out, keep=held)
                raw = (raw, held)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        if raw is not None:  # keep what the launch reads until the event says it has run
            self._raw = [(e, r) for e, r in self._raw if not e.query()] + [(ev, raw)]
        return out, ev

    def _run(self):
        torch.cuda.set_device(self.device)
        try:
            epoch = 0
            while not self._stop:
                _start_epoch(self.loader, epoch)
                epoch += 1
                for batch in self.loader:
                    if self._stop:
                        return
                    self.q.put(self._upload(batch))
        except BaseException as e:  # surfaced by the consumer
            self.q.put(e)

    def __iter__(self):
        return self

    def __next__(self):
        item = self.q.get()
        if isinstance(item, BaseException):
            raise item
        batch, ev = item
        torch.cuda.current_stream(self.device).wait_event(ev)
        for k in TRANSPOSE_KEYS + VIDEO_TABLES:
            if k in batch and torch.is_tensor(batch[k]) and batch[k].is_cuda:
                batch[k].record_stream(torch.cuda.current_stream(self.device))
        return batch

    def close(self):
        self._stop = True
        while not self.q.empty():
            self.q.get_nowait()


def get_batch(loader, device, prefetch: bool = True):
    """Infinite batch generator for a dataloader (robonet_dataset.py:454-467); `prefetch`: through DevicePrefetcher."""
    if prefetch and torch.device(device).type == "cuda":
        yield from DevicePrefetcher(loader, device)
        return
    epoch = 0
    while True:
        _start_epoch(loader, epoch)
        epoch += 1
        for batch in loader:
            yield process_batch(batch, device)


class SyntheticVideoDataset(data.Dataset):
    """Batch-first synthetic videos in the dataset's item layout (images (T,3,H,W), masks (T,1,H,W), ...),
    for `--data_root synthetic` runs and dataloader plumbing tests."""

    def __init__(self, n: int, T: int, H: int = 64, W: int = 64, R: int = 5, A: int = 5, seed: int = 0):
        self.n, self.T, self.H, self.W, self.R, self.A, self.seed = n, T, H, W, R, A, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from .synthetic import synth_video
        v = synth_video(self.seed * 100003 + i, self.T, 1, self.H, self.W, self.R, self.A)
        out = {k: v[k][:, 0] for k in ("images", "masks", "states", "actions", "qpos")}
        out["robot"] = "sawyer"
        out["folder"] = "synthetic"
        return out
