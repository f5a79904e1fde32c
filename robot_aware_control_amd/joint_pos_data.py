"""Data path of the learned robot model's training (reference src/dataset/joint_pos_dataset.py and the two
`*_joint_pos_dataloaders.py`): (qpos, states, actions) windows of RoboNet trajectories, plus the masks the plot compares
its renders with.

Two forms of the same batches:
  * the host form -- `JointPosDataset`, `create_loaders`, `create_finetune_loaders`: the reference's public API, item for
    item, and what the tests compare against;
  * the device form -- `DeviceJointPosData` holds a whole split on the GPU in stored form (a few hundred bytes per
    trajectory; no masks) and `device_batches` yields the batches the host loader would yield, each made by ONE
    `rac_joint_batch` launch from an uploaded (index, window start) pair per sample.  `RobotPredictionTrainer` trains
    on this form.

Differences from the reference, on purpose: `.npz` trajectories next to `.hdf5` (data.open_trajectory); the baxter
loader filters by `--world_error_dict` only when that file is given, and not by the file name.
"""
from __future__ import annotations

import os
import pickle
import random
import zipfile

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.data as tdata

from . import ops
from .data import TRAJ_EXTENSIONS, _NpzTrajectory, open_trajectory

STRATEGIES = ("raw", "state_infer")
GRIP = 4  # the gripper-force column of a state


# --------------------------------------------------------------------------- #
# the image transform: tf.Compose([tf.ToTensor(), tf.CenterCrop(image_width)])
# --------------------------------------------------------------------------- #
def center_crop(t: torch.Tensor, size: int) -> torch.Tensor:
    """torchvision's CenterCrop(size) on (..., H, W): a side shorter than `size` is zero-padded first (the odd pixel goes
    right / below), the offsets are Python-rounded halves."""
    h, w = t.shape[-2:]
    if size > w or size > h:
        pw, ph = max(size - w, 0), max(size - h, 0)
        t = F.pad(t, [pw // 2, (pw + 1) // 2, ph // 2, (ph + 1) // 2])
        h, w = t.shape[-2:]
        if (h, w) == (size, size):
            return t
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    return t[..., top:top + size, left:left + size]


def mask_transform(masks, size: int) -> torch.Tensor:
    """ToTensor + CenterCrop(size) of a stack of (H, W) masks: (n, 1, size, size) float32; uint8 is scaled by 1 / 255."""
    arr = np.ascontiguousarray(np.stack([np.asarray(m) for m in masks]))
    if arr.ndim != 3:
        raise ValueError(f"masks must be (H, W) arrays, got {arr.shape[1:]}")
    t = torch.from_numpy(arr).unsqueeze(1)
    t = t.to(torch.float32).div(255) if t.dtype == torch.uint8 else t.to(torch.float32)
    return center_crop(t, size).contiguous()


# --------------------------------------------------------------------------- #
# the dataset (joint_pos_dataset.py:20-206)
# --------------------------------------------------------------------------- #
def episode_length(traj, path: str) -> int:
    """Rows of the file's `frames` (joint_pos_dataset.py:67) without reading them."""
    if isinstance(traj, _NpzTrajectory):
        with zipfile.ZipFile(path) as z, z.open("frames.npy") as f:
            major, _ = np.lib.format.read_magic(f)
            read = np.lib.format.read_array_header_1_0 if major == 1 else np.lib.format.read_array_header_2_0
            return int(read(f)[0][0])
    return int(traj["frames"].shape[0])


def _text(attr) -> str:
    return attr.decode() if isinstance(attr, bytes) else str(attr)


def draw_start(rng, ep_len: int, window: int) -> int:
    """joint_pos_dataset.py:69-74: a draw only when the episode is longer than the window."""
    return int(rng.randint(0, ep_len - window + 1)) if ep_len > window else 0


class JointPosDataset(tdata.Dataset):
    def __init__(self, hdf5_list, robot_list, config, augment_img=False, load_snippet=False):
        self._traj_names = list(hdf5_list)
        self._traj_robots = list(robot_list)
        self._config = config
        self._data_root = config.data_root
        self._video_length = config.n_past + config.n_future if load_snippet else config.video_length
        self._action_dim = config.action_dim
        self._impute_autograsp_action = config.impute_autograsp_action
        self._augment_img = augment_img  # (unused, as in the reference)
        self._rng = np.random.RandomState(config.seed)
        self._lengths = None
        self._robots = {}

    def __len__(self):
        return len(self._traj_names)

    @property
    def video_length(self) -> int:
        return self._video_length

    def path(self, idx: int) -> str:
        return os.path.join(self._data_root, self._traj_names[idx])

    def folder(self, idx: int) -> str:
        return os.path.basename(os.path.dirname(self._traj_names[idx]))

    def robot(self, idx: int) -> str:
        """The file's `robot` attribute (read once per file)."""
        if idx not in self._robots:
            with open_trajectory(self.path(idx)) as hf:
                self._robots[idx] = _text(hf.attrs["robot"])
        return self._robots[idx]

    @property
    def lengths(self) -> np.ndarray:
        """Every file's episode length (read once, headers only)."""
        if self._lengths is None:
            out = np.zeros(len(self), np.int64)
            for i in range(len(self)):
                with open_trajectory(self.path(i)) as hf:
                    out[i] = episode_length(hf, self.path(i))
            self._lengths = out
        return self._lengths

    def __getitem__(self, idx):
        path = self.path(idx)
        with open_trajectory(path) as hf:
            ep_len = episode_length(hf, path)
            assert ep_len >= self._video_length, f"{ep_len}, {path}"
            return self._item(hf, idx, draw_start(self._rng, ep_len, self._video_length), ep_len)

    def item(self, idx: int, start: int, masks: bool = True):
        """The item of a given window start (what `__getitem__` returns when its draw is `start`)."""
        path = self.path(idx)
        with open_trajectory(path) as hf:
            return self._item(hf, idx, start, episode_length(hf, path), masks)

    def masks(self, idx: int, start: int, length: int) -> torch.Tensor:
        """The transformed masks (length, 1, w, w) of the file's steps [start, start + length)."""
        with open_trajectory(self.path(idx)) as hf:
            return mask_transform(hf["mask"][start:start + length].astype(np.float32), self._config.image_width)

    def _item(self, hf, idx, start, ep_len, want_masks=True):
        path = self.path(idx)
        end = start + self._video_length if ep_len > self._video_length else ep_len
        states = hf["states"][start:end].astype(np.float32)
        low, high = hf["low_bound"][:], hf["high_bound"][:]
        actions = self._load_actions(hf, low, high, start, end - 1)
        qpos = hf["qpos"][start:end].astype(np.float32)
        out = {}
        if want_masks:
            masks = hf["mask"][start:end].astype(np.float32)
            assert len(states) == len(actions) + 1 == len(masks) == len(qpos), \
                f"{path}, {states.shape}, {actions.shape}, {masks.shape}"
            out["masks"] = mask_transform(masks, self._config.image_width)
        actions = self._preprocess_actions(states, actions, low, high)
        states = self._preprocess_states(states, low, high)
        out.update(states=states, actions=actions, robot=_text(hf.attrs["robot"]), folder=self.folder(idx),
                   file_path=path, idx=idx, qpos=qpos)
        return out

    def _load_actions(self, hf, low, high, start, end):
        """joint_pos_dataset.py:107-129."""
        actions = hf["actions"][:].astype(np.float32)
        a_T, adim = actions.shape
        if self._action_dim == adim:
            return actions[start:end]
        if self._impute_autograsp_action and adim + 1 == self._action_dim:
            append = np.zeros((a_T, 1))
            next_state = hf["states"][:][1:, -1]
            high_val, low_val = high[-1], low[-1]
            midpoint = (high_val + low_val) / 2.0
            for t, s in enumerate(next_state):
                append[t, 0] = high_val if s > midpoint else low_val
            return np.concatenate((actions, append), axis=-1)[start:end].astype(np.float32)
        raise ValueError(f"file adim {adim}, target adim {self._action_dim}")

    @staticmethod
    def _preprocess_states(states, low, high):
        """joint_pos_dataset.py:131-141: only the gripper force is normalised here."""
        states = torch.from_numpy(states)
        force_min, force_max = low[GRIP], high[GRIP]
        states[:, GRIP] = (states[:, GRIP] - force_min) / (force_max - force_min)
        return states

    def _preprocess_actions(self, states, actions, low, high):
        """joint_pos_dataset.py:183-203."""
        strategy = self._config.preprocess_action
        if strategy == "raw":
            return torch.from_numpy(actions)
        if strategy == "state_infer":
            states = states.copy()
            xyz = states[:, :3] * (high[:3] - low[:3])
            states[:, :3] = xyz + low[:3]
            for t in range(len(actions)):
                actions[t][:3] = states[t + 1][:3] - states[t][:3]
            return torch.from_numpy(actions)
        raise ValueError(f"preprocess_action {strategy!r}: the joint-position dataset knows {STRATEGIES}")


# --------------------------------------------------------------------------- #
# the loaders (widowx_joint_pos_dataloaders.py, baxter_joint_pos_dataloaders.py)
# --------------------------------------------------------------------------- #
def _trajectories(folder):
    return [d.path for d in os.scandir(folder) if d.is_file() and d.path.lower().endswith(TRAJ_EXTENSIONS)]


def _finetune_loaders(config, files, labels):
    n_test, n_train = config.finetune_num_test, config.finetune_num_train
    train = JointPosDataset(files[n_test:n_test + n_train], labels[n_test:n_test + n_train], config,
                            augment_img=getattr(config, "img_augmentation", False))
    test = JointPosDataset(files[:n_test], labels[:n_test], config)

    def loader(ds, batch_size):
        return tdata.DataLoader(ds, num_workers=config.data_threads, batch_size=batch_size, shuffle=True, drop_last=False,
                                pin_memory=True,
                                generator=torch.Generator().manual_seed(config.seed))
    return loader(train, config.batch_size), loader(test, config.test_batch_size)


def create_loaders(config):
    """widowx_joint_pos_dataloaders.py:13-82: every viewpoint folder of <data_root>/widowx_views, sorted by path, shuffled
    with the config seed; the first finetune_num_test files test, the next finetune_num_train train."""
    pairs = []
    for folder in os.scandir(os.path.join(config.data_root, "widowx_views")):
        if folder.is_dir():
            pairs += [(p, folder.name) for p in _trajectories(folder.path)]
    pairs = sorted(pairs, key=lambda x: x[0])
    random.seed(config.seed)
    random.shuffle(pairs)
    return _finetune_loaders(config, [p[0] for p in pairs], [p[1] for p in pairs])


def create_finetune_loaders(config):
    """baxter_joint_pos_dataloaders.py:16-69: <data_root>/baxter_views/left_c0.  With `--world_error_dict` (a pickle of
    {path: [{"high_error": bool}, ...]}) only the trajectories it marks as high-error are kept, as in the reference."""
    files = _trajectories(os.path.join(config.data_root, "baxter_views", "left_c0"))
    if getattr(config, "world_error_dict", None):
        with open(config.world_error_dict, "rb") as f:
            motion_info = pickle.load(f)
        files = [p for p in files if any(x["high_error"] for x in motion_info[p])]
    files = sorted(files)
    random.seed(config.seed)
    random.shuffle(files)
    return _finetune_loaders(config, files, ["baxter"] * len(files))


# --------------------------------------------------------------------------- #
# the device-resident split
# --------------------------------------------------------------------------- #
class DeviceJointPosData:
    """A JointPosDataset's trajectories on the device, in stored form: states fp64 (N, Tmax, R), actions fp32
    (N, Tmax - 1, A), qpos fp32 (N, Tmax, J), bounds fp64 (N, 2, R), meta int32 (N, 3) = (length, action width, bounds
    stored as float64); no masks.  `batch` gathers and preprocesses one batch in one `rac_joint_batch` launch."""

    def __init__(self, dataset: JointPosDataset, device):
        cf = dataset._config
        if cf.preprocess_action not in STRATEGIES:
            raise ValueError(f"preprocess_action {cf.preprocess_action!r}: the joint-position dataset knows {STRATEGIES}")
        self.dataset, self.device = dataset, torch.device(device)
        self.window, self.A = dataset.video_length, int(cf.action_dim)
        self.state_infer = cf.preprocess_action == "state_infer"
        rows = []
        for i in range(len(dataset)):
            path = dataset.path(i)
            with open_trajectory(path) as hf:
                n = episode_length(hf, path)
                states, actions, qpos = hf["states"][:], hf["actions"][:], hf["qpos"][:]
                low, high = hf["low_bound"][:], hf["high_bound"][:]
                dataset._robots[i] = _text(hf.attrs["robot"])  # (the batches list it: no file is opened per batch)
            adim = actions.shape[1]
            if adim != self.A and not (cf.impute_autograsp_action and adim + 1 == self.A):
                raise ValueError(f"file adim {adim}, target adim {self.A}")
            for b in (low, high):
                if b.dtype not in (np.float32, np.float64) or b.shape != (states.shape[1],):
                    raise ValueError(f"{path}: bounds must be float32 / float64 of the states' width, got {b.dtype} {b.shape}")
            if states.dtype not in (np.float32, np.float64):
                raise ValueError(f"{path}: states must be stored as float32 / float64, got {states.dtype}")
            if n < self.window or not (len(states) == len(qpos) == len(actions) + 1 == n):
                raise ValueError(f"{path}: {n} frames, {len(states)} states, {len(qpos)} qpos, {len(actions)} actions for "
                                 f"a window of {self.window}")
            rows.append((states, actions.astype(np.float32), qpos.astype(np.float32), low, high))
        if not rows:
            raise ValueError("DeviceJointPosData: an empty dataset")
        N, self.Tmax = len(rows), max(len(r[0]) for r in rows)
        self.R, self.J = rows[0][0].shape[1], rows[0][2].shape[1]
        if self.R <= GRIP or any(r[0].shape[1] != self.R or r[2].shape[1] != self.J for r in rows):
            raise ValueError(f"DeviceJointPosData: states of width {self.R} (>= 5) and qpos of width {self.J} in every file")
        if self.state_infer and self.A < 3:
            raise ValueError("state_infer needs action_dim >= 3")
        states = np.zeros((N, self.Tmax, self.R), np.float64)
        actions = np.zeros((N, self.Tmax - 1, self.A), np.float32)
        qpos = np.zeros((N, self.Tmax, self.J), np.float32)
        bounds = np.zeros((N, 2, self.R), np.float64)
        meta = np.zeros((N, 3), np.int32)
        for i, (s, a, q, low, high) in enumerate(rows):
            states[i, :len(s)], actions[i, :len(a), :a.shape[1]], qpos[i, :len(q)] = s, a, q
            bounds[i, 0], bounds[i, 1] = low, high
            meta[i] = len(s), a.shape[1], int(low.dtype == np.float64 or high.dtype == np.float64)
        self.lengths = meta[:, 0].astype(np.int64)
        up = lambda a: torch.from_numpy(a).to(self.device)
        self.states, self.actions, self.qpos, self.bounds, self.meta = (up(a) for a in (states, actions, qpos, bounds, meta))

    def __len__(self):
        return len(self.lengths)

    def check(self, index, start):
        """The (index, start) pairs of a batch as int32 arrays, refused unless every window lies inside its episode: the
        kernel reads them from device memory, where the entry point cannot look."""
        index, start = np.asarray(index), np.asarray(start)
        if (index.ndim != 1 or index.shape != start.shape or not len(index)
                or not (np.issubdtype(index.dtype, np.integer) and np.issubdtype(start.dtype, np.integer))):
            raise ValueError(f"joint batch: one integer index and start per sample, got {index.shape} and {start.shape}")
        if index.min() < 0 or index.max() >= len(self):
            raise ValueError(f"joint batch: trajectory index outside [0, {len(self)}): {index.tolist()}")
        if start.min() < 0 or np.any(start + self.window > self.lengths[index]):
            raise ValueError(f"joint batch: a window of {self.window} from {start.tolist()} leaves its episode "
                             f"(lengths {self.lengths[index].tolist()})")
        return index.astype(np.int32), start.astype(np.int32)

    def batch(self, index, start):
        """Time-first (qpos (L, B, J), states (L, B, R), actions (L - 1, B, A)) of the windows [start, start + L) of the
        trajectories `index`: two small uploads and one launch on the current stream."""
        index, start = self.check(index, start)
        table = torch.from_numpy(np.stack([index, start])).to(self.device, non_blocking=True)
        return ops.joint_batch(self.states, self.actions, self.qpos, self.bounds, self.meta, table[0], table[1],
                               self.window, self.state_infer)


# --------------------------------------------------------------------------- #
# batches: the host loader's index order, the device's gather
# --------------------------------------------------------------------------- #
class _Indices(tdata.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return int(i)


def host_gather(dataset):
    """`gather` of `device_batches` by the host dataset (time-first CPU tensors): what the launch must reproduce."""
    def gather(index, start):
        items = [dataset.item(i, s, masks=False) for i, s in zip(index, start)]
        return tuple(torch.stack([torch.as_tensor(it[k]) for it in items], 1) for k in ("qpos", "states", "actions"))
    return gather


class DeviceBatches:
    """The batches of one host loader from the device-resident split: time-first dicts {qpos, states, actions, robot,
    folder, file_path, idx, start, time_first=True}.  No masks: `plot` reads those of its few videos from the host
    dataset by `idx` and `start`.

    The index batches are the host loader's: an index-only dataset in a real DataLoader over the loader's own batch
    sampler and generator, so the generator's state moves exactly as under `iter(loader)`.  Iterating the object is ONE
    epoch, a fresh iterator of that DataLoader every time (the form for a test loader: always a full pass, whatever else
    has drawn in between); `forever()` is the reference's `get_batch` (joint_pos_dataset.py:217-230), a loop over such
    epochs with an iterator of its own.  All of them share the loader's generator and one RandomState(seed) for the
    window starts, drawn in the order the items are produced by the dataset's rule -- as the iterators of one host loader
    with `--data_threads 0` share its generator and its dataset's RandomState.  `gather(index, start)` replaces the
    launch (tests)."""

    def __init__(self, loader, device, gather=None):
        ds = self.dataset = loader.dataset
        self.loader = loader
        self.resident = DeviceJointPosData(ds, device) if gather is None else None
        self._gather = gather if gather is not None else self.resident.batch
        self._rng = np.random.RandomState(ds._config.seed)
        self._lengths, self._window = ds.lengths, ds.video_length
        if not len(ds) or self._lengths.min() < self._window:
            raise ValueError(f"{len(ds)} episodes, the shortest of {self._lengths.min() if len(ds) else 0} steps, for a "
                             f"window of {self._window}")
        self._order = tdata.DataLoader(_Indices(len(ds)), batch_sampler=loader.batch_sampler, generator=loader.generator,
                                       num_workers=0, collate_fn=list)

    def _batch(self, idx):
        ds = self.dataset
        start = [draw_start(self._rng, int(self._lengths[i]), self._window) for i in idx]
        qpos, states, actions = self._gather(idx, start)
        return {"qpos": qpos, "states": states, "actions": actions, "robot": [ds.robot(i) for i in idx],
                "folder": [ds.folder(i) for i in idx], "file_path": [ds.path(i) for i in idx],
                "idx": torch.as_tensor(idx), "start": start, "time_first": True}

    def __len__(self):
        return len(self._order)

    def __iter__(self):
        for idx in self._order:
            yield self._batch(idx)

    def forever(self):
        while True:
            yield from self


def device_batches(loader, device, epochs=None, gather=None):
    """The reference's `get_batch` from the device-resident split: `DeviceBatches(loader, device)`'s batches without end,
    or `epochs` passes over the loader."""
    feed = DeviceBatches(loader, device, gather)
    if epochs is None:
        yield from feed.forever()
    for _ in range(epochs or 0):
        yield from feed


def mask_iou(counts) -> float:
    """joint_pos_trainer.py:547-567 from the per-frame counts (V, T, 2) of |pred & true| and |pred | true|: the IoU per
    frame (an empty union gives NaN, as there), its float32 mean over a video's frames, the mean over the videos."""
    counts = torch.as_tensor(counts).to(torch.int64)
    per_frame = counts[..., 0] / counts[..., 1]
    return float(np.mean([v.mean().item() for v in per_frame]))


def get_batch(loader, device):
    """The host form of the same generator (joint_pos_dataset.py:217-230)."""
    from .robot_trainer import process_batch
    while True:
        for data in loader:
            yield process_batch(data, device)
