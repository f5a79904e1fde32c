"""The object-movement pass (reference src/prediction/measure_obj_movement.py): score every video of a viewpoint folder
with the copy baseline's summed world error, threshold the score, and write the `obj_movement.pkl` that
`--load_movement_info True` (`RoboNetDataset._movement_tables`) and `data.create_movement_loader` read.

The reference scores one video per batch (`batch_size = 1`, measure_obj_movement.py:168), because its
`world_mse_criterion` returns a batch mean.  Here `ops.video_movement` returns one score PER VIDEO from one launch per
batch, so any `--batch_size` gives what the reference gives at batch size 1; at a larger batch the reference would
average the videos of a batch, which it never does and this pass does not either."""
from __future__ import annotations

import copy
import json
import os
import pickle
from collections import defaultdict

import torch
import torch.utils.data as data

from . import ops
from .data import MOVEMENT_FILE, TRAJ_EXTENSIONS, RoboNetDataset, collate, process_batch

# measure_obj_movement.py:146-159: "<robot>_<viewpoint folder>" -> the summed world error from which a video counts as
# showing object movement
MOVEMENT_THRESHOLDS = {
    "sawyer_sudri0_c0": 0.114,
    "sawyer_sudri0_c1": 0.21,
    "sawyer_sudri0_c2": 0.18,
    "sawyer_vestri_table2_c0": 0.09,
    "sawyer_vestri_table2_c1": 0.26,
    "sawyer_vestri_table2_c2": 0.149,
    "sawyer_sudri2_c0": 0.095,
    "sawyer_sudri2_c1": 0.223,
    "sawyer_sudri2_c2": 0.165,
    "baxter_left_c0": 0.017,
    "widowx_widowx1_c0": 0.11,
    "locobot_c0": 0.15,
}
# measure_obj_movement.py:178-183: the folders the reference's command line walks
ROBOT_VIEWPOINTS = {
    "baxter": ["left_c0"],
    "widowx": ["widowx1_c0"],
    "sawyer": ["sudri0_c0", "sudri0_c1", "sudri0_c2", "sudri2_c0", "sudri2_c1", "sudri2_c2", "vestri_table2_c0",
               "vestri_table2_c1", "vestri_table2_c2"],
    "locobot": ["c0"],
}
SCORES_FILE = "obj_movement_scores.json"


def score_videos(loader, device) -> dict:
    """{file_path: score} of every video a loader yields, walked once: `process_batch` (so `--device_images True`
    batches work too), one `ops.video_movement` call over the batch's whole window and one device-to-host copy per
    batch."""
    scores = {}
    for batch in loader:
        paths = list(batch["file_path"])
        batch = process_batch(batch, device)
        score, _ = ops.video_movement(batch["images"], batch["masks"])
        for path, s in zip(paths, score.tolist()):
            scores[path] = s
    return scores


def folder_loader(folder, label, config):
    """An unshuffled loader over every trajectory of one viewpoint folder (sorted by path), without augmentation and
    with `load_movement_info` off: the table is what this pass makes."""
    files = sorted(d.path for d in os.scandir(folder) if d.is_file() and d.path.lower().endswith(TRAJ_EXTENSIONS))
    cf = copy.copy(config)
    cf.load_movement_info = False
    dataset = RoboNetDataset(files, [label] * len(files), cf, device_images=getattr(cf, "device_images", False))
    return data.DataLoader(dataset, num_workers=cf.data_threads, batch_size=cf.batch_size, pin_memory=True,
                           collate_fn=collate)


def _replace(path, mode, write):
    """Write to a temporary name and rename: a reader never sees half a file."""
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, mode) as f:
        write(f)
    os.replace(tmp, path)


def measure_obj_movement(robot, viewpoint, config, threshold=None, overwrite=False):
    """Score and flag every trajectory of <data_root>/<robot>_views/<viewpoint>/ (measure_obj_movement.py:109-162).

    The videos are the windows `RoboNetDataset(files, labels, config)` yields without augmentation: `video_length`
    frames, a seeded random start (`_window`) in longer files; the reference's loop runs over `n_past + n_future` frames,
    which its command line sets to the same 31.  `flag = score >= threshold`; `threshold` defaults to
    `MOVEMENT_THRESHOLDS`.  Written next to the trajectories:
      obj_movement.pkl          a pickled `defaultdict(bool)`: item["file_path"] -> bool, the reference's file
      obj_movement_scores.json  the raw scores, the threshold, T, H, W, the seed and the count above the threshold, so
                                that another threshold can be picked without scoring again
    An existing obj_movement.pkl is kept unless `overwrite`.  The per-video score is the reference's at its batch size
    1 whatever `config.batch_size` is (module docstring).  Returns (scores, flags)."""
    key = f"{robot}_{viewpoint}"
    if threshold is None:
        if key not in MOVEMENT_THRESHOLDS:
            raise KeyError(f"no movement threshold is known for {key!r}: pass threshold=")
        threshold = MOVEMENT_THRESHOLDS[key]
    folder = os.path.join(config.data_root, f"{robot}_views", viewpoint)
    table_path = os.path.join(folder, MOVEMENT_FILE)
    if os.path.exists(table_path) and not overwrite:
        raise FileExistsError(f"{table_path} exists and is kept: pass overwrite=True (--overwrite True) to replace it")
    cf = config
    if not torch.cuda.is_available():
        raise ops._lib.RacError("measure_obj_movement needs an MI355X (no CPU fallback)")
    device = getattr(cf, "device", None) or torch.device("cuda", torch.cuda.current_device())
    scores = score_videos(folder_loader(folder, key, cf), device)
    flags = defaultdict(bool)
    for path, s in scores.items():
        flags[path] = bool(s >= threshold)
    above = sum(flags.values())
    print(f"above threshold videos: {above}")
    info = {"robot": robot, "viewpoint": viewpoint, "threshold": float(threshold), "T": cf.video_length,
            "H": cf.image_height, "W": cf.image_width, "seed": cf.seed,
            "videos": len(scores), "above_threshold": above, "scores": scores}
    _replace(os.path.join(folder, SCORES_FILE), "w", lambda f: json.dump(info, f, indent=1))
    _replace(table_path, "wb", lambda f: pickle.dump(flags, f))
    return scores, flags
