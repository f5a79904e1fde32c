"""Helpers of the object-movement tests (test_gpu_movement.py, test_movement_host.py); no tests here.

`movement_ref`: the formula of `rac_video_movement` (include/rac_hip.h) restated in torch on the CPU, in the dtype
asked for -- fp64 is the reference, fp32 gives the e_cpu32 of the rule in tests/fp64_tools.py from the same code:

    step_err[t-1][v] = sum_{c, p : mask(t,v)[p] == 0} (img(t,v)[c][p] - img(t-1,v)[c][p])^2 / (3 #{p : mask(t,v)[p] == 0} + 1)
    score[v]         = step_err[0][v] + step_err[1][v] + ...   (a running sum in that order)

`expected_order`: the movement loader's sort / seed / shuffle rule restated on a list of paths.

`write_movement_fixture`: npz trajectories in RoboNet layout (the keys tools/make_synthetic_robonet.py writes) whose
copy-baseline error is small in one half of the files and large in the other."""
import os
import random

import numpy as np
import torch


def movement_ref(images, masks, dt):
    """images (T, B, 3, H, W), masks (T, B, 1, H, W), CPU -> (score (B,), step_err (T - 1, B)) in dtype `dt`."""
    x = images.to(dt)
    world = masks[1:] == 0                                   # a robot pixel is mask != 0
    d = x[1:] - x[:-1]
    sq = torch.where(world.expand_as(d), d * d, torch.zeros((), dtype=dt)).sum((2, 3, 4))
    count = 3 * world.sum((2, 3, 4)) + 1                     # an integer
    step = sq / count.to(dt)
    score = step[0].clone()
    for k in range(1, step.shape[0]):
        score = score + step[k]
    return score, step


def expected_order(flagged, seed):
    """The reference's selection rule restated (robonet_dataloaders.py:210-311) on a list of flagged paths: per robot
    sorted by path and shuffled after `random.seed(seed)`; baxter + widowx + sawyer; reseeded and shuffled again."""
    out = []
    for robot in ("baxter", "widowx", "sawyer"):
        fl = sorted(p for p in flagged if os.sep + robot + "_views" + os.sep in p)
        random.seed(seed)
        random.shuffle(fl)
        out += fl
    random.seed(seed)
    random.shuffle(out)
    return out


def write_movement_fixture(root, views=(("baxter", "left_c0"), ("widowx", "widowx1_c0")), moving=3, static=3, T=8, h=16,
                           w=21, seed=0):
    """<root>/<robot>_views/<view>/traj_XXX.npz, the `moving` files of a view first, then its `static` ones.  Every video: one
    static uint8 background repeated over T with +-2 grey levels of per-frame noise, and a robot blob that moves in
    `mask` only.  A "moving" video also shows a 10 x 10 constant-colour square shifted 3 px per frame.
    Returns {file path: True for a moving video}."""
    truth = {}
    n = 0
    for robot, view in views:
        d = os.path.join(root, f"{robot}_views", view)
        os.makedirs(d, exist_ok=True)
        for i in range(moving + static):
            is_moving = i < moving
            g = np.random.Generator(np.random.Philox(key=[seed, n]))
            n += 1
            background = g.integers(90, 166, (h, w, 3))
            frames = background[None] + g.integers(-2, 3, (T, h, w, 3))
            mask = np.zeros((T, h, w), np.uint8)
            for t in range(T):
                mask[t, h - 4:h, min(2 * t, w - 4):min(2 * t, w - 4) + 4] = 1
                if is_moving:
                    frames[t, 2:12, 3 * t:3 * t + 10] = (250, 20, 20)
            low = np.array([0.2, -0.3, 0.05, -1.5, -1.0], np.float32)
            path = os.path.join(d, f"traj_{i:03d}.npz")
            np.savez(path, frames=np.clip(frames, 0, 255).astype(np.uint8), mask=mask,
                     states=g.random((T, 5), dtype=np.float32), actions=g.normal(0, 0.03, (T - 1, 4)).astype(np.float32),
                     qpos=g.normal(0, 1, (T, 7)).astype(np.float32), low_bound=low,
                     high_bound=low + np.array([0.5, 0.6, 0.3, 3.0, 2.0], np.float32), attr_robot=np.array(robot))
            truth[path] = bool(is_moving)
    return truth
