"""Shared by the joint-position data tests (tests/test_joint_pos_data_host.py, tests/test_gpu_joint_pos.py) and by
tools/gen_golden_joint_pos.py: seeded trajectory files in RoboNet's layout, the config they are read with, and
restatements of the reference's image transform and IoU.  Plain numpy / torch; no reference code."""
import argparse
import os

import numpy as np
import torch

WINDOW, A, R = 6, 5, 5
SEED = 3
# (length, action width in the file, bounds stored as float64, states stored as float64): both bound dtypes, imputed and
# full action width, episodes longer than the window and equal to it
SPECS = ((9, 4, False, False), (9, 4, True, True), (6, 5, False, False), (6, 5, True, False), (6, 4, True, False),
         (8, 5, False, True), (9, 4, True, False), (7, 5, True, True))


def write_trajectory(path, key, length, adim, bounds64, states64, J=7, hw=(4, 6), robot="widowx"):
    g = np.random.Generator(np.random.Philox(key=[SEED, key]))
    low = np.array([0.2, -0.3, 0.05, -1.5, -1.0]) + g.normal(0, 0.01, R)
    high = low + np.array([0.5, 0.6, 0.3, 3.0, 2.0]) + g.normal(0, 0.01, R)
    bdt, sdt = (np.float64 if bounds64 else np.float32), (np.float64 if states64 else np.float32)
    states = g.random((length, R))
    states[:, 4] = low[4] + (high[4] - low[4]) * g.random(length)  # the raw gripper force, on both sides of the midpoint
    mask = (g.random((length,) + hw) > 0.6).astype(np.uint8)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, frames=g.integers(0, 256, (length,) + hw + (3,), dtype=np.uint8), mask=mask, states=states.astype(sdt),
             actions=g.normal(0, 0.03, (length - 1, adim)).astype(np.float32), qpos=g.normal(0, 1, (length, J)).astype(sdt),
             low_bound=low.astype(bdt), high_bound=high.astype(bdt), attr_robot=np.array(robot))


def write_root(root, specs=SPECS, view="widowx_views", folders=("cam0", "cam1"), J=7, hw=(4, 6)):
    """One file per spec under <root>/<view>/<folder>/, folders taken in turn; returns the paths in spec order."""
    paths = []
    for i, (length, adim, b64, s64) in enumerate(specs):
        p = os.path.join(root, view, folders[i % len(folders)], f"traj_{i:03d}.npz")
        write_trajectory(p, i, length, adim, b64, s64, J=J, hw=hw, robot=view.split("_")[0])
        paths.append(p)
    return paths


def config(root, **kw):
    d = dict(data_root=str(root), video_length=WINDOW, n_past=2, n_future=2, n_eval=WINDOW, action_dim=A,
             impute_autograsp_action=True, image_width=8, seed=SEED, preprocess_action="raw", data_threads=0, batch_size=3,
             test_batch_size=2, finetune_num_test=2, finetune_num_train=5, img_augmentation=False, world_error_dict=None,
             experiment="finetune_widowx")
    d.update(kw)
    return argparse.Namespace(**d)


def to_tensor_center_crop(mask, size):
    """tf.Compose([tf.ToTensor(), tf.CenterCrop(size)]) of one (H, W) array, restated: ToTensor gives (1, H, W) float
    (uint8 / 255); CenterCrop zero-pads a short side by (d // 2, (d + 1) // 2) and cuts from the rounded half offset."""
    m = np.asarray(mask)
    t = torch.from_numpy(m.astype(np.float32) / 255 if m.dtype == np.uint8 else m.astype(np.float32))
    h, w = t.shape
    out = torch.zeros(max(h, size), max(w, size))
    top, left = (max(size - h, 0)) // 2, (max(size - w, 0)) // 2
    out[top:top + h, left:left + w] = t
    h, w = out.shape
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    return out[top:top + size, left:left + size].unsqueeze(0)


def compute_iou(prediction, target):
    """joint_pos_trainer.py:561-567 on (T, 1, H, W) masks: the IoU per frame."""
    prediction, target = prediction.type(torch.bool), target.type(torch.bool)
    return (prediction & target).sum((1, 2, 3)) / (prediction | target).sum((1, 2, 3))


def comparison_frames(pred, true):
    """(T, V H, 3 W) uint8 rows [true | predicted | xor] of (V, T, H, W) float masks."""
    u8 = lambda t: (t.clamp(0, 1) * 255).to(torch.uint8)
    xor = ((pred != 0) ^ (true != 0)).to(torch.uint8) * 255
    V, T, H, W = pred.shape
    return torch.cat([u8(true), u8(pred), xor], 3).permute(1, 0, 2, 3).reshape(T, V * H, 3 * W)


def mean_iou(pred, true):
    """The plot's number: per video the float32 mean of the frame IoUs, then numpy's mean over the videos."""
    return float(np.mean([compute_iou(p.unsqueeze(1), t.unsqueeze(1)).mean().item() for p, t in zip(pred, true)]))


def joint_batch_restatement(res, index, start):
    """The arithmetic include/rac_hip.h states for rac_joint_batch, element by element in numpy scalars, on the staged
    arrays of a `DeviceJointPosData` (built on the CPU): what the kernel must compute, checkable without a GPU."""
    f32, f64 = np.float32, np.float64
    S, Ac, Q, Bd, M = (t.cpu().numpy() for t in (res.states, res.actions, res.qpos, res.bounds, res.meta))
    L, B = res.window, len(index)
    q = np.zeros((L, B, res.J), f32)
    s = np.zeros((L, B, res.R), f32)
    a = np.zeros((L - 1, B, res.A), f32)

    def denorm(x, lo, hi, wide):
        if wide:
            return f32(f64(x) * (hi - lo) + lo)
        return f32(f32(x * (f32(hi) - f32(lo))) + f32(lo))
    for b, (n, t0) in enumerate(zip(index, start)):
        low, high = Bd[n, 0], Bd[n, 1]
        adim, wide = int(M[n, 1]), bool(M[n, 2])
        for l in range(L):
            t = t0 + l
            q[l, b] = Q[n, t]
            s[l, b] = S[n, t].astype(f32)
            span = f32(high[4] - low[4]) if wide else f32(high[4]) - f32(low[4])
            s[l, b, 4] = f32(f32(s[l, b, 4] - f32(low[4])) / span)
            if l == L - 1:
                continue
            for c in range(res.A):
                if res.state_infer and c < 3:
                    a[l, b, c] = denorm(f32(S[n, t + 1, c]), low[c], high[c], wide) - denorm(f32(S[n, t, c]), low[c], high[c], wide)
                elif c < adim:
                    a[l, b, c] = Ac[n, t, c]
                else:
                    lo, hi = low[-1], high[-1]
                    mid = (hi + lo) / 2.0 if wide else f64(f32(f32(hi) + f32(lo)) / f32(2))
                    a[l, b, c] = f32(hi if S[n, t + 1, -1] > mid else lo)
    return torch.from_numpy(q), torch.from_numpy(s), torch.from_numpy(a)
