"""TEST INFRASTRUCTURE ONLY -- golden vectors of the end-effector heatmaps (`create_heatmaps`, robonet_dataset.py:482-544).

Runs only where the reference checkout is present: it loads oracle/gen_golden.py for its recipe (absent third-party
modules stubbed, the reference first on sys.path so that the name `src` is the reference's), imports the REFERENCE's own
`create_heatmaps` and runs it on the CPU, one configuration per robot (sawyer sudri0_c0, baxter left_c0, widowx
widowx1_c0, locobot c0).  It records numbers only, to tests/golden/heatmaps.npz: per robot the K, wTc, low, high used,
64 seeded states with the reference's integers (mx, my as it cast them to uint8, and whether the frame was drawn) and
the full reference heatmap of 4 of them.

The reference's `get_2d_eef_pos` is wrapped to record what `create_heatmaps` hands it and what it returns, and is run a
second time on an array whose `astype` is the identity, which gives the coordinates just before the cast.  Only states
for which that cast is defined and robust are kept (both coordinates inside (-100, 200), fractional parts in
[0.001, 0.999]; asserted), and the draws are searched so that the set holds centres at all four image corners, a
coordinate in (-1, 0) (truncates to 0: valid), and mx == W and my == H (invalid).  The bounds of each configuration are
the box around a part of the camera's viewing volume, so that every robot has frames inside and outside the image.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_heatmaps.py
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


gg = _load("gen_golden", os.path.join(REPO, "oracle", "gen_golden.py"))  # stubs + sys.path: the reference imports now
refs = _load("heatmap_refs", os.path.join(REPO, "tests", "heatmap_refs.py"))

for name in ("tqdm",):
    try:
        __import__(name)
    except ImportError:
        gg.MISSING.add(name)

import src.dataset.robonet.robonet_dataset as ref_mod  # noqa: E402

W, H, N_STATES, N_FULL = 64, 48, 64, 4
_calls = []
_orig = ref_mod.get_2d_eef_pos


class _NoCast(np.ndarray):
    """An array whose astype returns the values as they are: the reference's own arithmetic, minus its final cast."""

    def astype(self, *a, **k):
        return np.asarray(self)


def _recording(state, cam_intrinsics, world_to_cam, target_dim, orig_dim):
    before = _orig(state.copy().view(_NoCast), cam_intrinsics, world_to_cam, target_dim, orig_dim)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # numpy's "invalid value encountered in cast" for coordinates below 0
        cast = _orig(state, cam_intrinsics, world_to_cam, target_dim, orig_dim)
    _calls.append(dict(K=np.array(cam_intrinsics), wTc=np.array(world_to_cam), before=np.array(before), cast=np.array(cast)))
    return cast


ref_mod.get_2d_eef_pos = _recording


def run_reference(states, low, high, robot, vp):
    _calls.clear()
    hm = ref_mod.create_heatmaps(torch.from_numpy(states.copy()), low, high, robot, vp)
    (call,) = _calls
    return hm, call


def view_box(wTc, z_off):
    """low / high (5,) float32: the box around the camera rays X/Z in [-0.85, 0.85], Y/Z in [-0.7, 0.7] (wider than
    either camera's image) at depths 0.45 .. 0.9 m."""
    c2w = np.linalg.inv(wTc)
    pts = np.array([(c2w @ np.array([a * d, b * d, d, 1.0]))[:3]
                    for d in (0.45, 0.9) for a in (-0.85, 0.85) for b in (-0.7, 0.7)])
    low = np.append(pts.min(0) - [0, 0, z_off], [0.0, 0.0]).astype(np.float32)
    high = np.append(pts.max(0) - [0, 0, z_off], [1.0, 1.0]).astype(np.float32)
    return low, high


def robust(x, y):
    fx, fy = np.abs(x - np.trunc(x)), np.abs(y - np.trunc(y))
    return ((x > -100) & (x < 200) & (y > -100) & (y < 200) & (fx >= 0.001) & (fx <= 0.999) & (fy >= 0.001) & (fy <= 0.999))


def main():
    rng = np.random.RandomState(20260)
    out, seen = {}, set()
    for robot, (z_off, cam, (ow, oh), vp) in refs.ROBOTS.items():
        probe = np.zeros((1, 5), dtype=np.float32)
        _, call = run_reference(probe, np.zeros(5, np.float32), np.ones(5, np.float32), robot, vp)
        K, wTc = call["K"], call["wTc"]
        low, high = view_box(wTc, z_off)
        draws = rng.uniform(0, 1, size=(400000, 5)).astype(np.float32)
        x, y, mx, my, valid = refs.centres(draws, low, high, robot, K, wTc, H, W)
        ok = robust(x, y)
        wanted = {  # special centres, searched for in every robot's draws
            "corner00": valid & (mx == 0) & (my == 0) & (x > 0) & (y > 0), "corner0H": valid & (mx == 0) & (my == H - 1),
            "cornerW0": valid & (mx == W - 1) & (my == 0), "cornerWH": valid & (mx == W - 1) & (my == H - 1),
            "x_neg_frac": valid & (x > -1) & (x < 0), "y_neg_frac": valid & (y > -1) & (y < 0),
            "mx_eq_W": (mx == W) & (y > 0) & (y < H), "my_eq_H": (my == H) & (x > 0) & (x < W),
        }
        pick = []
        for name, cond in wanted.items():
            hit = np.nonzero(cond & ok)[0]
            if len(hit):
                pick.append(hit[0])
                seen.add(name)
        n_valid = (N_STATES - len(pick)) * 2 // 3
        rest_valid = [i for i in np.nonzero(valid & ok)[0] if i not in pick][:n_valid]
        rest_invalid = [i for i in np.nonzero(~valid & ok)[0] if i not in pick][:N_STATES - len(pick) - len(rest_valid)]
        states = draws[np.array(pick + rest_valid + rest_invalid)]
        assert len(states) == N_STATES, len(states)
        hm, call = run_reference(states, low, high, robot, vp)
        bx, by = call["before"]
        assert robust(bx, by).all(), (robot, bx, by)
        drawn = hm.reshape(N_STATES, -1).max(1) > 0
        cx, cy = call["cast"].astype(np.int64)
        assert (drawn == ((np.trunc(bx) >= 0) & (np.trunc(bx) < W) & (np.trunc(by) >= 0) & (np.trunc(by) < H))).all(), robot
        assert 8 <= drawn.sum() <= N_STATES - 8, (robot, drawn.sum())
        full = np.nonzero(drawn)[0][:N_FULL]
        out.update({f"{robot}_K": K, f"{robot}_wTc": wTc, f"{robot}_low": low, f"{robot}_high": high,
                    f"{robot}_states": states, f"{robot}_centres": np.stack([cx, cy, drawn.astype(np.int64)], 1),
                    f"{robot}_precast": np.stack([bx, by], 1), f"{robot}_full_idx": full, f"{robot}_heatmaps": hm[full]})
        print(robot, "drawn", int(drawn.sum()), "of", N_STATES, "x", bx.min().round(1), bx.max().round(1), "y",
              by.min().round(1), by.max().round(1))
    assert seen == {"corner00", "corner0H", "cornerW0", "cornerWH", "x_neg_frac", "y_neg_frac", "mx_eq_W", "my_eq_H"}, seen
    gg.save("heatmaps", **out)


if __name__ == "__main__":
    main()
