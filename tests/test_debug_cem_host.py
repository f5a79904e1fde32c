"""CPU: the --debug_cem sheet's numpy restatement agrees with itself (vectorised vs loops, tests/debug_cem_refs.py), and the
texts of both planners' sheets land at the reference's anchors (src/cem/cem.py:144-172, push/cem.py:202-233)."""
import argparse

import numpy as np
import pytest
import torch

from robot_aware_control_amd import cem
from tests import debug_cem_refs as refs


@pytest.mark.parametrize("H,W,R,T,G,with_mask", [(2, 4, 1, 1, 1, False), (6, 8, 4, 3, 5, True), (6, 8, 4, 3, 2, True),
                                                 (4, 4, 2, 3, 3, False)])
def test_restatements_agree(H, W, R, T, G, with_mask):
    frames, start, goals, masks = refs.random_problem(3, 5, T, H, W, G, with_mask)
    rows = [4, 0, 0, 2][:R]
    a = refs.sheet_vectorised(frames, rows, start, goals, masks)
    b = refs.sheet_loops(frames, rows, start, goals, masks)
    assert a.shape == b.shape == (T + 1, R * H, 3 * W, 3) and a.dtype == b.dtype == np.uint8
    assert np.array_equal(a, b)


def test_sheet_layout_goal_index_and_masks():
    """G < T: steps past the last goal show the last one; masks black goals from sheet 1 on, never sheet 0."""
    H, W, T, G = 4, 8, 4, 2
    frames, start, goals, masks = refs.random_problem(5, 3, T, H, W, G, True)
    goals = np.maximum(goals, 1)  # no accidental zeros: a 0 in a goal panel is then a masked pixel
    sheet = refs.sheet_vectorised(frames, [2, 1], start, goals, masks)
    assert not sheet[:, :, :W].any()
    for r in range(2):
        blk = sheet[:, r * H:(r + 1) * H]
        assert np.array_equal(blk[0, :, W:2 * W], start) and np.array_equal(blk[0, :, 2 * W:], goals[0])
        for t in range(T):
            g = min(t, G - 1)
            assert np.array_equal(blk[t + 1, :, W:2 * W], refs.u8(frames[[2, 1][r], t]).transpose(1, 2, 0))
            assert np.array_equal(blk[t + 1, :, 2 * W:] == 0, np.repeat((masks[g] != 0)[:, :, None], 3, 2))
            assert np.array_equal(blk[t + 1, :, 2 * W:][masks[g] == 0], goals[g][masks[g] == 0])
    assert masks[0].all() and not sheet[1, :, 2 * W:].any()  # the all-robot goal: black on sheet 1, shown on sheet 0


def test_u8_rule_is_numpys_cast_of_the_product():
    x = refs.planted_values()
    assert np.array_equal(np.uint8(255 * x), refs.u8(x))
    assert refs.u8(np.float32(1)) == 255 and refs.u8(np.nextafter(np.float32(1), np.float32(0))) == 254


def by_sheet(labels):
    out = {}
    for s, x, y, text in labels:
        out.setdefault(s, []).append((x, y, text))
    return out


def test_labels_real_robot_with_and_without_opt():
    H, T = 48, 3
    acts = np.zeros((3, T, 2), np.float32)
    acts[0, 1] = (0.0123, -0.05)
    acts[2, 2] = (-0.0004, 0.0349)
    lab = by_sheet(cem.sheet_labels(3, T, H, True, actions=acts))
    assert sorted(lab) == [0, 1, 2, 3]
    assert lab[0] == [(0, 8, "Start"), (0, H + 8, "Start"), (0, 2 * H + 8, "Start")]
    s2 = lab[2]  # step t = 1
    assert (0, 8, "Opt") in s2 and (0, H + 8, "Rank 0") in s2 and (0, 2 * H + 8, "Rank 1") in s2
    assert (0, 16, "X:1.2cm") in s2 and (0, 24, "Y:-5.0cm") in s2
    assert (0, 2 * H + 16, "X:-0.0cm") in lab[3] and (0, 2 * H + 24, "Y:3.5cm") in lab[3]
    for t in range(T):
        for k in range(3):
            assert (64, k * H + 8, str(t)) in lab[t + 1] and (128, k * H + 8, "GOAL") in lab[t + 1]
        assert len(lab[t + 1]) == 3 * 5
    lab = by_sheet(cem.sheet_labels(2, T, H, False, actions=acts[:2]))
    assert (0, 8, "Rank 0") in lab[1] and (0, H + 8, "Rank 1") in lab[1]
    assert not any(text == "Opt" for rows in lab.values() for _, _, text in rows)


def test_labels_sim_policy():
    lab = by_sheet(cem.sheet_labels(6, 2, 64, True, first_step=1))
    assert (0, 8, "Opt") in lab[1] and (0, 5 * 64 + 8, "Rank 4") in lab[1]
    assert (64, 8, "1") in lab[1] and (64, 8, "2") in lab[2] and (128, 8, "GOAL") in lab[2]
    assert not any(t.startswith(("X:", "Y:")) for rows in lab.values() for _, _, t in rows)
    assert len(lab[1]) == 6 * 3


class _Goal:
    def __init__(self, masks):
        self.masks = masks


def _policies():
    """Both policies without a model or a sampler: only the plot's row choice, labels and folder are exercised."""
    cfg = argparse.Namespace(reward_type="dontcare", log_dir="/tmp/rac_debug_cem_host")
    real, sim = cem.CEMPolicy.__new__(cem.CEMPolicy), cem.SimCEMPolicy.__new__(cem.SimCEMPolicy)
    for p in (real, sim):
        p.cfg, p.debug_cem_dir, p.ep_num, p.step = cfg, cfg.log_dir, 7, 3
    return real, sim, cfg


def test_policy_row_choice_labels_and_folders():
    real, sim, cfg = _policies()
    topk_idx = np.array([9, 2, 5, 7, 1, 0, 3])
    assert list(real._plot_elites(topk_idx)) == list(topk_idx)
    assert list(sim._plot_elites(topk_idx)) == [9, 2, 5, 7, 1]          # min(K, 5)
    assert list(sim._plot_elites(topk_idx[:3])) == [9, 2, 5]
    assert real._plot_folder() == cfg.log_dir and sim._plot_folder() == cfg.log_dir + "/ep_7"
    assert not real._plot_mask_goal(_Goal([1])) and sim._plot_mask_goal(_Goal([1])) and not sim._plot_mask_goal(_Goal(None))
    cfg.reward_type = "dense"
    assert not sim._plot_mask_goal(_Goal([1]))
    T = 2
    act_seq = torch.arange(10 * T * 5, dtype=torch.float32).reshape(10, T, 5) / 1000
    opt = torch.tensor([[0.01, 0.02], [0.03, -0.04]])
    lab = by_sheet(real._plot_labels(3, T, 48, act_seq, [9, 2], opt))
    assert (0, 8, "Opt") in lab[1] and (0, 16, "X:1.0cm") in lab[1] and (0, 24, "Y:-4.0cm") in lab[2]
    assert (0, 48 + 16, f"X:{float(act_seq[9, 0, 0]) * 100:.1f}cm") in lab[1]       # Rank 0 = act_seq[topk_idx[0]]
    assert (0, 96 + 24, f"Y:{float(act_seq[2, 1, 1]) * 100:.1f}cm") in lab[2]
    lab = by_sheet(real._plot_labels(2, T, 48, act_seq, [9, 2], None))
    assert (0, 16, f"X:{float(act_seq[9, 0, 0]) * 100:.1f}cm") in lab[1] and (0, 8, "Rank 0") in lab[1]
    lab = by_sheet(sim._plot_labels(3, T, 48, act_seq, [9, 2], opt))
    assert (64, 8, "1") in lab[1] and len(lab[1]) == 9


def test_draw_labels_anchors_text_at_its_lower_left():
    sheet = np.zeros((2, 48, 192, 3), np.uint8)
    imgs = cem.draw_labels(sheet, [(1, 64, 20, "GOAL"), (1, 0, 40, "X:1.2cm")])
    assert not np.asarray(imgs[0]).any()
    ink = np.asarray(imgs[1]).any(2)
    ys, xs = np.nonzero(ink[:21])
    assert ys.max() == 19 and xs.min() == 64  # ink ends on the row above y and starts in column x
    ys, xs = np.nonzero(ink[21:])
    assert ys.max() + 21 == 39 and xs.min() == 0
    assert not sheet.any()  # the unlabelled sheet is left as it was
