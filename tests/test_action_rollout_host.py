"""CPU: the host half of the action-sweep probe -- `action_rollout.sweep_actions` against the reference's loop
(test_action_rollout.py:196-213) restated here, the numpy sheet reference of tests/action_rollout_refs.py on a case
worked out by hand, the command line's flag split, `response.json` from a hand-made table, and the ABI entry."""
import json
import os

import numpy as np
import pytest
import torch

from tests import action_rollout_refs as refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_and_bound():
    from robot_aware_control_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rac_hip.h")).read()
    assert "int rac_action_rollout_sheet(" in hdr and "#define RAC_ABI_VERSION 12" in hdr
    assert len(_lib._SIGS["rac_action_rollout_sheet"]) == 14 and _lib.ABI_VERSION == 12
    assert hasattr(_lib.load(), "rac_action_rollout_sheet")


def test_sweep_actions_names_order_and_columns():
    from robot_aware_control_amd.action_rollout import sweep_actions
    g = torch.Generator().manual_seed(3)
    actions = torch.randn(4, 3, 5, generator=g)
    keep = actions.clone()
    names, sets = sweep_actions(actions)
    assert names == ["recorded", "x_-20mm", "y_-20mm", "x_20mm", "y_20mm"]
    assert tuple(sets.shape) == (5, 4, 3, 5) and torch.equal(actions, keep)
    assert torch.equal(sets[0], actions)
    for s, (axis, value) in enumerate([(0, -0.02), (1, -0.02), (0, 0.02), (1, 0.02)], start=1):
        want = torch.zeros_like(actions)
        want[:, :, 2] = actions[:, :, 2]  # the recorded z
        want[:, :, axis] = value
        assert torch.equal(sets[s], want), names[s]
    names, sets = sweep_actions(actions, include_recorded=False)
    assert names == ["x_-20mm", "y_-20mm", "x_20mm", "y_20mm"] and sets.shape[0] == 4
    names, sets = sweep_actions(actions, step_size=0.015, axes=("y",), directions=(1,), include_recorded=False)
    assert names == ["y_15mm"] and torch.equal(sets[0, :, :, 1], torch.full((4, 3), 0.015))
    assert not sets[0, :, :, [0, 3, 4]].any()
    with pytest.raises(ValueError):
        sweep_actions(actions, axes=("z",))


def test_sheet_reference_on_a_case_worked_out_by_hand():
    """One sweep, two sample columns, two videos of 1 x 2 pixels: every byte of the sheet written down."""
    truth = np.zeros((1, 2, 3, 1, 2), np.float32)
    gen = np.zeros((1, 2, 1, 2, 3, 1, 2), np.float32)
    truth[0, 0, :, 0, :] = [[0.0, 1.0], [0.5, 2.0], [-1.0, 100 / 255]]   # (channel, x)
    truth[0, 1] = 1.0
    gen[0, 0, 0, 0] = 0.25
    gen[0, 1, 0, 0] = np.nan
    gen[0, 0, 0, 1, 1] = 1 - 2.0 ** -24
    gen[0, 1, 0, 1, 2] = 3 / 255
    sheet = refs.sheet_ref(truth, gen)
    assert sheet.shape == (1, 1, 2, 3 * 2 + 2, 3) and sheet.dtype == np.uint8
    W = [255, 255, 255]
    v = int(np.float32(100 / 255) * np.float32(255))
    w = int(np.float32(3 / 255) * np.float32(255))
    assert sheet[0, 0].tolist() == [
        [[0, 127, 0], [255, 255, v], W, [63, 63, 63], [63, 63, 63], W, [0, 0, 0], [0, 0, 0]],
        [W, W, W, [0, 254, 0], [0, 254, 0], W, [0, 0, w], [0, 0, w]]]


def test_response_reference_and_bound():
    gen = np.zeros((2, 1, 1, 1, 3, 1, 4), np.float32)
    gen[1] = 0.5
    gen[1, 0, 0, 0, 0, 0, 0] = -1.0
    r = refs.response_ref(gen, 0)
    assert r.shape == (2, 1, 1, 1) and r[0, 0, 0, 0] == 0.0 and r[1, 0, 0, 0] == (11 * 0.5 + 1.0) / 12
    assert refs.response_bound(1, 4) == pytest.approx(24 * 2.0 ** -24, rel=1e-5)
    assert refs.response_bound(48, 64) == pytest.approx(48 * 2.0 ** -24, rel=1e-5)


def test_flag_split_and_unknown_flags():
    from src.prediction import test_action_rollout as cli
    config, tool = cli.parse_args(["--model", "det", "--step_size", "0.01", "--batch_size", "3", "--nsample", "2",
                                   "--lstm_group_norm", "True", "--out", "somewhere"])
    assert (tool.step_size, tool.video_len, tool.nsample, tool.include_recorded, tool.out) == (0.01, 5, 2, True, "somewhere")
    assert config.model == "det" and config.batch_size == 3 and config.lstm_group_norm is True
    assert not hasattr(config, "step_size") and not hasattr(tool, "model")
    _, tool = cli.parse_args(["--include_recorded", "False"])
    assert tool.include_recorded is False and tool.step_size == 0.02 and tool.out == "."
    with pytest.raises(AssertionError):
        cli.parse_args(["--no_such_flag", "1"])


def test_response_json_from_a_hand_made_table(tmp_path):
    from robot_aware_control_amd.action_rollout import ActionRollout, response_summary
    names = ["recorded", "x_20mm"]
    table = np.zeros((2, 2, 3, 2), np.float32)          # (sweep, sample, step, video)
    table[1, :, 1] = [[1.0, 2.0], [3.0, 6.0]]           # step 1: mean 3
    table[1, :, 2] = [[0.5, 0.5], [0.5, 2.5]]           # step 2: mean 1
    want = {"base": "recorded", "shape": [2, 2, 3, 2], "layout": ["sweep", "sample", "step", "video"],
            "sweeps": {"recorded": {"per_step": [0.0, 0.0, 0.0], "mean": 0.0},
                       "x_20mm": {"per_step": [0.0, 3.0, 1.0], "mean": 4.0 / 3}}}
    assert response_summary(names, table, "recorded") == want
    sheets = np.zeros((2, 3, 4, 2 * 3 + 2, 3), np.uint8)  # b H = 4 rows, [truth | 2 samples] of width 2
    sheets[1, 1], sheets[1, 2] = 100, 200               # (the GIF writer merges frames that repeat)
    files = ActionRollout(names, None, sheets, table).write(str(tmp_path / "out"))
    assert [os.path.basename(f) for f in files] == ["recorded.gif", "x_20mm.gif", "response.json"]
    assert json.load(open(files[2])) == want
    from PIL import Image
    im = Image.open(files[1])
    assert im.n_frames == 3 and im.size == (8, 4) and im.info["duration"] == 250
    # without a recorded sweep there is no table and no response.json
    files = ActionRollout(names[1:], None, sheets[1:], None).write(str(tmp_path / "plain"))
    assert [os.path.basename(f) for f in files] == ["x_20mm.gif"]
