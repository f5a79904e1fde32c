"""Host half of the sampled evaluation (`--eval_best_of_three`, reference trainer.py:491-564): the flag, the selection
rule of `_eval_video`, the window bookkeeping around a stubbed `_eval_step`, the table-to-scalars helper of
`rac_eval_frames` against a numpy restatement, and the ctypes signature."""
import argparse
from collections import defaultdict

import numpy as np
import pytest
import torch


def test_flag_parses_and_defaults_to_false():
    from robot_aware_control_amd import config
    d, _ = config.argparser([])
    assert d.eval_best_of_three is False
    on, unparsed = config.argparser(["--eval_best_of_three", "True"])
    assert on.eval_best_of_three is True and unparsed == []
    off, _ = config.argparser(["--eval_best_of_three", "False"])
    assert off.eval_best_of_three is False


def test_sigs_carry_rac_eval_frames():
    import ctypes as C

    from robot_aware_control_amd import EXPORTS, _lib
    i32, vp, f32 = C.c_int32, C.c_void_p, C.c_float
    assert "rac_eval_frames" in EXPORTS
    assert _lib._SIGS["rac_eval_frames"] == [i32, vp, vp, vp, f32, vp, i32, i32, i32, i32, vp]
    assert _lib.ABI_VERSION == 12  # a new symbol within version 12


def test_selection_is_by_psnr_descending_and_ties_keep_the_first():
    from robot_aware_control_amd.trainer import PredictionTrainer
    pick = PredictionTrainer._best_eval_sample
    mk = lambda psnr, world: defaultdict(float, autoreg_psnr=psnr, autoreg_world_loss=world)
    # descending by psnr; the world loss (what predict_video sorts by) points the other way and is ignored
    assert pick([mk(20.0, 0.1), mk(25.0, 0.9), mk(22.0, 0.5)]) == 1
    assert pick([mk(20.0, 0.9), mk(19.0, 0.1), mk(18.0, 0.2)]) == 0
    assert pick([mk(1.0, 0.0), mk(2.0, 0.0), mk(3.0, 0.0)]) == 2
    # ties keep the earlier sample
    assert pick([mk(20.0, 0.3), mk(25.0, 0.2), mk(25.0, 0.1)]) == 1
    assert pick([mk(7.0, 0.3), mk(7.0, 0.2), mk(7.0, 0.1)]) == 0
    # nothing is sorted when the evaluation is not an autoregressive svg one (trainer.py:558)
    assert pick([mk(1.0, 0.0), mk(2.0, 0.0), mk(3.0, 0.0)], by_psnr=False) == 0


def stub_trainer(**cfg):
    from robot_aware_control_amd.trainer import PredictionTrainer
    tr = object.__new__(PredictionTrainer)
    base = dict(n_past=1, n_future=2, n_eval=3, model_use_heatmap=False, experiment="finetune_locobot", model="svg",
                model_use_mask=True, model_use_robot_state=True, preprocess_action="raw", eval_best_of_three=True)
    base.update(cfg)
    tr._config = argparse.Namespace(**base)

    class Robot:
        calls = 0

        def predict_batch(self, bd):
            Robot.calls += 1
            return bd["states"], bd["masks"]
    tr.robot_model = Robot()
    return tr, Robot


def video(T=6, B=2):
    return {"images": torch.zeros(T, B, 3, 4, 4), "states": torch.zeros(T, B, 5), "actions": torch.zeros(T - 1, B, 5),
            "masks": torch.zeros(T, B, 1, 4, 4), "qpos": torch.zeros(T, B, 5), "robot": ["a", "b"], "folder": ["f", "f"],
            "low": torch.zeros(B, 5), "high": torch.ones(B, 5)}


@pytest.mark.parametrize("batched", [True, False])
def test_eval_video_accumulates_per_sample_and_divides_the_winner(monkeypatch, batched):
    """Two windows, three samples: per-sample sums over the windows, the winner by summed psnr (sample 1 wins the sum
    although sample 2 wins the first window), divided by the window count; the robot model is asked once per window;
    `RAC_PREDICT_BATCH_SAMPLES=0` asks `_eval_step` for one sample three times per window."""
    monkeypatch.setenv("RAC_PREDICT_BATCH_SAMPLES", "1" if batched else "0")
    tr, robot = stub_trainer()
    psnr = [[20.0, 22.0, 24.0], [20.0, 26.0, 21.0]]  # [window][sample]
    asked, draws = [], []

    def eval_step(bd, autoreg, num_samples=None):
        assert autoreg and num_samples is not None and "pred_masks" in bd
        asked.append(num_samples)
        out = []
        for _ in range(num_samples):
            n = len(draws) % 3
            win = len(draws) // 3
            draws.append(n)
            out.append({"autoreg_psnr": psnr[win][n], "autoreg_world_loss": float(n), "1_step_psnr": 10.0 * n})
        return out
    tr._eval_step = eval_step
    got = tr._eval_video(video(), autoregressive=True)
    assert asked == ([3, 3] if batched else [1] * 6) and robot.calls == 2
    assert tr.last_best_eval_sample == 1
    assert dict(got) == {"autoreg_psnr": (22.0 + 26.0) / 2, "autoreg_world_loss": 1.0, "1_step_psnr": 10.0}


@pytest.mark.parametrize("change", [dict(eval_best_of_three=False), dict(model="det"), dict(experiment="train_robonet"),
                                    dict(autoregressive=False)])
def test_one_sample_when_the_flag_is_off_or_the_run_does_not_qualify(change):
    """The flag off, `--model det`, a non-finetune experiment or a one-step evaluation: `_eval_step` is called as it
    always was (two positional arguments), once per window."""
    autoregressive = change.pop("autoregressive", True)
    tr, _ = stub_trainer(**change)
    calls = []
    tr._eval_step = lambda bd, autoreg: calls.append(autoreg) or {"autoreg_psnr": 3.0}
    got = tr._eval_video(video(), autoregressive=autoregressive)
    assert calls == [autoregressive] * 2 and dict(got) == {"autoreg_psnr": 3.0}
    assert tr.last_best_eval_sample == 0


# ------------------------------------------------------------------ the table-to-scalars helper
def numpy_scalars(rows, dontcare, n_values, index=None):
    """losses.py:11-78 and src/utils/metrics.py:61-78 on the per-video sums, in float64."""
    r = np.asarray(rows, np.float64)
    if index is not None:
        r = r[..., list(index), :]
    main, rob2, world2, rob_n, se = (r[..., k] for k in range(5))
    world_n = n_values - rob_n
    recon = main / (world_n + 1) if dontcare else main / n_values
    return {"recon_loss": recon.mean(-1), "robot_loss": (rob2 / (rob_n + 1)).mean(-1),
            "world_loss": (world2 / (world_n + 1)).mean(-1),
            "psnr": (10 * np.log10(1 / (se / n_values))).mean(-1),
            "ssim": r[..., 5:8].sum(-1).sum(-1) / (r.shape[-2] * n_values)}


def test_table_scalars_match_a_numpy_restatement():
    from robot_aware_control_amd import metrics
    g = np.random.Generator(np.random.Philox(key=[5, 77]))
    n_values = 3 * 12 * 20
    rows = np.empty((4, 3, 5, 8), np.float32)  # (steps, samples, videos, columns)
    rows[..., 3] = 3 * g.integers(0, 12 * 20 + 1, rows.shape[:-1])  # robot values: whole pixels
    rows[0, 0, 0, 3], rows[0, 0, 1, 3] = 0.0, n_values              # no robot pixel; no world pixel (the `+ 1`)
    for k in (0, 1, 2, 4):
        rows[..., k] = g.random(rows.shape[:-1], dtype=np.float32) * 50 + 0.01
    rows[..., 5:8] = g.random(rows.shape[:-1] + (3,), dtype=np.float32) * 12 * 20
    t = torch.from_numpy(rows)
    for kind, dontcare in ((0, False), (1, False), (2, True), (3, True)):
        for index in (None, [0, 3], [2], np.array([4, 1, 0])):
            got = metrics.table_scalars(t, kind, n_values, index=index)
            want = numpy_scalars(rows, dontcare, n_values, index)
            assert set(got) == set(want) == {"recon_loss", "robot_loss", "world_loss", "psnr", "ssim"}
            for k in want:
                assert got[k].shape == (4, 3) and got[k].dtype == torch.float32
                np.testing.assert_allclose(got[k].numpy(), want[k], rtol=2e-6, err_msg=f"{k} kind {kind} index {index}")
    # a group's numbers do not depend on the groups next to it
    alone = metrics.table_scalars(t[1:2, 2:3], 3, n_values)
    among = metrics.table_scalars(t, 3, n_values)
    for k in alone:
        assert torch.equal(alone[k], among[k][1:2, 2:3])
