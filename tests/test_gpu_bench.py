"""A plain `bench.py --gpus 1` run: the headline workload alone (what `--full` adds does not run), `--steps` timed
steps, and `--dump-outputs DIR`: what the last timed step computed, the same inputs from run to run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "RAC_DIST_FORCE", "RAC_BENCH_ONE_GPU"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", out_dir]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(out_dir, "*.npy")))}
    return json.loads(lines[0]), arrays


def test_plain_bench_headline_and_dumped_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out, got = _run(str(tmp_path / "a"))
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"].startswith("fp32")
    assert out["ms_per_step"] > 0 and abs(out["value"] - 16 * 6 / (out["ms_per_step"] / 1e3)) < 1e-6 * out["value"]
    for key in ("cem", "cem_ra", "side", "fp32_exact", "cpu_baseline", "arith_error", "ddp_modes"):
        assert key not in out, key
    # the train step's loss terms (float64) and the model's state after it (float32, whole or a fixed sample)
    losses = {k: v for k, v in got.items() if k.startswith("train.loss.")}
    state = {k: v for k, v in got.items() if k.startswith("train.state.")}
    assert {"train.loss.recon_loss", "train.loss.kld"} <= set(losses) and len(state) > 100
    assert all(v.dtype == np.float64 and v.shape == (1,) for v in losses.values())
    assert all(v.dtype == np.float32 and 0 < v.size <= 1 << 17 for v in state.values())
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20 and set(got) == set(losses) | set(state)
    # the same arguments, the same inputs: a second run computes the same losses (up to the order of atomic sums)
    _, again = _run(str(tmp_path / "b"))
    assert set(again) == set(got) and all(again[k].shape == got[k].shape for k in got)
    for k in losses:
        assert np.allclose(again[k], got[k], rtol=1e-3, atol=1e-9), (k, again[k], got[k])
