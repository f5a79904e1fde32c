"""GPU: the video export.  `rac_predict_frames` against numpy / torch (layout, truncation, blacking, untouched
neighbours, the frame-read form, the documented clamp), the three samples rolled as one batch against one after the
other, `predict_video` against the reference's golden vectors (svg, best of three, det, copy) and tools/export_videos.py.

Tolerances: scalars to 1e-4 relative against the reference (the project's gate, tests/test_gpu_model.py) and 1e-6 between
the two sample orders (same kernels on the same numbers; the SSIM sums use float atomics); uint8 frames by the frame
criterion of tests/predict_video_oracle.py against the reference, bit-equal between the two sample orders."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import svg_oracle as orc  # noqa: E402
from robot_aware_control_amd import synthetic as syn  # noqa: E402
from tests import det_oracle as det  # noqa: E402
from tests import predict_video_oracle as pvo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = ("gen_imgs", "true_imgs")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def ns_for(cfg, dev, **extra):
    d = dict(cfg.__dict__)
    d.update(device=dev, debug_cem=False, log_dir="/tmp/rac_test_pv", img_cost_threshold=None, img_cost_world_norm=True,
             experiment="train_robonet", robot_joint_dim=5, multiview=False, load_movement_info=False,
             movement_weight=1.0, scheduled_sampling=False, scheduled_sampling_k=4000, model="svg", optimizer="adam",
             seed=0, wandb=False, cem_shard=True, ddp_bucket_mb=64, dynamics_model_ckpt=None, n_eval=4,
             test_batch_size=2, preprocess_action="raw")
    d.update(extra)
    return argparse.Namespace(**d)


def make_trainer(cfg, sd, dev, **extra):
    from robot_aware_control_amd.trainer import PredictionTrainer
    tr = PredictionTrainer(ns_for(cfg, dev, **extra))
    if sd is not None:
        tr.model.load_state_dict({k: v.clone() for k, v in sd.items()})
    tr.model.eval()
    return tr


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


# ------------------------------------------------------------------ the kernel
SPECIAL = np.concatenate([np.array([0.0, 1.0, 1.0 - 2.0 ** -24], np.float32),
                          (np.arange(256, dtype=np.float32) / np.float32(255.0))])


def expected_u8(x, mask):
    """trainer.py:1351-1355, 1398-1407 on the CPU: zero_robot_region, 255 *, (H, W, 3), numpy's truncating cast."""
    black = orc.zero_robot_region(mask, x)
    return (255 * black).permute(0, 2, 3, 1).numpy().astype(np.uint8)


def frame_inputs(n, nt, H, W, seed):
    """Random planes with, in image 0, the values 0, 1, 1 - 2^-24 and every k/255 at the head of `prev` and `target`
    under a decoder mask channel of exactly 0 (the composite is `prev`), and in image 3 (the second sample group's
    view of video 0, if there is one) at the head of the decoder's rgb under a mask channel of exactly 1 (it is rgb).
    Elsewhere the mask channel is exactly 0 / exactly 1 / random on a third of the pixels each.  True masks: all 0
    (video 0), all 1 (video 1), mixed (the rest)."""
    g = np.random.Generator(np.random.Philox(key=[seed, 77]))
    prev, rgb, target = (g.random((b, 3, H, W), dtype=np.float32) for b in (n, n, nt))
    m = g.random((n, 1, H, W), dtype=np.float32)
    pick = g.integers(0, 3, (n, 1, H, W))
    m = np.where(pick == 0, np.float32(0), np.where(pick == 1, np.float32(1), m)).astype(np.float32)
    prev[0].reshape(-1)[:len(SPECIAL)] = SPECIAL
    target[0].reshape(-1)[:len(SPECIAL)] = SPECIAL
    m[0] = 0.0
    if n > 3:
        rgb[3].reshape(-1)[:len(SPECIAL)] = SPECIAL
        m[3] = 1.0
    x4 = torch.from_numpy(np.concatenate([rgb, m], 1)).permute(0, 2, 3, 1).contiguous()  # (n, H, W, 4)
    mask = (g.random((nt, 1, H, W), dtype=np.float32) < 0.3).astype(np.float32)
    mask[0], mask[1] = 0.0, 1.0
    return x4, torch.from_numpy(prev), torch.from_numpy(target), torch.from_numpy(mask)


def guarded_video(n, T, H, W, dev, guard=256):
    """A (n, T, H, W, 3) uint8 video inside a flat buffer filled with 0xA5, `guard` bytes behind it."""
    flat = torch.full((n * T * H * W * 3 + guard,), 0xA5, dtype=torch.uint8, device=dev)
    return flat, flat[:n * T * H * W * 3].view(n, T, H, W, 3)


def check_video(flat, video, step, want):
    got = video.cpu().numpy()
    assert np.array_equal(got[:, step], want)
    others = [t for t in range(video.shape[1]) if t != step]
    assert (got[:, others] == 0xA5).all()                      # the other steps
    assert (flat[video.numel():].cpu().numpy() == 0xA5).all()  # the bytes past the buffer


@pytest.mark.parametrize("n,nt,H,W", [(3, 3, 8, 12), (6, 3, 8, 12), (3, 3, 48, 64)])
def test_predict_frames_vs_numpy(dev, n, nt, H, W):
    from robot_aware_control_amd import ops
    T, step = 3, 1
    x4, prev, target, mask = frame_inputs(n, nt, H, W, seed=n + H)
    x4d, prevd, targetd, maskd = (t.to(dev) for t in (x4, prev, target, mask))
    want_pred = ops.Composite.apply(x4d, prevd)
    gflat, gen = guarded_video(n, T, H, W, dev)
    tflat, true = guarded_video(nt, T, H, W, dev)
    pred = ops.predict_frames(x4d, prevd, targetd, maskd, gen, true, step)
    torch.cuda.synchronize()
    assert torch.equal(pred, want_pred)  # the frame fed back: the bits of ops.Composite
    mask_n = mask.repeat(n // nt, 1, 1, 1)  # image b is blacked with true_mask[b % nt]
    want_gen = expected_u8(want_pred.cpu(), mask_n)
    check_video(gflat, gen, step, want_gen)
    check_video(tflat, true, step, expected_u8(target, mask))
    # the special values arrive: image 0 is `prev` / `target` unblacked; 1 - 2^-24 truncates to 254, not 255
    heads = [want_gen[0], expected_u8(target, mask)[0]] + ([want_gen[3]] if n > 3 else [])
    for head in heads:
        flat = np.ascontiguousarray(head.transpose(2, 0, 1)).reshape(-1)[:len(SPECIAL)]  # back to plane order
        assert flat[:3].tolist() == [0, 255, 254] and flat[3] == 0 and flat[-1] == 255
        assert (np.abs(flat[3:].astype(int) - np.arange(256)) <= 1).all() and len(np.unique(flat)) >= 250
    assert (want_gen[1] == 0).all()  # video 1 is all robot
    # x4 = NULL: the finished frame is read, not written; no true frames asked for
    gflat2, gen2 = guarded_video(n, T, H, W, dev)
    keep = pred.clone()
    out = ops.predict_frames(None, None, targetd, maskd, gen2, None, step, pred=pred)
    torch.cuda.synchronize()
    assert out is pred and torch.equal(pred, keep)
    check_video(gflat2, gen2, step, want_gen)


def test_predict_frames_clamps_what_numpy_leaves_undefined(dev):
    """Outside [0, 1] the product is clamped to [0, 255] before the cast and NaN gives 0 (include/rac_hip.h)."""
    from robot_aware_control_amd import ops
    vals = [-0.5, 1.5, float("nan"), float("inf"), -float("inf"), 300.0, -1e-9, 1.0 + 2.0 ** -20, 0.5, 1.0]
    want = [0, 255, 0, 255, 0, 255, 0, 255, 127, 255]
    n, H, W = 1, 4, 4
    frame = torch.tensor(vals + [0.25] * (3 * H * W - len(vals)), dtype=torch.float32).view(n, 3, H, W).to(dev)
    mask = torch.zeros(n, 1, H, W, device=dev)
    gen = torch.zeros(n, 1, H, W, 3, dtype=torch.uint8, device=dev)
    true = torch.zeros(n, 1, H, W, 3, dtype=torch.uint8, device=dev)
    ops.predict_frames(None, None, frame, mask, gen, true, 0, pred=frame.clone())
    for video in (gen, true):
        got = video[0, 0].permute(2, 0, 1).reshape(-1).cpu().tolist()  # back to plane order
        assert got[:len(vals)] == want and set(got[len(vals):]) == {63}
    # under the mask everything is 0, NaN included
    ops.predict_frames(None, None, frame, torch.ones_like(mask), gen, true, 0, pred=frame.clone())
    assert int(gen.max()) == 0 and int(true.max()) == 0


def test_predict_frames_refuses_bad_shapes(dev):
    from robot_aware_control_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, device=dev)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.RacError):   # step outside the video
        ops.predict_frames(z(2, 4, 8, 4), z(2, 3, 4, 8), z(2, 3, 4, 8), z(2, 1, 4, 8), u8(2, 3, 4, 8, 3), None, 3)
    with pytest.raises(_lib.RacError):   # 3 images over 2 videos
        ops.predict_frames(z(3, 4, 8, 4), z(3, 3, 4, 8), z(2, 3, 4, 8), z(2, 1, 4, 8), u8(3, 3, 4, 8, 3), None, 0)
    with pytest.raises(_lib.RacError, match="W % 4"):
        ops.predict_frames(z(2, 4, 6, 4), z(2, 3, 4, 6), z(2, 3, 4, 6), z(2, 1, 4, 6), u8(2, 3, 4, 6, 3), None, 0)


# ------------------------------------------------------------------ batched samples == sequential samples
def sequential_source(eps):
    q = [e for win in eps for sample in win for pair in sample for e in pair]
    return q, lambda shape: q.pop(0)


def batched_source(eps):
    S, steps = len(eps[0]), len(eps[0][0])
    q = [torch.cat([win[s][i][j] for s in range(S)]) for win in eps for i in range(steps) for j in (0, 1)]

    def source(shape):
        e = q.pop(0)
        assert tuple(e.shape) == tuple(shape), (e.shape, shape)
        return e
    return q, source


def run_best3(tr, data, eps, batched, monkeypatch):
    monkeypatch.setenv("RAC_PREDICT_BATCH_SAMPLES", "1" if batched else "0")
    q, tr.model.eps_source = (batched_source if batched else sequential_source)(eps)
    calls = []
    inner = tr._predict_video
    tr._predict_video = lambda *a, **k: (calls.append(k.get("num_samples", 1)), inner(*a, **k))[1]
    try:
        out = tr.predict_video(data)
    finally:
        tr._predict_video = inner
    assert not q
    return out, tr.last_best_sample, calls


@pytest.mark.parametrize("group_norm,H,T", [(False, 64, 8), (True, 48, 4)])
def test_batched_samples_equal_sequential_samples(dev, monkeypatch, group_norm, H, T):
    """B 2, S 3, n_eval 4 under finetune_*: the three samples as one batch of 6 and one after the other, fed from one
    eps table, give the same frames to the bit, the same winner and the same scalars (this path also runs the posterior
    branch, for the KL term)."""
    cfg = orc.Cfg(g_dim=64, z_dim=16, batch_size=2, n_past=1, n_future=2, image_height=H, image_width=64,
                  lstm_group_norm=group_norm, **pvo.RA_FLAGS)
    tr = make_trainer(cfg, orc.make_weights(cfg, seed=11), dev, experiment="finetune_sawyer_view")
    tr.robot_model = pvo.RolledRobotModel()
    data = syn.synth_video(seed=71, T=T, B=2, H=H, W=64)
    data["low"], data["high"] = torch.zeros(2, 5), torch.ones(2, 5)
    eps = pvo.eps_table(syn, 900, T // 4, 3, h=H // 8)
    a, win_a, calls_a = run_best3(tr, data, eps, True, monkeypatch)
    b, win_b, calls_b = run_best3(tr, data, eps, False, monkeypatch)
    assert calls_a == [3] * (T // 4) and calls_b == [1] * (3 * (T // 4))
    assert win_a == win_b
    assert set(a) == set(b) and "autoreg_kld" in a
    for k in FRAMES:
        assert len(a[k]) == len(b[k]) == T // 4
        for x, y in zip(a[k], b[k]):
            assert x.dtype == np.uint8 and x.shape == (2, 3, H, 64, 3) and np.array_equal(x, y), k
    for k in set(a) - set(FRAMES):
        print(k, a[k], b[k])
        np.testing.assert_allclose(a[k], b[k], rtol=1e-6, err_msg=k)


# ------------------------------------------------------------------ against the reference
def check_vs_golden(got, g, prefix=""):
    ref = {k[len(prefix) + 2:]: float(g[k]) for k in g.files if k.startswith(prefix + "s:")}
    assert set(got) - set(FRAMES) == set(ref) and ref
    for k in ref:
        print(k, got[k], ref[k])
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, err_msg=k)
    assert np.array_equal(np.stack(got["true_imgs"]), g[prefix + "true_imgs"])
    pvo.assert_frames_close(np.stack(got["gen_imgs"]), g[prefix + "gen_imgs"])


def test_predict_video_svg_vs_reference_golden(dev, golden_dir):
    g = load(golden_dir, "predict_video_ra")
    cfg = orc.Cfg(g_dim=64, z_dim=16, batch_size=2, n_past=1, n_future=2, **pvo.RA_FLAGS)
    tr = make_trainer(cfg, orc.make_weights(cfg, seed=7), dev)
    q, tr.model.eps_source = sequential_source(pvo.eps_table(syn, 600, 2, 1))
    got = tr.predict_video(syn.synth_video(seed=61, T=8, B=2))
    assert not q and tr.last_best_sample == 0
    check_vs_golden(got, g)


@pytest.mark.parametrize("batched", [True, False])
def test_predict_video_best_of_three_vs_reference_golden(dev, golden_dir, monkeypatch, batched):
    g = load(golden_dir, "predict_video_best3")
    cfg, sd, data = pvo.best3_problem(syn)
    tr = make_trainer(cfg, sd, dev, experiment="finetune_locobot")
    tr.robot_model = pvo.RolledRobotModel()
    got, winner, _ = run_best3(tr, data, pvo.eps_table(syn, int(g["eps_seed"]), 2, 3), batched, monkeypatch)
    assert winner == int(g["winner"])
    check_vs_golden(got, g)


@pytest.mark.parametrize("model", ["det", "copy"])
def test_predict_video_det_and_copy_vs_reference_golden(dev, golden_dir, model):
    g = load(golden_dir, "predict_video_det")
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, **pvo.RA_FLAGS)
    sd = det.make_weights(cfg, seed=7) if model == "det" else None
    tr = make_trainer(cfg, sd, dev, model=model)
    got = tr.predict_video(syn.synth_video(seed=63, T=4, B=2))
    assert not any("kld" in k for k in got)
    check_vs_golden(got, g, prefix=model + ":")


# ------------------------------------------------------------------ the export tool
def test_export_videos_tool_on_the_synthetic_loader(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_videos
    out = str(tmp_path / "videos")
    argv = ("--wandb False --batch_size 2 --test_batch_size 2 --n_future 2 --n_past 1 --n_eval 4 --model copy "
            "--reconstruction_loss dontcare_l1 --last_frame_skip True --action_dim 5 --robot_dim 5 --data_threads 0 "
            "--model_use_robot_state True --model_use_mask True --model_use_future_mask True --video_length 8 "
            f"--image_height 64 --image_width 64 --data_root synthetic --log_dir {tmp_path / 'log'} --out {out}").split()
    export_videos.main(argv)
    true, gen = np.load(os.path.join(out, "true_imgs.npy")), np.load(os.path.join(out, "gen_imgs.npy"))
    # the synthetic test set: 2 batches of test_batch_size videos, 8 frames = 2 windows of n_eval 4
    assert true.dtype == gen.dtype == np.uint8 and true.shape == gen.shape == (2 * 2 * 2, 3, 64, 64, 3)
    assert true.any() and gen.any() and not np.array_equal(true, gen)
    metrics = json.load(open(os.path.join(out, "metrics.json")))
    assert {"autoreg_psnr", "autoreg_ssim", "autoreg_world_loss", "1_step_psnr", "2_step_world_loss"} <= set(metrics)
    assert all(np.isfinite(v) for v in metrics.values())
