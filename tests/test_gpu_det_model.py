"""GPU parity of the deterministic baselines (`--model det`, `--model copy`): DeterministicConvModel forward and train
step against the reference's golden vectors and the CPU oracle (tests/det_oracle.py), the padded ConvLSTM width (split
kernels really taken, padding exactly zero through optimiser steps, state-dict round trip), bit reproducibility, the
eval step of both baselines and the checkpoint format.

Tolerances are the project's own (tests/test_gpu_model.py, with the slope-flip reasoning written there): 1e-4 relative
for frames, losses and running statistics, GRAD_TOL per parameter and GRAD_COS for the flat gradient."""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import svg_oracle as orc  # noqa: E402
from robot_aware_control_amd import synthetic as syn  # noqa: E402
from tests import det_oracle as det  # noqa: E402

GRAD_TOL = 3e-2      # norm-wise, per parameter (tests/test_gpu_model.py)
GRAD_COS = 0.9995    # cosine of the whole flat gradient

FLAGSETS = {
    "vanilla": dict(model_use_mask=False, model_use_future_mask=False, model_use_robot_state=False,
                    reconstruction_loss="l1"),
    "ra": dict(model_use_mask=True, model_use_future_mask=True, model_use_robot_state=True,
               reconstruction_loss="dontcare_l1"),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def ns_for(cfg, dev, **extra):
    d = dict(cfg.__dict__)
    d.update(device=dev, debug_cem=False, log_dir="/tmp/rac_test_det", img_cost_threshold=None, img_cost_world_norm=True,
             experiment="train_robonet", robot_joint_dim=5, multiview=False, load_movement_info=False,
             movement_weight=1.0, scheduled_sampling=False, scheduled_sampling_k=4000, model="det", optimizer="adam",
             seed=0, wandb=False, cem_shard=True, ddp_bucket_mb=64, dynamics_model_ckpt=None)
    d.update(extra)
    return argparse.Namespace(**d)


def build_model(cfg, sd, dev, train=False):
    from robot_aware_control_amd.model import DeterministicConvModel
    m = DeterministicConvModel(ns_for(cfg, dev))
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    m.train(train)
    return m


def make_trainer(cfg, sd, dev, **extra):
    from robot_aware_control_amd.trainer import PredictionTrainer
    tr = PredictionTrainer(ns_for(cfg, dev, **extra))
    if sd is not None:
        tr.model.load_state_dict({k: v.clone() for k, v in sd.items()})
        tr.model.train()
    return tr


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def rel(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def step_inputs(cfg, data, i, dev):
    from robot_aware_control_amd.image import zero_robot_region
    x, m, s, a = (data[k].to(dev) for k in ("images", "masks", "states", "actions"))
    x_j, m_j, m_i = x[i - 1], m[i - 1], m[i]
    if "dontcare" in cfg.reconstruction_loss or cfg.black_robot_input:
        x_j = zero_robot_region(m_j, x_j)
    m_in = torch.cat([m_j, m_i], 1) if cfg.model_use_future_mask else m_j
    return x_j, m_in, s[i - 1], a[i - 1]


def reference_grads(model):
    """Every parameter's gradient under its state-dict key, in the reference's shape (the padded ones gathered)."""
    return model._export_state({k: p.grad for k, p in model.named_parameters()})


def check_grads(model, ref_sd, keys):
    grads = reference_grads(model)
    dot = na = nb = 0.0
    for k in keys:
        a, b = grads[k].double().cpu(), ref_sd[k].grad.double()
        assert a.shape == b.shape, k
        assert float((a - b).norm() / (b.norm() + 1e-20)) < GRAD_TOL, k
        dot, na, nb = dot + float((a * b).sum()), na + float((a * a).sum()), nb + float((b * b).sum())
    assert dot / np.sqrt(na * nb) > GRAD_COS


def padding_is_zero(model):
    flat, grad = model.flat_parameters()
    pad = model.padding_mask()
    return bool((flat[pad] == 0).all()) and bool((grad[pad] == 0).all())


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("tag", ["vanilla", "ra"])   # widths 66 -> 128 and 68 -> 128
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_forward_vs_reference_golden(dev, golden_dir, tag, mode):
    g = load(golden_dir, f"det_fwd_{tag}")
    cfg = orc.Cfg(g_dim=64, batch_size=2, **FLAGSETS[tag])
    model = build_model(cfg, det.make_weights(cfg, seed=7), dev, train=(mode == "train"))
    assert model.padded_width == 128
    data = syn.synth_video(seed=3, T=3, B=2)
    model.init_hidden(2)
    with torch.no_grad():
        for step in (1, 2):
            x_pred, skip = model(*step_inputs(cfg, data, step, dev), None)
            assert tuple(x_pred.shape) == (2, 4, 64, 64) and len(skip) == 4
            assert rel(x_pred[:, :, ::2], g[f"{mode}_s{step}_x_pred_rows"]) < 1e-4
            assert abs(float(x_pred.double().abs().sum().cpu()) / float(g[f"{mode}_s{step}_x_pred_abs"]) - 1) < 1e-5
            for k in range(3):
                assert abs(float(skip[k].double().abs().sum().cpu()) / float(g[f"{mode}_s{step}_skip{k}_abs"]) - 1) < 1e-5
            if step == 1:
                assert tuple(skip[3].shape) == (2, 64, 8, 8) and rel(skip[3], g[f"{mode}_s1_skip3"]) < 1e-4
    if mode == "train":
        sd = model.state_dict()
        for k in ("encoder.c1.0.main.1", "encoder.c4.2.main.1", "decoder.upc2.0.main.1", "decoder.upc5.0.main.1"):
            assert rel(sd[k + ".running_mean"], g[k + ".running_mean"]) < 1e-4
            assert rel(sd[k + ".running_var"], g[k + ".running_var"]) < 1e-4
            assert int(sd[k + ".num_batches_tracked"]) == int(g[k + ".num_batches_tracked"])


# ------------------------------------------------------------------ train step
@pytest.mark.parametrize("tag,use_truth", [("plain", None), ("fed", [True, True, False])])
def test_train_step_vs_reference_golden(dev, golden_dir, tag, use_truth):
    """g 32 (width 36 -> 64), B 2, n_past 1, n_future 2; `fed`: the second input frame is the model's own prediction."""
    g = load(golden_dir, "det_train_ra")
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, lr=1e-4, **FLAGSETS["ra"])
    tr = make_trainer(cfg, det.make_weights(cfg, seed=1, randomize_bn_stats=False), dev)
    assert tr.model.padded_width == 64
    step = tr.optimizer.step
    tr.optimizer.step = lambda: None  # first the raw gradients ...
    losses = tr._train_step(syn.synth_video(seed=20, T=3, B=2), use_truth=use_truth)
    assert set(losses) == {"recon_loss", "robot_loss", "world_loss"}
    for k in losses:
        np.testing.assert_allclose(losses[k], float(g[f"{tag}_{k}"]), rtol=1e-4)
    grads = reference_grads(tr.model)
    pk = [k for k, _, kind in det.param_spec(cfg) if not orc.is_buffer(kind)]
    gn = np.array([grads[k].double().norm().item() for k in pk])
    np.testing.assert_allclose(gn, g[f"{tag}_grad_norms"], rtol=GRAD_TOL, atol=1e-9)
    assert rel(grads["encoder.c1.0.main.0.weight"], g[f"{tag}_grad_slice_enc"]) < GRAD_TOL
    assert rel(grads["frame_predictor.lstm.1.gates.weight"][:4, :8], g[f"{tag}_grad_slice_lstm"]) < GRAD_TOL
    step()                            # ... then the weights behind the optimiser step
    sd = tr.model.state_dict()
    keys = [k for k, _, kind in det.param_spec(cfg) if kind != "bn_nbt"]
    norms = np.array([sd[k].double().norm().item() for k in keys])
    np.testing.assert_allclose(norms, g[f"{tag}_norms"], rtol=2e-4)
    assert rel(sd["encoder.c1.1.main.1.running_mean"], g[f"{tag}_rm_enc"]) < 1e-4
    assert rel(sd["decoder.upc2.0.main.1.running_var"], g[f"{tag}_rv_dec"]) < 1e-4
    assert padding_is_zero(tr.model)


@pytest.mark.parametrize("g_dim,n_future,seed", [(128, 3, 3),    # 132 -> 192: split-K and the 128-row tiles
                                                 (512, 2, 5)])   # 516 -> 576: the full-size model
def test_train_step_vs_oracle(dev, g_dim, n_future, seed):
    cfg = orc.Cfg(g_dim=g_dim, batch_size=4, n_past=1, n_future=n_future, lr=1e-4, **FLAGSETS["ra"])
    sd = det.make_weights(cfg, seed=seed, randomize_bn_stats=False)
    data = syn.synth_video(seed=9, T=n_future + 1, B=4)
    ts = det.TrainState.create(cfg, sd)
    ref = det.train_step(ts, data, None, do_update=False)
    tr = make_trainer(cfg, sd, dev)
    assert tr.model.padded_width == {128: 192, 512: 576}[g_dim]
    tr.optimizer.step = lambda: None  # compare raw gradients
    got = tr._train_step(data)
    assert set(got) == set(ref)
    for k in ref:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-4)
    check_grads(tr.model, ts.sd, ts.param_keys)
    assert padding_is_zero(tr.model)


def lstm_launches(log, gp, rows, steps):
    """Shape-log entries of the frame predictor's gate convs (ops._log_shape) on `rows` = B h w pixels: forward N = 4 Gp
    over K = (1 or 2) Gp k^2 (the first step skips the all-zero hidden half), data gradient K = 4 Gp k^2 into
    N = (1 or 2) Gp, weight gradient M = 4 Gp, N = 2 Gp k^2 over K = the pixels of 1 .. `steps` time steps.  (At these
    sizes no vgg layer has such a shape on as few pixels.)"""
    out = {"fwd": [], "dgrad": [], "wgrad": []}
    for e in log:
        kk = e["k"] * e["k"]
        if e["mode"] == "fwd" and e["M"] == rows and e["N"] == 4 * gp and e["K"] in (gp * kk, 2 * gp * kk):
            out["fwd"].append(e)
        elif e["mode"] == "dgrad" and e["M"] == rows and e["K"] == 4 * gp * kk and e["N"] in (gp, 2 * gp):
            out["dgrad"].append(e)
        elif (e["mode"] == "wgrad" and e["M"] == 4 * gp and e["N"] == 2 * gp * kk
              and e["K"] in [rows * t for t in range(1, steps + 1)]):
            out["wgrad"].append(e)
    return out


def test_gate_convs_take_the_split_kernels(dev, monkeypatch):
    """The padded width exists so that the ConvLSTM runs on the split-precision kernels: every forward, data-gradient
    and weight-gradient launch of the frame predictor must be one of theirs (a fallback to the exact-fp32 kernel fails
    here), and the same step with the split kernels switched off must agree to GRAD_TOL."""
    from robot_aware_control_amd import ops
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, lr=1e-4, **FLAGSETS["ra"])
    sd = det.make_weights(cfg, seed=1, randomize_bn_stats=False)
    data = syn.synth_video(seed=20, T=3, B=2)
    results = {}
    for split in (True, False):
        monkeypatch.setattr(ops, "SPLIT_GEMM", split)
        monkeypatch.setattr(ops, "SHAPE_LOG", [])
        tr = make_trainer(cfg, sd, dev)
        tr.optimizer.step = lambda: None
        losses = tr._train_step(data)
        torch.cuda.synchronize()
        hits = lstm_launches(ops.SHAPE_LOG, tr.model.padded_width, 2 * 8 * 8, 2)
        fams = {mode: sorted({e["family"] for e in es}) for mode, es in hits.items()}
        print("split" if split else "exact", {m: (len(es), fams[m]) for m, es in hits.items()})
        # 2 layers x 2 steps forward; backward: every launch that carries a gradient; one weight gradient per layer
        assert len(hits["fwd"]) == 4 and len(hits["dgrad"]) >= 3 and len(hits["wgrad"]) >= 2
        if split:
            assert fams == {"fwd": ["conv16"], "dgrad": ["conv16"], "wgrad": ["wgrad16"]}, fams
        else:
            assert fams == {"fwd": ["igemm"], "dgrad": ["igemm"], "wgrad": ["igemm"]}, fams
        results[split] = (losses, {k: v.clone() for k, v in reference_grads(tr.model).items()})
    (l1, g1), (l0, g0) = results[True], results[False]
    for k in l1:
        np.testing.assert_allclose(l1[k], l0[k], rtol=1e-4)
    for k in g1:
        assert float((g1[k] - g0[k]).double().norm() / (g0[k].double().norm() + 1e-20)) < GRAD_TOL, k


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop", "sgd"])
def test_padding_stays_zero_through_optimizer_steps(dev, optimizer):
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, lr=1e-4, **FLAGSETS["ra"])
    tr = make_trainer(cfg, det.make_weights(cfg, seed=1, randomize_bn_stats=False), dev, optimizer=optimizer)
    before = tr.model.flat_parameters()[0].clone()
    for step in range(3):
        losses = tr._train_step(syn.synth_video(seed=20 + step, T=3, B=2))
        assert all(np.isfinite(v) for v in losses.values())
        assert padding_is_zero(tr.model), step
    assert not torch.equal(before, tr.model.flat_parameters()[0])  # the steps did move the weights
    # reference-shaped state dict -> fresh model -> the same predictions, to the bit
    sd = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    assert tuple(sd["frame_predictor.lstm.0.gates.weight"].shape) == (4 * 36, 2 * 36, 5, 5)
    fresh = build_model(cfg, sd, dev)
    assert torch.equal(fresh.flat_parameters()[0], tr.model.flat_parameters()[0])  # nothing lost, padding zero again
    tr.model.eval()
    data = syn.synth_video(seed=3, T=3, B=2)
    preds = []
    for m in (tr.model, fresh):
        m.init_hidden(2)
        with torch.no_grad():
            preds.append([m(*step_inputs(cfg, data, i, dev), None)[0].clone() for i in (1, 2)])
    assert all(torch.equal(a, b) for a, b in zip(*preds))


def test_train_step_is_bit_reproducible(dev):
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, lr=1e-4, **FLAGSETS["ra"])
    sd = det.make_weights(cfg, seed=1, randomize_bn_stats=False)
    data = syn.synth_video(seed=20, T=3, B=2)
    grads = []
    for _ in range(2):
        tr = make_trainer(cfg, sd, dev)
        tr.optimizer.step = lambda: None
        tr._train_step(data, use_truth=[True, True, False])
        grads.append(tr.model.flat_parameters()[1].clone())
    assert bool(grads[0].abs().sum() > 0) and torch.equal(grads[0], grads[1])


# ------------------------------------------------------------------ eval
def test_eval_step_det_vs_oracle(dev):
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, **FLAGSETS["ra"])
    sd = det.make_weights(cfg, seed=7)
    tr = make_trainer(cfg, sd, dev, n_eval=4, test_batch_size=2)
    tr.model.eval()
    data = syn.synth_video(seed=31, T=4, B=2)
    data["pred_masks"] = data["masks"]
    for autoreg in (False, True):
        ref = det.eval_step(sd, cfg, data, 4, autoreg)
        got = tr._eval_step(data, autoregressive=autoreg)
        assert set(got) == set(ref) and not any("kld" in k for k in got)
        for k in ref:
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, err_msg=k)
    video = tr._eval_video({**syn.synth_video(seed=32, T=8, B=2)}, autoregressive=True)
    assert "autoreg_psnr" in video and np.isfinite(video["autoreg_psnr"]) and not any("kld" in k for k in video)


def test_eval_step_copy_vs_reference_golden(dev, golden_dir):
    g = load(golden_dir, "copy_eval")
    cfg = orc.Cfg(batch_size=2, n_past=1, n_future=2, **FLAGSETS["ra"])
    tr = make_trainer(cfg, None, dev, model="copy", n_eval=4, test_batch_size=2, data_root="synthetic", video_length=4)
    assert tr.optimizer is None and list(tr.model.parameters()) == []
    data = syn.synth_video(seed=31, T=4, B=2)
    data["pred_masks"] = data["masks"]
    for tag, autoreg in (("one", False), ("ar", True)):
        got = tr._eval_step(data, autoregressive=autoreg)
        ref = {k.split(":", 1)[1]: float(g[k]) for k in g.files if k.startswith(tag + ":")}
        assert set(got) == set(ref) and not any("kld" in k for k in got)
        for k in ref:
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, err_msg=k)
    # train() with --model copy only evaluates (trainer.py:739-741, :794-827): here the synthetic test loader
    info = tr.train()
    assert "test/autoreg_psnr" in info and np.isfinite(info["test/autoreg_psnr"]) and not any("kld" in k for k in info)


# ------------------------------------------------------------------ checkpoints
def test_checkpoint_roundtrip_and_reference_shapes(dev, tmp_path):
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, lr=1e-4, **FLAGSETS["ra"])
    sd = det.make_weights(cfg, seed=1, randomize_bn_stats=False)
    tr = make_trainer(cfg, sd, dev, log_dir=str(tmp_path))
    tr._train_step(syn.synth_video(seed=20, T=3, B=2))
    tr._step = 7
    path = tr._save_checkpoint()
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"model", "optimizer", "step"} and ck["step"] == 7
    spec = det.param_spec(cfg)
    assert list(ck["model"].keys()) == [k for k, _, _ in spec] and len(spec) == 124
    for k, shape, _ in spec:
        assert tuple(ck["model"][k].shape) == tuple(shape), k
    assert tuple(ck["model"]["frame_predictor.lstm.0.gates.weight"].shape) == (4 * 36, 2 * 36, 5, 5)
    # optimiser state keeps storage shapes
    params = list(tr.model.parameters())
    idx = next(i for i, p in enumerate(params) if p is tr.model.frame_predictor.lstm[0].gates.weight)
    assert tuple(ck["optimizer"]["state"][idx]["exp_avg"].shape) == (4 * 64, 2 * 64, 5, 5)
    tr2 = make_trainer(cfg, sd, dev, log_dir=str(tmp_path))
    assert tr2._load_checkpoint(None) == 7
    assert torch.equal(tr2.model.flat_parameters()[0], tr.model.flat_parameters()[0])
    l1 = tr._train_step(syn.synth_video(seed=21, T=3, B=2))
    tr2.model.train()
    l2 = tr2._train_step(syn.synth_video(seed=21, T=3, B=2))
    for k in ("recon_loss", "world_loss"):
        np.testing.assert_allclose(l1[k], l2[k], rtol=1e-5)
    assert torch.equal(tr2.model.flat_parameters()[0], tr.model.flat_parameters()[0])
