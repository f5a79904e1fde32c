"""CPU: the deterministic baselines without a GPU -- tests/det_oracle.py against the reference's own outputs
(tests/golden/det_*.npz, copy_eval.npz; tolerances of tests/test_oracle_golden.py), the padded parameter storage of
DeterministicConvModel (reference shapes in, reference shapes out, zeros everywhere else) and the configuration errors."""
import argparse
import os

import numpy as np
import pytest
import torch

from oracle import svg_oracle as orc
from robot_aware_control_amd import synthetic as syn
from tests import det_oracle as det

FLAGSETS = {
    "vanilla": dict(model_use_mask=False, model_use_future_mask=False, model_use_robot_state=False,
                    reconstruction_loss="l1"),
    "ra": dict(model_use_mask=True, model_use_future_mask=True, model_use_robot_state=True,
               reconstruction_loss="dontcare_l1"),
}


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def close(a, b, rtol=1e-6, atol=1e-7):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=rtol, atol=atol)


def step_inputs(cfg, data, i):
    x, m, s, a = data["images"], data["masks"], data["states"], data["actions"]
    x_j, m_j, m_i = x[i - 1], m[i - 1], m[i]
    if "dontcare" in cfg.reconstruction_loss or cfg.black_robot_input:
        x_j = orc.zero_robot_region(m_j, x_j)
    m_in = torch.cat([m_j, m_i], 1) if cfg.model_use_future_mask else m_j
    return x_j, m_in, s[i - 1], a[i - 1]


def _ns(**kw):
    d = dict(device=torch.device("cpu"), image_width=64, image_height=64, channels=3, model_use_mask=True,
             model_use_future_mask=True, model_use_heatmap=False, model_use_future_heatmap=False,
             model_use_robot_state=True, model_use_future_robot_state=False, g_dim=32, z_dim=16, action_dim=5,
             robot_dim=5, batch_size=2, lstm_group_norm=False, last_frame_skip=True, model="det")
    d.update(kw)
    return argparse.Namespace(**d)


# ------------------------------------------------------------------ the oracle against the reference
@pytest.mark.parametrize("tag", ["vanilla", "ra"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_oracle_forward(golden_dir, tag, mode):
    g = load(golden_dir, f"det_fwd_{tag}")
    cfg = orc.Cfg(g_dim=64, batch_size=2, **FLAGSETS[tag])
    sd = det.make_weights(cfg, seed=7)
    data = syn.synth_video(seed=3, T=3, B=2)
    hidden = det.init_hidden(cfg, 2)
    training = mode == "train"
    with torch.no_grad():
        for step in (1, 2):
            x4, skip = det.det_forward(sd, cfg, hidden, *step_inputs(cfg, data, step), None, training=training)
            close(x4[:, :, ::2], g[f"{mode}_s{step}_x_pred_rows"])
            close(x4.double().abs().sum(), g[f"{mode}_s{step}_x_pred_abs"], rtol=1e-7)
            for k in range(3):
                close(skip[k].double().abs().sum(), g[f"{mode}_s{step}_skip{k}_abs"], rtol=1e-7)
            if step == 1:
                close(skip[3], g[f"{mode}_s1_skip3"])
            else:
                close(skip[3].double().abs().sum(), g[f"{mode}_s2_skip3_abs"], rtol=1e-7)
    if training:
        for k in ("encoder.c1.0.main.1", "encoder.c4.2.main.1", "decoder.upc2.0.main.1", "decoder.upc5.0.main.1"):
            close(sd[k + ".running_mean"], g[k + ".running_mean"])
            close(sd[k + ".running_var"], g[k + ".running_var"])
            assert int(sd[k + ".num_batches_tracked"]) == int(g[k + ".num_batches_tracked"]) == 2


@pytest.mark.parametrize("tag,use_truth", [("plain", None), ("fed", [True, True, False])])
def test_oracle_train_step(golden_dir, tag, use_truth):
    g = load(golden_dir, "det_train_ra")
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, lr=1e-4, **FLAGSETS["ra"])
    sd = det.make_weights(cfg, seed=1, randomize_bn_stats=False)
    ts = det.TrainState.create(cfg, sd)
    losses = det.train_step(ts, syn.synth_video(seed=20, T=3, B=2), use_truth=use_truth)
    assert set(losses) == {"recon_loss", "robot_loss", "world_loss"}
    for k in losses:
        close(losses[k], g[f"{tag}_{k}"], rtol=2e-5)
    pk = [k for k, _, kind in det.param_spec(cfg) if not orc.is_buffer(kind)]
    close(np.array([ts.sd[k].grad.double().norm().item() for k in pk]), g[f"{tag}_grad_norms"], rtol=1e-4, atol=1e-10)
    close(ts.sd["encoder.c1.0.main.0.weight"].grad, g[f"{tag}_grad_slice_enc"], rtol=1e-3, atol=1e-7)
    close(ts.sd["frame_predictor.lstm.1.gates.weight"].grad[:4, :8], g[f"{tag}_grad_slice_lstm"], rtol=1e-3, atol=1e-7)
    keys = [k for k, _, kind in det.param_spec(cfg) if kind != "bn_nbt"]
    close(np.array([ts.sd[k].detach().double().norm().item() for k in keys]), g[f"{tag}_norms"], rtol=1e-4)
    close(ts.sd["encoder.c1.1.main.1.running_mean"], g[f"{tag}_rm_enc"], rtol=1e-5, atol=1e-8)
    close(ts.sd["decoder.upc2.0.main.1.running_var"], g[f"{tag}_rv_dec"], rtol=1e-5, atol=1e-8)


def test_oracle_copy_eval(golden_dir):
    g = load(golden_dir, "copy_eval")
    cfg = orc.Cfg(batch_size=2, n_past=1, n_future=2, **FLAGSETS["ra"])
    data = syn.synth_video(seed=31, T=4, B=2)
    for autoreg, pre in ((False, "one:"), (True, "ar:")):
        ref = {k[len(pre):]: float(g[k]) for k in g.files if k.startswith(pre)}
        got = det.eval_step(None, cfg, data, 4, autoreg, model="copy")
        assert set(got) == set(ref) and not any("kld" in k for k in got)
        for k in ref:
            close(got[k], ref[k], rtol=1e-5)


# ------------------------------------------------------------------ padded storage
@pytest.mark.parametrize("use_state", [False, True])  # widths g + 2 and g + 4
def test_padded_storage_round_trip(use_state):
    from robot_aware_control_amd.model import DeterministicConvModel, det_padded_width
    ns = _ns(model_use_robot_state=use_state)
    cfg = orc.cfg_from_namespace(ns)
    m = DeterministicConvModel(ns)
    w = 32 + (4 if use_state else 2)
    assert (m.width, m.padded_width) == (w, 64) == (det.width(cfg), det_padded_width(w))
    spec = det.param_spec(cfg)
    sd0 = m.state_dict()
    assert list(sd0.keys()) == [k for k, _, _ in spec] and len(spec) == (124 if use_state else 122)
    for k, shape, _ in spec:
        assert tuple(sd0[k].shape) == tuple(shape), k
    assert tuple(m.frame_predictor.lstm[0].gates.weight.shape) == (256, 128, 5, 5)   # stored: (4 Gp, 2 Gp, k, k)
    assert tuple(m.decoder.upc2[0].main[0].weight.shape) == (512, 64, 3, 3)
    flat, _ = m.flat_parameters()
    pad = m.padding_mask()
    n_pad = 2 * (64 - w) * 4 + sum((4 * 64 * 2 * 64 - 4 * w * 2 * w) * k * k for k in (5, 3)) + 512 * (64 - w) * 9
    assert int(pad.sum()) == n_pad
    assert bool((flat[pad] == 0).all())  # the initialiser's draws never reach the padding
    ws = det.make_weights(cfg, seed=3)
    m.load_state_dict({k: v.clone() for k, v in ws.items()})
    sd1 = m.state_dict()
    for k in ws:
        assert torch.equal(sd1[k], ws[k]), k
    assert bool((flat[pad] == 0).all())
    # the gathered tensors are copies: writing to them does not reach the parameters
    sd1["frame_predictor.lstm.0.gates.weight"].zero_()
    assert torch.equal(m.state_dict()["frame_predictor.lstm.0.gates.weight"], ws["frame_predictor.lstm.0.gates.weight"])
    # dirt in the padding is removed by the next load
    with torch.no_grad():
        flat[pad] = 1.0
    m.load_state_dict({k: v.clone() for k, v in ws.items()})
    assert bool((flat[pad] == 0).all())
    # a storage-shaped tensor is not a state dict entry
    bad = {k: v.clone() for k, v in ws.items()}
    bad["frame_predictor.lstm.1.gates.bias"] = torch.zeros(4 * 64)
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad)


def test_padding_blocks_are_per_gate_and_per_input_half():
    from robot_aware_control_amd.model import pad_gate_param, unpad_gate_param
    w, p = 6, 8
    t = torch.arange(4 * w * 2 * w * 9, dtype=torch.float32).reshape(4 * w, 2 * w, 3, 3) + 1
    full = pad_gate_param(t, w, p)
    assert tuple(full.shape) == (4 * p, 2 * p, 3, 3)
    for gate in range(4):
        for half in range(2):
            blk = full[gate * p:(gate + 1) * p, half * p:(half + 1) * p]
            assert torch.equal(blk[:w, :w], t[gate * w:(gate + 1) * w, half * w:(half + 1) * w])
            assert bool((blk[w:] == 0).all()) and bool((blk[:, w:] == 0).all())
    assert torch.equal(unpad_gate_param(full, w, p), t)
    b = torch.arange(4 * w, dtype=torch.float32) + 1
    assert torch.equal(unpad_gate_param(pad_gate_param(b, w, p), w, p), b)
    assert bool((pad_gate_param(b, w, p).view(4, p)[:, w:] == 0).all())


def test_optimizer_state_with_reference_shapes_is_refused():
    """Optimiser state lives at storage shapes; a state dict with the reference's shapes raises before anything is copied."""
    from robot_aware_control_amd.model import DeterministicConvModel
    from robot_aware_control_amd.optim import FusedAdam
    m = DeterministicConvModel(_ns())
    opt = FusedAdam(m, lr=1e-4)
    opt._steps = 1
    mom, _ = opt._moments()
    mom.fill_(0.25)
    good = opt.state_dict()
    opt.load_state_dict(good)  # storage shapes load
    params = list(m.parameters())
    idx = next(i for i, p in enumerate(params) if p is m.frame_predictor.lstm[0].gates.weight)
    bad = {"state": {k: dict(v) for k, v in good["state"].items()}, "param_groups": good["param_groups"]}
    for k in bad["state"]:
        bad["state"][k] = {n: (torch.full_like(t, 0.75) if t.dim() else t) for n, t in bad["state"][k].items()}
    bad["state"][idx]["exp_avg"] = torch.full((4 * 36, 2 * 36, 5, 5), 0.75)
    with pytest.raises(ValueError):
        opt.load_state_dict(bad)
    assert bool((opt._moments()[0] == 0.25).all())  # nothing was copied


# ------------------------------------------------------------------ configuration errors
def test_config_errors():
    from robot_aware_control_amd.model import CopyModel, DeterministicConvModel
    from robot_aware_control_amd.trainer import PredictionTrainer
    with pytest.raises(ValueError, match="divisible by num_groups"):
        DeterministicConvModel(_ns(lstm_group_norm=True))
    with pytest.raises(ValueError):
        DeterministicConvModel(_ns(image_width=128, image_height=128))
    with pytest.raises(ValueError, match="cdna_det"):
        PredictionTrainer.__new__(PredictionTrainer)._init_models(_ns(model="cdna_det"))
    assert list(CopyModel().parameters()) == []
    from src.prediction.models import dynamics
    assert dynamics.DeterministicConvModel is DeterministicConvModel and dynamics.CopyModel is CopyModel
