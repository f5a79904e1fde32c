"""TEST INFRASTRUCTURE ONLY -- golden vectors of the deterministic baselines (`--model det`, `--model copy`).

Runs only where the reference checkout is present: it loads oracle/gen_golden.py for its recipe (absent third-party
modules stubbed, the reference first on sys.path so that the name `src` is the reference's), builds the reference's
DeterministicConvModel / CopyModel / PredictionTrainer on the CPU with the name-keyed weights of tests/det_oracle.py and
writes tests/golden/det_fwd_{vanilla,ra}.npz, det_train_ra.npz and copy_eval.npz.  The reference never travels; only
these vectors do.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_det.py
"""
import importlib.util
import os
import sys

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
sys.path.append(REPO)  # behind the reference: `oracle` is this repository's, `src` stays the reference's
det = _load("det_oracle", os.path.join(REPO, "tests", "det_oracle.py"))
orc, syn = gg.orc, gg.syn

from src.prediction.models.dynamics import DeterministicConvModel  # noqa: E402

TRAINER_NS = dict(wandb=False, jobname="g", wandb_project="x", wandb_entity="x", wandb_group=None, wandb_job_type=None,
                  img_augmentation=False, seed=0, scheduled_sampling=False, scheduled_sampling_k=4000,
                  learned_robot_model=False)
GRAD_SLICES = (("enc", "encoder.c1.0.main.0.weight", (slice(None), slice(None))),
               ("lstm", "frame_predictor.lstm.1.gates.weight", (slice(0, 4), slice(0, 8))))


def gen_forward():
    """DeterministicConvModel.forward, eval + train mode, two consecutive steps at g 64, B 2, 64x64.  Frames are stored
    on every second row (the file stays the size of the svg fixtures) next to the absolute sum of the whole frame."""
    for tag, flags in gg.FLAGSETS.items():
        cfg = orc.Cfg(g_dim=64, batch_size=2, **flags)
        sd = det.make_weights(cfg, seed=7)
        data = syn.synth_video(seed=3, T=3, B=2)
        out = {}
        for mode in ("eval", "train"):
            m = DeterministicConvModel(gg.ns_for(cfg, model="det"))
            m.load_state_dict({k: v.clone() for k, v in sd.items()})
            m.train(mode == "train")
            m.init_hidden(2)
            with torch.no_grad():
                for step in (1, 2):
                    x_j, m_in, r, a = gg.step_inputs(cfg, data, step)[:4]
                    x_pred, skip = m(x_j, m_in, r, a, None)
                    out[f"{mode}_s{step}_x_pred_rows"] = x_pred[:, :, ::2].clone()
                    out[f"{mode}_s{step}_x_pred_abs"] = x_pred.double().abs().sum()
                    for k, sk in enumerate(skip[:3]):
                        out[f"{mode}_s{step}_skip{k}_abs"] = sk.double().abs().sum()
                    if step == 1:
                        out[f"{mode}_s1_skip3"] = skip[3].clone()
                    else:
                        out[f"{mode}_s2_skip3_abs"] = skip[3].double().abs().sum()
            if mode == "train":
                st = m.state_dict()
                for k in ("encoder.c1.0.main.1", "encoder.c4.2.main.1", "decoder.upc2.0.main.1", "decoder.upc5.0.main.1"):
                    out[k + ".running_mean"] = st[k + ".running_mean"].clone()
                    out[k + ".running_var"] = st[k + ".running_var"].clone()
                    out[k + ".num_batches_tracked"] = st[k + ".num_batches_tracked"].clone()
        gg.save(f"det_fwd_{tag}", **out)


def gen_train():
    """PredictionTrainer._train_step with --model det at g 32, B 2, n_past 1, n_future 2: one teacher-forced step and,
    from the same weights, one step whose second input frame is the model's own prediction (scheduled sampling)."""
    from src.prediction.trainer import PredictionTrainer
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, lr=1e-4, **gg.FLAGSETS["ra"])
    sd = det.make_weights(cfg, seed=1, randomize_bn_stats=False)
    pk = [k for k, _, kind in det.param_spec(cfg) if not orc.is_buffer(kind)]
    keys = [k for k, _, kind in det.param_spec(cfg) if kind != "bn_nbt"]
    data = syn.synth_video(seed=20, T=3, B=2)
    out = {}
    for tag, fed_back in (("plain", False), ("fed", True)):
        tr = PredictionTrainer(gg.ns_for(cfg, model="det", **dict(TRAINER_NS, scheduled_sampling=fed_back)))
        tr.model.load_state_dict({k: v.clone() for k, v in sd.items()})
        tr.model.train()
        tr._step = 0
        if fed_back:
            tr._use_true_token = lambda: False
        losses = tr._train_step(data)
        assert "kld" not in losses
        for k, v in losses.items():
            out[f"{tag}_{k}"] = v
        grads = dict(tr.model.named_parameters())
        out[f"{tag}_grad_norms"] = np.array([grads[k].grad.double().norm().item() for k in pk])
        for name, key, sl in GRAD_SLICES:
            out[f"{tag}_grad_slice_{name}"] = grads[key].grad[sl].clone()
        st = tr.model.state_dict()
        out[f"{tag}_norms"] = np.array([st[k].double().norm().item() for k in keys])
        out[f"{tag}_rm_enc"] = st["encoder.c1.1.main.1.running_mean"].clone()
        out[f"{tag}_rv_dec"] = st["decoder.upc2.0.main.1.running_var"].clone()
    gg.save("det_train_ra", **out)


def gen_copy():
    """PredictionTrainer._eval_step with --model copy (1-step and autoregressive) on synthetic.synth_video."""
    from src.prediction.trainer import PredictionTrainer
    cfg = orc.Cfg(batch_size=2, n_past=1, n_future=2, **gg.FLAGSETS["ra"])
    tr = PredictionTrainer(gg.ns_for(cfg, model="copy", n_eval=4, test_batch_size=2, **TRAINER_NS))
    data = syn.synth_video(seed=31, T=4, B=2)
    data["pred_masks"] = data["masks"]
    out = {}
    for autoreg in (False, True):
        for k, v in tr._eval_step(data, autoregressive=autoreg).items():
            assert "kld" not in k
            out[f"{'ar' if autoreg else 'one'}:{k}"] = v
    gg.save("copy_eval", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["forward", "train", "copy"]
    if "forward" in which:
        gen_forward()
    if "train" in which:
        gen_train()
    if "copy" in which:
        gen_copy()
