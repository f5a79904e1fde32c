"""TEST INFRASTRUCTURE ONLY -- golden vectors of the video export (`PredictionTrainer.predict_video`).

Runs only where the reference checkout is present: it loads oracle/gen_golden.py for its recipe (absent third-party
modules stubbed, the reference first on sys.path, `Tensor.normal_` popping injected draws), builds the reference's
PredictionTrainer on the CPU with the name-keyed weights, runs the reference's OWN `predict_video` on
`synthetic.synth_video` / `synthetic.synth_eps` (the three-sample fixture on predict_video_oracle.best3_problem) and writes tests/golden/predict_video_{ra,best3,det}.npz.  The reference
never travels; only these vectors do.

The three-sample fixture goes through the reference's own `predict_video` with `experiment="finetune_locobot"` and a
stand-in robot model (tests/predict_video_oracle.py: RolledRobotModel).  The reference trainer's constructor would build
the MuJoCo-backed LocobotAnalyticalModel for that experiment, so the trainer is constructed as `train_robonet` and the
experiment name and `robot_model` are set on it before the call: selection, window sums and averaging are the
reference's code, nothing of them is restated here.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_predict_video.py
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
pvo = _load("predict_video_oracle", os.path.join(REPO, "tests", "predict_video_oracle.py"))
orc, syn = gg.orc, gg.syn

from src.prediction.trainer import PredictionTrainer  # noqa: E402

TRAINER_NS = dict(wandb=False, jobname="g", wandb_project="x", wandb_entity="x", wandb_group=None, wandb_job_type=None,
                  img_augmentation=False, seed=0, scheduled_sampling=False, scheduled_sampling_k=4000,
                  learned_robot_model=False, n_eval=4, test_batch_size=2, preprocess_action="raw")
BEST3_GAP = 1e-2  # least relative gap between the best and the second-best summed world loss


def eps_table(seed, windows, samples):
    return pvo.eps_table(syn, seed, windows, samples)


def queue(eps):
    """The draws in the order predict_video consumes them: window, sample, step, prior then posterior."""
    return [e for win in eps for sample in win for pair in sample for e in pair]


def trainer_for(cfg, sd, model):
    tr = PredictionTrainer(gg.ns_for(cfg, model=model, **TRAINER_NS))
    if sd is not None:
        tr.model.load_state_dict({k: v.clone() for k, v in sd.items()})
        tr.model.eval()
    return tr


def scalars(info):
    return {k: v for k, v in info.items() if k not in ("gen_imgs", "true_imgs")}


def gen_ra():
    """svg, RA flags, g 64, z 16, B 2, 64x64, n_eval 4, T 8 (two windows), one sample."""
    cfg = orc.Cfg(g_dim=64, z_dim=16, batch_size=2, n_past=1, n_future=2, **gg.FLAGSETS["ra"])
    tr = trainer_for(cfg, orc.make_weights(cfg, seed=7), "svg")
    data = syn.synth_video(seed=61, T=8, B=2)
    gg._EPS.extend(queue(eps_table(600, 2, 1)))
    info = tr.predict_video(data)
    assert not gg._EPS and len(info["gen_imgs"]) == 2
    out = {f"s:{k}": v for k, v in scalars(info).items()}
    out["gen_imgs"], out["true_imgs"] = np.stack(info["gen_imgs"]), np.stack(info["true_imgs"])
    gg.save("predict_video_ra", **out)


def gen_best3():
    """The three-sample path (svg under finetune_locobot) on predict_video_oracle.best3_problem, two windows: every
    sample's summed autoreg_world_loss, the winner's index, its scalars and frames.  The eps seed is the first of a
    short list for which the best and second-best summed world losses differ by at least BEST3_GAP relative (stored as
    `gap`) and the winner is not sample 0 (which a selection that never sorts would return)."""
    cfg, sd, data = pvo.best3_problem(syn)
    for seed in (700, 800, 900, 1000, 1100, 1200):
        tr = trainer_for(cfg, sd, "svg")
        tr._config.experiment = "finetune_locobot"
        tr.robot_model = pvo.RolledRobotModel()
        world = []
        inner = tr._predict_video

        def spy(batch):
            r = inner(batch)
            world.append(r["autoreg_world_loss"])
            return r
        tr._predict_video = spy
        gg._EPS.extend(queue(eps_table(seed, 2, 3)))
        info = tr.predict_video(data)
        assert not gg._EPS and len(world) == 6
        sums = np.array(world).reshape(2, 3).sum(0)  # calls come window-major, sample-minor
        srt = np.sort(sums)
        gap = (srt[1] - srt[0]) / srt[0]
        print("seed", seed, "summed world losses", sums, "gap %.3e" % gap)
        winner = int(np.argsort(sums, kind="stable")[0])
        if gap >= BEST3_GAP and winner != 0:
            break
    assert gap >= BEST3_GAP and winner != 0, (gap, winner)
    assert abs(info["autoreg_world_loss"] - sums[winner] / 2) <= 1e-12
    out = {f"s:{k}": v for k, v in scalars(info).items()}
    out.update(gen_imgs=np.stack(info["gen_imgs"]), true_imgs=np.stack(info["true_imgs"]), world_sums=sums,
               winner=winner, gap=gap, eps_seed=seed)
    gg.save("predict_video_best3", **out)


def gen_det():
    """--model det at g 32 and --model copy, one window each (T 4)."""
    out = {}
    cfg = orc.Cfg(g_dim=32, batch_size=2, n_past=1, n_future=2, **gg.FLAGSETS["ra"])
    data = syn.synth_video(seed=63, T=4, B=2)
    for model, sd in (("det", det.make_weights(cfg, seed=7)), ("copy", None)):
        info = trainer_for(cfg, sd, model).predict_video(data)
        assert not any("kld" in k for k in info) and len(info["gen_imgs"]) == 1
        out.update({f"{model}:s:{k}": v for k, v in scalars(info).items()})
        out[f"{model}:gen_imgs"], out[f"{model}:true_imgs"] = np.stack(info["gen_imgs"]), np.stack(info["true_imgs"])
    gg.save("predict_video_det", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["ra", "best3", "det"]
    if "ra" in which:
        gen_ra()
    if "best3" in which:
        gen_best3()
    if "det" in which:
        gen_det()
