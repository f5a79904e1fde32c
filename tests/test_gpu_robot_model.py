"""GPU: the learned robot model (`--learned_robot_model`) -- the rac_mlp4_* / rac_robot_rollout / rac_mse_rows kernels through
the C ABI, both trainers against the reference's golden numbers, and PredictionTrainer under finetune_widowx.

Arithmetic is compared with tests/fp64_tools.Rule: e_gpu <= max(2e-6, 4 * e_cpu32) against the fp64 oracle
(tests/robot_model_oracle.py), e_cpu32 being the same formula in fp32 on the CPU -- or, for the golden numbers, the
golden file's own error against the fp64 oracle.  Determinism and row independence are compared with torch.equal."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import svg_oracle as orc  # noqa: E402
from robot_aware_control_amd import synthetic as syn  # noqa: E402
from tests import predict_video_oracle as pvo  # noqa: E402
from tests import robot_model_oracle as rmo  # noqa: E402
from tests.fp64_tools import Rule, rnd  # noqa: E402

DIMS = [(7, 5), (5, 2), (6, 4)]
C = rmo.GOLDEN


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ shared inputs and CPU references
def flat_of(sd):
    return torch.cat([sd[k].reshape(-1) for k in rmo.KEYS])


@functools.lru_cache(maxsize=None)
def problem(D, A, M=70):
    """Weights, M input rows and the CPU references (fp64, fp32) of one (D, A): every test slices the rows it needs."""
    sd = rmo.make_weights(f"k{D}{A}", D, A, seed=3)
    x, a, dy = rnd(100 + D, M, D, scale=0.5), rnd(200 + A, M, A, scale=0.1), rnd(300 + D, M, D)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        m = rmo.build(sd, dtype)
        seq, h, acts = m.predictor, torch.cat([x, a], 1).to(dtype), []
        with torch.no_grad():
            for i, layer in enumerate(seq):
                h = layer(h)
                if i in (1, 3, 5):
                    acts.append(h)
        ref[dtype] = (h, torch.stack(acts))
    return sd, x, a, dy, ref


def cpu_grads(sd, x, a, dy, dtype):
    m = rmo.build(sd, dtype)
    (m(x.to(dtype), a.to(dtype)) * dy.to(dtype)).sum().backward()
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()])


def abi_fwd(dev, params, x, a, residual, save):
    from robot_aware_control_amd import _lib
    M, D = x.shape
    y = torch.full((M, D), float("nan"), device=dev)
    acts = torch.full((3, M, 512), float("nan"), device=dev) if save else None
    _lib.call("rac_mlp4_fwd", params.data_ptr(), x.data_ptr(), a.data_ptr(), y.data_ptr(), _lib.ptr(acts), M, D,
              a.shape[1], int(residual), _lib.stream_ptr())
    return y, acts


def abi_bwd(dev, params, x, a, acts, dy, grads, accumulate):
    from robot_aware_control_amd import _lib
    M, D = x.shape
    dz = torch.empty((3, M, 512), device=dev)
    _lib.call("rac_mlp4_bwd", params.data_ptr(), x.data_ptr(), a.data_ptr(), acts.data_ptr(), dy.data_ptr(),
              dz.data_ptr(), grads.data_ptr(), M, D, a.shape[1], int(accumulate), _lib.stream_ptr())
    return grads


def abi_rollout(dev, jp, gp, q0, s0, actions):
    from robot_aware_control_amd import _lib
    T, N, A = actions.shape
    q = torch.full((T + 1, N, q0.shape[1]), float("nan"), device=dev) if jp is not None else None
    s = torch.full((T + 1, N, s0.shape[1]), float("nan"), device=dev) if gp is not None else None
    _lib.call("rac_robot_rollout", _lib.ptr(jp), _lib.ptr(gp), _lib.ptr(q0 if jp is not None else None),
              _lib.ptr(s0 if gp is not None else None), actions.data_ptr(), _lib.ptr(q), _lib.ptr(s), T, N,
              q0.shape[1] if jp is not None else 0, s0.shape[1] if gp is not None else 0, A, _lib.stream_ptr())
    return q, s


# ------------------------------------------------------------------ rac_mlp4_fwd
@pytest.mark.parametrize("D,A", DIMS)
@pytest.mark.parametrize("M", [1, 31, 32, 33, 70])
def test_mlp4_fwd_vs_fp64(dev, M, D, A):
    from robot_aware_control_amd import _lib
    sd, x, a, _, ref = problem(D, A)
    assert _lib.load().rac_mlp4_param_count(D, A) == flat_of(sd).numel()
    params, xg, ag = flat_of(sd).to(dev), x[:M].contiguous().to(dev), a[:M].contiguous().to(dev)
    rule = Rule(f"mlp4_fwd M{M} D{D} A{A}")
    outs = {}
    for residual in (0, 1):
        for save in (False, True):
            y, acts = abi_fwd(dev, params, xg, ag, residual, save)
            outs[residual, save] = y
            r64, r32 = (ref[t][0][:M] + (x[:M].to(t) if residual else 0) for t in (torch.float64, torch.float32))
            rule.check(f"y residual={residual} save={save}", y, r64, r32)
            if save:
                rule.check(f"acts residual={residual}", acts, ref[torch.float64][1][:, :M], ref[torch.float32][1][:, :M])
        assert torch.equal(outs[residual, False], outs[residual, True])  # saving the activations changes nothing
    rule.done()


# ------------------------------------------------------------------ rac_mlp4_bwd
@pytest.mark.parametrize("D,A", DIMS)
@pytest.mark.parametrize("M", [1, 33, 70])
def test_mlp4_bwd_vs_fp64_autograd(dev, M, D, A):
    sd, x, a, dy, _ = problem(D, A)
    x, a, dy = x[:M].contiguous(), a[:M].contiguous(), dy[:M].contiguous()
    g64, g32 = cpu_grads(sd, x, a, dy, torch.float64), cpu_grads(sd, x, a, dy, torch.float32)
    params, xg, ag, dyg = flat_of(sd).to(dev), x.to(dev), a.to(dev), dy.to(dev)
    _, acts = abi_fwd(dev, params, xg, ag, 0, True)
    n = params.numel()
    over = abi_bwd(dev, params, xg, ag, acts, dyg, torch.full((n,), float("nan"), device=dev), accumulate=0)
    rule = Rule(f"mlp4_bwd M{M} D{D} A{A}")
    off = 0
    for k in rmo.KEYS:
        cnt = sd[k].numel()
        rule.check(k, over[off:off + cnt], g64[off:off + cnt], g32[off:off + cnt])
        off += cnt
    rule.done()
    again = abi_bwd(dev, params, xg, ag, acts, dyg, torch.zeros(n, device=dev), accumulate=0)
    assert torch.equal(over, again)  # two runs: the same bits
    base = rnd(9, n).to(dev)
    acc = abi_bwd(dev, params, xg, ag, acts, dyg, base.clone(), accumulate=1)
    assert torch.equal(acc, base + over)  # accumulate = the overwrite result added once


# ------------------------------------------------------------------ rac_robot_rollout
@functools.lru_cache(maxsize=None)
def rollout_problem(T, N):
    J, R, A = 7, 5, 5
    jsd, gsd = rmo.make_weights("rj", J, A, seed=5), rmo.make_weights("rg", R, A, seed=5)
    q0, s0, ac = rnd(1, N, J, scale=0.5), rnd(2, N, R, scale=0.5), rnd(3, T, N, A, scale=0.1)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        ref[dtype] = rmo.rollout(rmo.build(jsd, dtype), rmo.build(gsd, dtype), q0.to(dtype), s0.to(dtype), ac.to(dtype))
    return jsd, gsd, q0, s0, ac, ref


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("N", [1, 33, 70])
def test_rollout_vs_fp64_and_chained_forward(dev, T, N):
    jsd, gsd, q0, s0, ac, ref = rollout_problem(T, N)
    jp, gp = flat_of(jsd).to(dev), flat_of(gsd).to(dev)
    q0g, s0g, acg = q0.to(dev), s0.to(dev), ac.to(dev)
    q, s = abi_rollout(dev, jp, gp, q0g, s0g, acg)
    rule = Rule(f"rollout T{T} N{N}")
    rule.check("qpos", q, ref[torch.float64][0], ref[torch.float32][0])
    rule.check("states", s, ref[torch.float64][1], ref[torch.float32][1])
    rule.done()
    assert torch.equal(q[0], q0g) and torch.equal(s[0], s0g)
    for t in range(T):  # step t + 1 = rac_mlp4_fwd(residual) on the rollout's own step t, to the bit
        assert torch.equal(q[t + 1], abi_fwd(dev, jp, q[t].contiguous(), acg[t].contiguous(), 1, False)[0])
        assert torch.equal(s[t + 1], abi_fwd(dev, gp, s[t].contiguous(), acg[t].contiguous(), 1, False)[0])
    # either model absent: the other's result is unchanged
    q_only, none = abi_rollout(dev, jp, None, q0g, s0g, acg)
    assert none is None and torch.equal(q_only, q)
    none, s_only = abi_rollout(dev, None, gp, q0g, s0g, acg)
    assert none is None and torch.equal(s_only, s)


def test_rollout_rows_do_not_depend_on_their_batch(dev):
    T, N = 3, 70
    jsd, gsd, q0, s0, ac, _ = rollout_problem(T, N)
    jp, gp = flat_of(jsd).to(dev), flat_of(gsd).to(dev)
    q0g, s0g, acg = q0.to(dev), s0.to(dev), ac.to(dev)
    q, s = abi_rollout(dev, jp, gp, q0g, s0g, acg)
    cut = lambda lo, hi: abi_rollout(dev, jp, gp, q0g[lo:hi].contiguous(), s0g[lo:hi].contiguous(),
                                     acg[:, lo:hi].contiguous())
    for spans in ([(0, 33), (33, 70)], [(i, i + 1) for i in range(N)]):
        parts = [cut(lo, hi) for lo, hi in spans]
        assert torch.equal(torch.cat([p[0] for p in parts], 1), q)
        assert torch.equal(torch.cat([p[1] for p in parts], 1), s)


def test_module_forward_and_autograd_match_the_kernels(dev):
    """nn.Module.forward returns the delta through ops.Mlp4; loss.backward() through ops.MseRows fills the gradient block
    with what rac_mlp4_bwd gives for the same dy; inputs that require grad are refused."""
    from robot_aware_control_amd import ops
    from robot_aware_control_amd.robot_model import JointPosPredictor
    D, A, M = 7, 5, 33
    sd, x, a, _, ref = problem(D, A)
    m = JointPosPredictor(argparse.Namespace(robot_joint_dim=D, action_dim=A)).to(dev)
    m.load_state_dict(sd)
    xg, ag, target = x[:M].to(dev), a[:M].to(dev), rnd(5, M, D).to(dev)
    params, grads = m.flat_parameters()
    assert torch.equal(params.cpu(), flat_of(sd))
    m.zero_grad()
    delta = m(xg, ag)
    assert torch.equal(delta, abi_fwd(dev, params, xg, ag, 0, False)[0])
    loss = ops.MseRows.apply(delta + xg, target)
    loss.sum().backward()
    _, acts = abi_fwd(dev, params, xg, ag, 0, True)
    _, dy = ops.mse_rows(delta + xg, target, 1.0 / (M * D), want_grad=True)
    want = abi_bwd(dev, params, xg, ag, acts, dy, torch.zeros_like(params), accumulate=0)
    assert torch.equal(m.flat_parameters()[1], want) and float(want.abs().max()) > 0
    assert m.predictor[2].weight.grad.data_ptr() == m.flat_parameters()[1].data_ptr() + 4 * 512 * (D + A + 1)
    rule = Rule("MseRows")
    r = lambda t: rmo.mse((ref[t][0][:M] + x[:M].to(t)), target.cpu().to(t))
    rule.check("loss", loss[0], r(torch.float64), r(torch.float32))
    rule.done()
    with pytest.raises(ValueError, match="require grad"):
        m(xg.clone().requires_grad_(True), ag)


# ------------------------------------------------------------------ RobotPredictionTrainer
def robot_cf(dev, tmp, **kw):
    d = dict(robot_joint_dim=C["J"], robot_dim=C["R"], action_dim=C["A"], n_past=C["n_past"], n_future=C["n_future"],
             n_eval=C["n_eval"], optimizer="adam", lr=C["lr"], beta1=C["beta1"], experiment="finetune_widowx",
             log_dir=str(tmp), scheduled_sampling=False, wandb=False, dynamics_model_ckpt=None, niter=1, epoch_size=2,
             checkpoint_interval=1, eval_interval=1, device=dev)
    d.update(kw)
    return argparse.Namespace(**d)


def robot_trainer(dev, tmp, fk=None, **kw):
    from robot_aware_control_amd.robot_trainer import RobotPredictionTrainer
    tr = RobotPredictionTrainer(robot_cf(dev, tmp, **kw), forward_kinematics=fk)
    tr.joint_model.load_state_dict(rmo.make_weights("joint", C["J"], C["A"], C["seed"]))
    tr.gripper_model.load_state_dict(rmo.make_weights("gripper", C["R"], C["A"], C["seed"]))
    return tr


def test_robot_trainer_vs_reference_golden(dev, golden_dir, tmp_path):
    """Two Adam train steps, the weight slices behind them and both eval dicts against tests/golden/robot_model.npz: the
    GPU's error against the fp64 oracle is at most 4 x the golden's (fp32 on the CPU) own error against it."""
    g = np.load(os.path.join(golden_dir, "robot_model.npz"))
    r64 = rmo.golden_recipe(g, torch.float64)
    data = rmo.golden_inputs(g)
    tr = robot_trainer(dev, tmp_path, fk=rmo.fake_fk)
    got = {}
    q, s = tr_rollout(tr, data)
    got["rollout_qpos"], got["rollout_states"] = q, s
    got["delta_joint"] = tr.joint_model(data["qpos"][0].to(dev), data["actions"][0].to(dev))
    got["delta_gripper"] = tr.gripper_model(data["states"][0].to(dev), data["actions"][0].to(dev))
    for step in (1, 2):
        losses = tr._train_step(data)
        assert set(losses) == {"joint_loss", "joint_mse", "gripper_loss"}
        for k, v in losses.items():
            got[f"train{step}_{k}"] = torch.tensor(v, dtype=torch.float64)
    sds = {"joint": tr.joint_model.state_dict(), "gripper": tr.gripper_model.state_dict()}
    for key in g.files:
        if key.startswith("after_"):
            which, name = key[len("after_"):].split("_", 1)
            got[key] = sds[which][name][tuple(slice(0, n) for n in g[key].shape)]
    for ar in (False, True):
        for k, v in tr._eval_step(data, autoregressive=ar).items():
            got[f"eval_{k}"] = torch.tensor(v, dtype=torch.float64)
    keys = [k for k in g.files if not k.startswith("in_") and k != "source"]
    assert set(got) == set(keys)
    rule = Rule("robot trainer vs golden")
    for k in keys:
        rule.check(k, got[k], r64[k], torch.from_numpy(np.asarray(g[k])))
    rule.done()
    # without a forward-kinematics callable the end-effector key is omitted, the others are unchanged
    tr.forward_kinematics = None
    plain = tr._eval_step(data, autoregressive=True)
    assert set(plain) == {"autoreg_joint_loss", "autoreg_joint_mse", "autoreg_gripper_loss"}
    assert plain["autoreg_gripper_loss"] == float(got["eval_autoreg_gripper_loss"])


def tr_rollout(tr, data):
    from robot_aware_control_amd.robot_model import LearnedRobotModel
    return LearnedRobotModel(tr._config, tr.joint_model, tr.gripper_model).rollout(data["qpos"][0], data["states"][0],
                                                                                   data["actions"])


def test_robot_trainer_step_is_reproducible_and_videos_average(dev, golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "robot_model.npz"))
    data = rmo.golden_inputs(g)
    flats = []
    for _ in range(2):
        tr = robot_trainer(dev, tmp_path)
        first = tr._train_step(data)
        flats.append(tr.models.flat_parameters()[0].clone())
    assert torch.equal(flats[0], flats[1])
    # _train_video / _eval_video: a video of two windows is the mean of its windows' steps
    video = {k: (torch.cat([v, v]) if torch.is_tensor(v) else v) for k, v in data.items()}
    video["actions"] = torch.cat([data["actions"], data["actions"][:1], data["actions"]])
    tr = robot_trainer(dev, tmp_path)
    both = tr._train_video(video)
    tr2 = robot_trainer(dev, tmp_path)
    one, two = tr2._train_step(data), tr2._train_step(data)
    assert one == first
    for k in one:
        assert both[k] == one[k] / 2 + two[k] / 2
    ev = tr._eval_video(video, autoregressive=True)
    assert ev == {k: (v + v) / 2 for k, v in tr._eval_step(data, autoregressive=True).items()}
    # T = 0: the starts, no launch
    q, s = tr_rollout(tr, dict(data, actions=data["actions"][:0]))
    assert q.shape == (1, C["B"], C["J"]) and torch.equal(q[0].cpu(), data["qpos"][0]) and torch.equal(s[0].cpu(), data["states"][0])


def test_robot_trainer_train_loop_checkpoints_and_resumes(dev, golden_dir, tmp_path):
    """train() with an injected batch generator and test loader: step count, epoch metrics of both eval forms, the
    checkpoint cadence, and a second trainer resuming from the newest checkpoint of the log directory."""
    g = np.load(os.path.join(golden_dir, "robot_model.npz"))
    data = rmo.golden_inputs(g)

    def batches():
        while True:
            yield data
    loader = [{k: (v.transpose(0, 1).contiguous() if torch.is_tensor(v) else v) for k, v in data.items()}]  # batch-first
    tr = robot_trainer(dev, tmp_path, niter=2, epoch_size=2, experiment="train_robot_model")
    info = tr.train(batches(), loader)
    assert tr._step == 4 and set(info) == {"joint_loss", "joint_mse", "gripper_loss"}
    assert [e for e, _ in tr.eval_history] == [0, 1]
    last = tr.eval_history[-1][1]
    assert set(last) == {f"test/{p}_{k}" for p in ("1step", "autoreg") for k in ("joint_loss", "joint_mse", "gripper_loss")}
    assert last["test/autoreg_joint_loss"] == tr._eval_video(data, autoregressive=True)["autoreg_joint_loss"]
    assert last["test/1step_gripper_loss"] == tr._eval_video(data)["1step_gripper_loss"]
    assert last["test/1step_joint_loss"] < tr.eval_history[0][1]["test/1step_joint_loss"]  # it trains
    assert sorted(os.listdir(tmp_path)) == ["ckpt_4.pt"]  # epoch 1: checkpoint_interval 1, epoch > 0
    again = robot_trainer(dev, tmp_path, niter=1, epoch_size=1, experiment="train_robot_model")
    assert again._load_checkpoint(None) == 4 and again.optimizer._steps == 4
    assert torch.equal(again.models.flat_parameters()[0], tr.models.flat_parameters()[0])
    assert torch.equal(again.optimizer._moments()[1], tr.optimizer._moments()[1])
    assert again._train_step(data) == tr._train_step(data)  # the same next step, to the bit


@pytest.mark.parametrize("name", ["rmsprop", "sgd"])
def test_robot_trainer_other_optimizers_vs_torch(dev, golden_dir, tmp_path, name):
    """One step of --optimizer rmsprop / sgd (torch's defaults, as the reference builds them) against torch.optim on the
    oracle models.  SGD's update is linear in the gradient: every parameter is compared.  RMSprop's first step is
    lr g / (sqrt(0.01 g^2) + eps) = 0.1 sign(g), a jump at g = 0: among half a million weights some gradient lies within
    fp32 rounding of zero and lands on the other side, in any fp32 evaluation (the whole last-layer weight of the gripper
    model shows it: 5e-5 on the GPU, 1e-4 in fp32 on the CPU), so the golden file's weight slices and the two output
    biases (a few hundred elements, none of them near zero) are compared instead."""
    g = np.load(os.path.join(golden_dir, "robot_model.npz"))
    data = rmo.golden_inputs(g)
    tr = robot_trainer(dev, tmp_path, optimizer=name)
    got_losses = tr._train_step(data)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        joint = rmo.build(rmo.make_weights("joint", C["J"], C["A"], C["seed"]), dtype)
        gripper = rmo.build(rmo.make_weights("gripper", C["R"], C["A"], C["seed"]), dtype)
        params = list(joint.parameters()) + list(gripper.parameters())
        opt = torch.optim.RMSprop(params) if name == "rmsprop" else torch.optim.SGD(params)
        losses = rmo.train_step(joint, gripper, opt, rmo.cast(data, dtype), C["n_past"], C["n_future"])
        refs[dtype] = (losses, {"joint": joint.state_dict(), "gripper": gripper.state_dict()})
    rule = Rule(f"robot trainer {name}")
    for k, v in got_losses.items():
        rule.check(k, torch.tensor(v, dtype=torch.float64), *(torch.tensor(refs[t][0][k], dtype=torch.float64)
                                                               for t in (torch.float64, torch.float32)))
    sds = {"joint": tr.joint_model.state_dict(), "gripper": tr.gripper_model.state_dict()}
    moved = 0.0
    for which in ("joint", "gripper"):
        for key in rmo.KEYS:
            if name == "sgd":
                sl = (slice(None),)
            elif f"after_{which}_{key}" in g.files:
                sl = tuple(slice(0, n) for n in g[f"after_{which}_{key}"].shape)
            elif key == "predictor.6.bias":
                sl = (slice(None),)
            else:
                continue
            got = sds[which][key][sl]
            rule.check(f"{which}.{key}", got, refs[torch.float64][1][which][key][sl], refs[torch.float32][1][which][key][sl])
            start = rmo.make_weights(which, C["J" if which == "joint" else "R"], C["A"], C["seed"])[key][sl]
            moved = max(moved, float((got.cpu() - start).abs().max()))
    rule.done()
    assert moved > 1e-5  # the step was taken


# ------------------------------------------------------------------ PredictionTrainer under finetune_widowx
def ns_for(cfg, dev, **extra):
    d = dict(cfg.__dict__)
    d.update(device=dev, debug_cem=False, log_dir="/tmp/rac_test_robot_model", img_cost_threshold=None,
             img_cost_world_norm=True, experiment="finetune_widowx", robot_joint_dim=5, multiview=False,
             load_movement_info=False, movement_weight=1.0, scheduled_sampling=False, scheduled_sampling_k=4000,
             model="svg", optimizer="adam", seed=0, wandb=False, cem_shard=True, ddp_bucket_mb=64,
             dynamics_model_ckpt=None, n_eval=4, test_batch_size=2, preprocess_action="raw", random_snippet=False)
    d.update(extra)
    return argparse.Namespace(**d)


def resized(m, h, w):
    """The reference's ToTensor + Resize((h, w)) + bool of one render (robot_model_oracle.img_transform)."""
    return (rmo.img_transform(h, w)(m)[0] != 0).numpy()


def test_predict_batch_resizes_renders_to_the_frames(dev):
    """48 x 64 frames (the default image shape) with renderers of the real mask envs' 64 x 85: every predicted mask is
    the render of the rollout's own joint position, resized as trainer.py:87-88 does; states against the fp64 oracle's
    step-by-step `_generate_learned_robot_states`."""
    from robot_aware_control_amd.robot_model import GripperStatePredictor, JointPosPredictor, LearnedRobotModel
    J, R, A, T, B, H, W = 7, 5, 5, 3, 3, 48, 64
    cf = argparse.Namespace(robot_joint_dim=J, robot_dim=R, action_dim=A, image_height=H, image_width=W,
                            experiment="finetune_widowx", preprocess_action="raw", model_use_heatmap=False)
    jsd, gsd = rmo.make_weights("joint", J, A, 31), rmo.make_weights("gripper", R, A, 31)
    joint, gripper = JointPosPredictor(cf).to(dev), GripperStatePredictor(cf).to(dev)
    joint.load_state_dict(jsd)
    gripper.load_state_dict(gsd)
    make = lambda: {"cam0": rmo.RectRenderer(0, H=64, W=85), "cam1": rmo.RectRenderer(1, H=64, W=85)}
    model = LearnedRobotModel(cf, joint, gripper, renderers=make())
    data = rmo.synth_window(13, T + 1, B, J, R, A)
    data["masks"] = (rnd(14, T + 1, B, 1, H, W) > 0.8).float()
    data["folder"] = ["cam1", "cam0", "cam1"]
    states, masks = model.predict_batch(data)
    q, s = model.rollout(data["qpos"][0], data["states"][0], data["actions"])
    assert masks.shape == (T + 1, B, 1, H, W) and masks.dtype == torch.float32
    assert torch.equal(states, s) and torch.equal(masks[0].cpu(), data["masks"][0])
    fresh, seen = make(), set()
    for t in range(1, T + 1):
        for b, vp in enumerate(data["folder"]):
            want = resized(fresh[vp].generate_masks([q[t, b].cpu().numpy()])[0], H, W)
            assert want.shape == (H, W) and want.any()
            assert np.array_equal(masks[t, b, 0].cpu().numpy() != 0, want), (t, b)
            seen.add(want.tobytes())
    assert len(seen) == T * B
    rule = Rule("predict_batch states")
    refs = [rmo.generate_learned_robot_states(rmo.build(jsd, t), rmo.build(gsd, t), rmo.cast(data, t), make(),
                                              rmo.img_transform(H, W))[0] for t in (torch.float64, torch.float32)]
    rule.check("states", states, *refs)
    rule.done()
    # a batch whose masks are not image_height x image_width is refused
    with pytest.raises(ValueError, match="48 x 64"):
        model.predict_batch(dict(data, masks=torch.zeros(T + 1, B, 1, 64, 64)))


def test_prediction_trainer_with_the_learned_robot_model(dev, tmp_path, monkeypatch):
    from robot_aware_control_amd.robot_trainer import RobotPredictionTrainer
    from robot_aware_control_amd.trainer import PredictionTrainer
    cfg = orc.Cfg(g_dim=64, z_dim=16, batch_size=2, n_past=1, n_future=2, **pvo.RA_FLAGS)
    # the checkpoint a RobotPredictionTrainer writes is the one --robot_model_ckpt loads
    rt = RobotPredictionTrainer(robot_cf(dev, tmp_path, robot_joint_dim=5, robot_dim=5, action_dim=5))
    rt.joint_model.load_state_dict(rmo.make_weights("joint", 5, 5, 21))
    rt.gripper_model.load_state_dict(rmo.make_weights("gripper", 5, 5, 21))
    rt._step = 3
    ckpt = rt._save_checkpoint()
    with pytest.raises(ValueError, match="robot_model_ckpt"):
        PredictionTrainer(ns_for(cfg, dev, learned_robot_model=True, robot_model_ckpt=None))
    sd = orc.make_weights(cfg, seed=11)

    def trainer():
        tr = PredictionTrainer(ns_for(cfg, dev, learned_robot_model=True, robot_model_ckpt=ckpt))
        tr.model.load_state_dict({k: v.clone() for k, v in sd.items()})
        tr.robot_model.renderers = {"cam0": rmo.RectRenderer(0), "cam1": rmo.RectRenderer(1)}
        return tr
    tr = trainer()
    for mine, theirs in ((tr.joint_model, rt.joint_model), (tr.gripper_model, rt.gripper_model)):
        for k, v in theirs.state_dict().items():
            assert torch.equal(mine.state_dict()[k], v), k
    assert tr.robot_model.joint_model is tr.joint_model and tr.robot_model.gripper_model is tr.gripper_model
    data = syn.synth_video(seed=71, T=4, B=2)
    data["folder"] = ["cam0", "cam1"]
    data["low"], data["high"] = torch.zeros(2, 5), torch.ones(2, 5)
    window = {k: (v[:3] if torch.is_tensor(v) and k not in ("low", "high") else v) for k, v in data.items()}
    window["actions"] = data["actions"][:2]
    # predict_batch: row 0 the ground truth, states the rollout, one render per predicted qpos from its sample's viewpoint
    states, masks = tr.robot_model.predict_batch(window)
    q, s = tr.robot_model.rollout(window["qpos"][0], window["states"][0], window["actions"])
    assert states.shape == window["states"].shape and masks.shape == window["masks"].shape
    assert torch.equal(states[0].cpu(), window["states"][0]) and torch.equal(masks[0].cpu(), window["masks"][0])
    assert torch.equal(states, s)
    fresh = {"cam0": rmo.RectRenderer(0), "cam1": rmo.RectRenderer(1)}
    seen = set()
    for t in (1, 2):
        for b, vp in enumerate(window["folder"]):
            want = resized(fresh[vp].generate_masks([q[t, b].cpu().numpy()])[0], 64, 64)  # 48 x 64 renders
            assert np.array_equal(masks[t, b, 0].cpu().numpy() != 0, want), (t, b)
            seen.add(want.tobytes())
    assert len(seen) == 4  # four different masks: a wrong row or viewpoint would show
    assert sum(len(r.calls) for r in tr.robot_model.renderers.values()) == 4
    # _train_video = _train_step on the batch with those states and masks substituted by hand, to the bit
    def feed(t, seed):  # the model's N(0, 1) draws from a seeded CPU generator: the same for both trainers
        gen = torch.Generator().manual_seed(seed)
        t.model.eps_source = lambda shape: torch.randn(shape, generator=gen)
    tr.model.train()
    feed(tr, 40)
    via_video = dict(tr._train_video(window))
    tr2 = trainer()
    tr2.model.train()
    feed(tr2, 40)
    by_hand = dict(window, states=states, masks=masks)
    assert via_video == tr2._train_step(by_hand)

    # _eval_video and predict_video roll out on the model's pred_masks, the true masks score
    tr.model.eval()
    handed, seen_batches = [], []
    inner_predict, inner_eval = tr.robot_model.predict_batch, tr._eval_step
    monkeypatch.setattr(tr.robot_model, "predict_batch", lambda b: handed.append(inner_predict(b)) or handed[-1])
    monkeypatch.setattr(tr, "_eval_step", lambda b, ar=False: seen_batches.append(b) or inner_eval(b, ar))
    feed(tr, 41)
    out = tr._eval_video(data, autoregressive=True)
    assert len(handed) == 1 and seen_batches[0]["pred_masks"] is handed[0][1] and seen_batches[0]["states"] is handed[0][0]
    assert torch.equal(seen_batches[0]["masks"], data["masks"]) and not torch.equal(handed[0][1].cpu(), data["masks"])
    assert out and all(np.isfinite(v) for v in out.values())
    monkeypatch.setattr(tr, "_eval_step", inner_eval)
    feed(tr, 42)
    pv = tr.predict_video(data)
    assert len(handed) >= 2 and np.stack(pv["gen_imgs"]).dtype == np.uint8
