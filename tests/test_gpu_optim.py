"""GPU: the fused RMSprop / SGD steps (rac_optim_step, rac_optim_ranges, ops.fused_optim_step, optim.FusedRMSprop /
FusedSGD, --optimizer rmsprop | sgd in the trainer).

Yardstick: torch.optim run in fp64 on the CPU from the same inputs.  Tolerance: the HIP result's largest element error
against that run may be at most 2x the largest error of torch's own fp32 CPU optimiser against it (the kernel does the
same handful of fp32 roundings per step, possibly in another association), with a floor of 1e-7 max |x64| for rules where
torch's fp32 error is nearly zero.  State buffers are held to the same rule, each against its own fp64 twin."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import svg_oracle as orc  # noqa: E402
from robot_aware_control_amd import synthetic as syn  # noqa: E402

RA = dict(model_use_mask=True, model_use_future_mask=True, model_use_robot_state=True, reconstruction_loss="dontcare_l1")

# name -> (torch class, its keyword arguments beyond the defaults)
RULES = {
    "rmsprop": (torch.optim.RMSprop, dict()),
    "rmsprop_momentum": (torch.optim.RMSprop, dict(momentum=0.9)),
    "sgd": (torch.optim.SGD, dict()),
    "sgd_momentum": (torch.optim.SGD, dict(momentum=0.9)),
    "sgd_nesterov": (torch.optim.SGD, dict(momentum=0.9, nesterov=True)),
    "sgd_dampening": (torch.optim.SGD, dict(momentum=0.9, dampening=0.1)),
}
N = 9220  # 2 305 float4: two full 1 024-float4 blocks and a ragged 257


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs():
    """p ~ N(0, 0.02) and five gradients whose elements cycle through the magnitudes {0, 1e-6, 1e-2, 1, 1e3} (shifted by
    one per step, so every element meets every magnitude) with random sign."""
    gen = torch.Generator().manual_seed(11)
    p = torch.randn(N, generator=gen) * 0.02
    mags = torch.tensor([0.0, 1e-6, 1e-2, 1.0, 1e3])
    grads = []
    for step in range(5):
        sign = torch.randint(0, 2, (N,), generator=gen).float() * 2 - 1
        grads.append(sign * mags[(torch.arange(N) + step) % 5])
    return p, grads


def hip_args(name, first_step):
    """(rule, state names, (lr, momentum, gain, alpha, eps), flags) of rac_optim_step for RULES[name] at torch's defaults."""
    from robot_aware_control_amd import _lib
    cls, kw = RULES[name]
    mom = kw.get("momentum", 0)
    if cls is torch.optim.RMSprop:
        return _lib.OPTIM_RMSPROP, ("square_avg", "momentum_buffer" if mom else None), (1e-2, mom, 1 - 0.99, 0.99, 1e-8), 0
    flags = (_lib.OPTIM_NESTEROV if kw.get("nesterov") else 0) | (_lib.OPTIM_FIRST_STEP if first_step else 0)
    return _lib.OPTIM_SGD, ("momentum_buffer" if mom else None, None), (1e-3, mom, 1 - kw.get("dampening", 0), 0.0, 0.0), flags


def torch_run(name, p, grads, dtype):
    """torch.optim on the CPU in `dtype`: (parameters, {state name: tensor}) after every step."""
    cls, kw = RULES[name]
    q = torch.nn.Parameter(p.to(dtype).clone())
    opt = cls([q], **kw)
    out = []
    for g in grads:
        q.grad = g.to(dtype).clone()
        opt.step()
        out.append((q.detach().clone(), {k: v.clone() for k, v in opt.state[q].items() if k != "step" and v is not None}))
    return out


def check(what, hip, t32, t64):
    """The tolerance rule of this module's docstring; the three numbers go into the message."""
    hip, t32 = hip.detach().cpu().double(), t32.detach().cpu().double()
    err_hip, err_t32 = float((hip - t64).abs().max()), float((t32 - t64).abs().max())
    floor = 1e-7 * float(t64.abs().max())
    msg = "%s: HIP error %.3e, torch fp32 error %.3e, floor %.3e" % (what, err_hip, err_t32, floor)
    print(msg)
    assert np.isfinite(err_hip) and err_hip <= max(2 * err_t32, floor), msg


@pytest.fixture(scope="module")
def torch_runs(inputs):
    p, grads = inputs
    return {name: (torch_run(name, p, grads, torch.float32), torch_run(name, p, grads, torch.float64)) for name in RULES}


@pytest.mark.parametrize("name", list(RULES))
def test_optim_step_matches_torch_fp64(dev, inputs, torch_runs, name):
    from robot_aware_control_amd import _lib
    p, grads = inputs
    r32, r64 = torch_runs[name]
    pd = p.to(dev)
    state = {}
    for step, g in enumerate(grads):
        rule, names, hyper, flags = hip_args(name, step == 0)
        s0, s1 = (None if k is None else state.setdefault(k, torch.zeros(N, device=dev)) for k in names)
        gd = g.to(dev)
        _lib.call("rac_optim_step", pd.data_ptr(), gd.data_ptr(), _lib.ptr(s0), _lib.ptr(s1), N, rule, flags, *hyper,
                  _lib.stream_ptr())
        torch.cuda.synchronize()
        check("%s step %d p" % (name, step), pd, r32[step][0], r64[step][0])
        assert set(state) == set(r64[step][1])
        for k, buf in state.items():
            check("%s step %d %s" % (name, step, k), buf, r32[step][1][k], r64[step][1][k])


def test_optim_step_tail_elements(dev, inputs, torch_runs):
    """A buffer whose length is no multiple of 4: the last elements take the same rule."""
    from robot_aware_control_amd import _lib
    p, grads = inputs
    n = 1003
    for name in ("rmsprop_momentum", "sgd_nesterov"):
        r32, r64 = torch_runs[name]  # (element-wise rules: a prefix of the buffers gives a prefix of the results)
        rule, names, hyper, flags = hip_args(name, True)
        pd, gd = p[:n].to(dev), grads[0][:n].to(dev)
        s0, s1 = (None if k is None else torch.zeros(n, device=dev) for k in names)
        _lib.call("rac_optim_step", pd.data_ptr(), gd.data_ptr(), _lib.ptr(s0), _lib.ptr(s1), n, rule, flags, *hyper,
                  _lib.stream_ptr())
        torch.cuda.synchronize()
        check("%s tail p" % name, pd, r32[0][0][:n], r64[0][0][:n])


@pytest.mark.parametrize("name", list(RULES))
def test_ranges_kernel_gives_the_same_bits_and_the_maxima(dev, inputs, name):
    """rac_optim_step over the whole buffer against rac_optim_ranges over three float4 ranges that tile it (two carry an
    amax slot, one none; one block, two blocks with a ragged second, one ragged block): equal bits in p and state, and
    every slot holds the bit pattern of max |p_new| of its range."""
    from robot_aware_control_amd import _lib
    p, grads = inputs
    ranges = [(0, 300, True), (300, 1029, False), (1329, 976, True)]
    assert sum(n4 for _, n4, _ in ranges) * 4 == N
    slots = torch.zeros(2, device=dev, dtype=torch.int32)
    table = (_lib.OptimRange * len(ranges))()
    blocks = k = 0
    for i, (b4, n4, has) in enumerate(ranges):
        table[i] = _lib.OptimRange(begin4=b4, n4=n4, block_begin=blocks, amax=slots[k:k + 1].data_ptr() if has else None)
        blocks += (n4 + 1023) // 1024
        k += has
    table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    pa, pb = p.to(dev), p.to(dev)
    sa, sb = {}, {}
    for step in range(2):
        rule, names, hyper, flags = hip_args(name, step == 0)
        gd = grads[step].to(dev)
        a0, a1 = (None if k is None else sa.setdefault(k, torch.zeros(N, device=dev)) for k in names)
        b0, b1 = (None if k is None else sb.setdefault(k, torch.zeros(N, device=dev)) for k in names)
        _lib.call("rac_optim_step", pa.data_ptr(), gd.data_ptr(), _lib.ptr(a0), _lib.ptr(a1), N, rule, flags, *hyper,
                  _lib.stream_ptr())
        slots.zero_()
        _lib.call("rac_optim_ranges", pb.data_ptr(), gd.data_ptr(), _lib.ptr(b0), _lib.ptr(b1), table_d.data_ptr(), len(ranges),
                  blocks, rule, flags, *hyper, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(pa, pb), (name, step)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (name, step, k)
        want = [pb[4 * b4:4 * (b4 + n4)].abs().max().view(torch.int32) for b4, n4, has in ranges if has]
        assert torch.equal(slots.cpu(), torch.stack(want).cpu()), (name, step, slots, want)


def ns_for(cfg, dev, **extra):
    import argparse
    d = dict(cfg.__dict__)
    d.update(device=dev, debug_cem=False, log_dir="/tmp/rac_test", img_cost_threshold=None, img_cost_world_norm=True,
             experiment="train_robonet", robot_joint_dim=5, multiview=False, load_movement_info=False,
             movement_weight=1.0, scheduled_sampling=False, scheduled_sampling_k=4000, model="svg", optimizer="adam",
             seed=0, wandb=False, cem_shard=True, ddp_bucket_mb=64, dynamics_model_ckpt=None)
    d.update(extra)
    return argparse.Namespace(**d)


def small_cfg():
    return orc.Cfg(g_dim=64, z_dim=16, batch_size=2, n_past=1, n_future=2, lr=1e-4, **RA)


@pytest.fixture(scope="module")
def weights():
    return orc.make_weights(small_cfg(), seed=1, randomize_bn_stats=False)


def make_trainer(sd, dev, optimizer, **extra):
    from robot_aware_control_amd.trainer import PredictionTrainer
    tr = PredictionTrainer(ns_for(small_cfg(), dev, optimizer=optimizer, **extra))
    tr.model.load_state_dict({k: v.clone() for k, v in sd.items()})
    tr.model.train()
    tr.model.eps_source = lambda shape: torch.zeros(shape)
    return tr


def registered_in(flat):
    """[(entry, weight)] of the split-precision weights that live in the flat parameter buffer."""
    from robot_aware_control_amd import ops
    out = []
    for ent, w in ops.registered_weights(flat.device):
        if getattr(w, "_rac_pad_source", None) is not None:
            continue
        if 0 <= w.data_ptr() - flat.data_ptr() < flat.numel() * 4:
            out.append((ent, w))
    return out


@pytest.mark.parametrize("optimizer", ["rmsprop", "sgd"])
def test_no_stale_operands_after_a_table_step(dev, weights, optimizer, monkeypatch):
    """After a step on the range-table path every registered weight's slot is its exact maximum and its fragments are what
    rac_weight_frag_split writes for the current weight -- and the model computes what a fresh model with the same
    parameters (parts from the lazy path) computes."""
    from robot_aware_control_amd import _lib, ops
    from robot_aware_control_amd.model import SVGConvModel
    tr = make_trainer(weights, dev, optimizer)
    tr._train_step(syn.synth_video(seed=20, T=3, B=2))  # registers the weights; the plain step
    names = []
    orig = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
    tr._train_step(syn.synth_video(seed=21, T=3, B=2))
    tail = names[len(names) - 1 - names[::-1].index("rac_optim_ranges"):] if "rac_optim_ranges" in names else None
    assert tail == ["rac_optim_ranges", "rac_weight_frag_split_multi"], names[-4:]  # the table path; no pass for the maxima
    monkeypatch.setattr(ops, "call", orig)
    flat, _ = tr.model.flat_parameters()
    entries = registered_in(flat)
    assert len(entries) >= 10
    for ent, w in entries:
        assert ent.current(w) and ent.exact_ok
        assert int(ent.slot) == int(w.detach().abs().max().view(torch.int32)), tuple(w.shape)
        co, ci, k, _ = w.shape
        for transposed, parts in ent.parts.items():
            ref = torch.empty_like(parts)
            _lib.call("rac_weight_frag_split", w.data_ptr(), ent.slot.data_ptr(), ref.data_ptr(), co, ci, k,
                      1 if transposed else 0, w.numel(), _lib.stream_ptr())
            assert torch.equal(parts.view(torch.int16), ref.view(torch.int16)), (tuple(w.shape), transposed)
    cfg = small_cfg()
    fresh = SVGConvModel(ns_for(cfg, dev)).to(dev)
    fresh.load_state_dict({k: v.clone() for k, v in tr.model.state_dict().items()})
    data = syn.synth_video(seed=3, T=3, B=2)
    from robot_aware_control_amd.image import zero_robot_region
    x, m, s, a = (data[k].to(dev) for k in ("images", "masks", "states", "actions"))
    outs = []
    for model in (tr.model, fresh):
        model.eval()
        model.init_hidden(2)
        with torch.no_grad():
            o = model.forward(zero_robot_region(m[0], x[0]), torch.cat([m[0], m[1]], 1), s[0], None, a[0], sample_mean=True)
        outs.append(o)
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][4], outs[1][4])


@pytest.mark.parametrize("optimizer", ["rmsprop", "sgd"])
def test_trainer_steps_match_torch_fp64(dev, weights, optimizer):
    """--optimizer rmsprop | sgd constructs and trains: each of three steps against torch.optim in fp64 applied to the
    parameters before the step with the step's flat gradient (optimiser state carried across the steps)."""
    from robot_aware_control_amd.optim import FusedRMSprop, FusedSGD
    tr = make_trainer(weights, dev, optimizer)  # (lr = 1e-4 in the config)
    cls = {"rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD}[optimizer]
    assert type(tr.optimizer) is {"rmsprop": FusedRMSprop, "sgd": FusedSGD}[optimizer]
    assert tr.optimizer.param_groups[0]["lr"] == {"rmsprop": 0.01, "sgd": 1e-3}[optimizer]  # torch's default, not --lr
    flat, grad = tr.model.flat_parameters()
    twins = {}
    for dtype in (torch.float32, torch.float64):
        q = torch.nn.Parameter(torch.zeros(flat.numel(), dtype=dtype))
        twins[dtype] = (q, cls([q]))
    for step in range(3):
        before = flat.detach().cpu().clone()
        losses = tr._train_step(syn.synth_video(seed=20 + step, T=3, B=2))
        assert all(np.isfinite(v) for v in losses.values()), losses
        g = grad.detach().cpu()
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0
        for dtype, (q, opt) in twins.items():
            with torch.no_grad():
                q.copy_(before.to(dtype))
            q.grad = g.to(dtype)
            opt.step()
        check("%s trainer step %d" % (optimizer, step), flat, twins[torch.float32][0], twins[torch.float64][0].detach())
        assert not torch.equal(flat.detach().cpu(), before)


@pytest.mark.parametrize("optimizer", ["rmsprop", "sgd"])
def test_checkpoint_resumes_bit_for_bit(dev, weights, optimizer, tmp_path):
    """_save_checkpoint after two steps, a new trainer loads it: its third step gives the bits of the original's third
    step (which takes the range-table path while the resumed trainer, its weights registered a moment ago, takes the
    plain step).  RMSprop steps with lr = 1e-4 set through `param_groups` -- which the checkpoint must carry along: at
    torch's default of 0.01 its first steps move every weight by 0.1 (no bias correction), the KL term of this model
    reaches 1e15 within two steps, and at such magnitudes the train step itself is no longer bit-reproducible (the
    BatchNorm reductions' fp64 atomics then depend on their order), whatever the optimiser path."""
    tr = make_trainer(weights, dev, optimizer, log_dir=str(tmp_path))
    if optimizer == "rmsprop":
        tr.optimizer.param_groups[0]["lr"] = 1e-4
    for step in range(2):
        tr._train_step(syn.synth_video(seed=20 + step, T=3, B=2))
    tr._step = 2
    path = tr._save_checkpoint()
    state = torch.load(path, map_location="cpu")["optimizer"]["state"]
    if optimizer == "rmsprop":
        assert set(state[0]) == {"step", "square_avg"} and float(state[0]["step"]) == 2.0
    else:
        assert state == {}  # torch.optim.SGD without momentum keeps no state
    tr2 = make_trainer(weights, dev, optimizer, log_dir=str(tmp_path))
    assert tr2._load_checkpoint(None) == 2
    assert tr2.optimizer.param_groups[0]["lr"] == tr.optimizer.param_groups[0]["lr"]
    tr2.model.train()
    data = syn.synth_video(seed=22, T=3, B=2)
    l1 = tr._train_step(data)
    l2 = tr2._train_step(data)
    assert l1 == l2 and all(np.isfinite(v) for v in l1.values()), (l1, l2)
    assert torch.equal(tr.model.flat_parameters()[1], tr2.model.flat_parameters()[1])  # the gradients, then the update
    assert torch.equal(tr.model.flat_parameters()[0], tr2.model.flat_parameters()[0])
    if optimizer == "rmsprop":
        assert torch.equal(tr.optimizer._buffer("square_avg"), tr2.optimizer._buffer("square_avg"))
        assert tr.optimizer._steps == tr2.optimizer._steps == 3
