"""CPU: FusedRMSprop / FusedSGD state dicts are interchangeable with torch.optim.RMSprop / torch.optim.SGD, and
make_optimizer maps --optimizer as the reference trainer does (trainer.py:109-122)."""
import argparse
import copy

import pytest
import torch


def _ns(**kw):
    d = dict(device=torch.device("cpu"), image_width=64, image_height=64, channels=3, model_use_mask=True,
             model_use_future_mask=True, model_use_heatmap=False, model_use_future_heatmap=False,
             model_use_robot_state=True, model_use_future_robot_state=False, g_dim=32, z_dim=8, action_dim=5,
             robot_dim=5, batch_size=2, lstm_group_norm=False, last_frame_skip=True)
    d.update(kw)
    return argparse.Namespace(**d)


@pytest.fixture(scope="module")
def model():
    from robot_aware_control_amd.model import SVGConvModel
    return SVGConvModel(_ns())


def _twin_params(model):
    ps = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    for p in ps:
        p.grad = torch.full_like(p, 0.25)
    return ps


def _same_state(a, b, name):
    """The per-parameter views of flat state buffer `name` agree (the flat buffers' padding belongs to no parameter)."""
    return all(torch.equal(va[0], vb[0]) and float(va[0].flatten()[0]) != 0.0
               for (_, va), (_, vb) in zip(a._views([name]), b._views([name])))


@pytest.mark.parametrize("momentum", [0, 0.9])
def test_fused_rmsprop_state_dict_is_torch_rmsprop_compatible(model, momentum):
    from robot_aware_control_amd.optim import FusedRMSprop
    opt = FusedRMSprop(model, momentum=momentum)
    opt._buffer("square_avg").fill_(0.5)
    if momentum:
        opt._buffer("momentum_buffer").fill_(0.125)
    opt._steps = 3
    sd = opt.state_dict()
    n_params = len(list(model.parameters()))
    keys = {"step", "square_avg"} | ({"momentum_buffer"} if momentum else set())
    assert set(sd) == {"state", "param_groups"} and len(sd["state"]) == n_params
    assert set(sd["state"][0]) == keys and float(sd["state"][0]["step"]) == 3.0
    assert sd["state"][0]["step"].dtype == torch.float32
    twin_params = _twin_params(model)
    ref = torch.optim.RMSprop(twin_params)
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])  # the keys torch 2.x writes
    ref.load_state_dict(copy.deepcopy(sd))  # the reference trainer's optimizer accepts it (trainer.py:877) ...
    before = twin_params[0].detach().clone()
    ref.step()               # ... and steps from it
    assert float(ref.state[twin_params[0]]["step"]) == 4.0 and not torch.equal(before, twin_params[0])
    assert ref.param_groups[0]["momentum"] == momentum and ref.param_groups[0]["lr"] == 1e-2
    opt2 = FusedRMSprop(model, momentum=momentum)
    opt2.load_state_dict(sd)
    assert opt2._steps == 3 and _same_state(opt2, opt, "square_avg")
    assert float(opt2._buffer("square_avg")[0]) == 0.5
    if momentum:
        assert _same_state(opt2, opt, "momentum_buffer")
    else:
        assert "momentum_buffer" not in opt2._bufs  # allocated only when momentum > 0
    assert opt2.state_dict()["state"][0].keys() == sd["state"][0].keys()


def test_fused_sgd_state_dict_is_torch_sgd_compatible(model):
    from robot_aware_control_amd.optim import FusedSGD
    # without momentum: no state, whatever the step count
    opt = FusedSGD(model)
    opt._steps = 3
    sd = opt.state_dict()
    assert sd["state"] == {} and not opt._bufs
    twin_params = _twin_params(model)
    ref = torch.optim.SGD(twin_params)
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    ref.load_state_dict(copy.deepcopy(sd))  # (torch adopts the tensors it is given and steps them in place)
    before = twin_params[0].detach().clone()
    ref.step()
    torch.testing.assert_close(twin_params[0].detach(), before - 1e-3 * 0.25, rtol=0, atol=1e-9)
    opt2 = FusedSGD(model)
    opt2.load_state_dict(sd)
    assert opt2.state_dict()["state"] == {}

    # with momentum: one `momentum_buffer` per parameter, torch's only key; torch's SGD keeps no step count
    opt = FusedSGD(model, momentum=0.9)
    assert opt.state_dict()["state"] == {}  # before the first step torch has no state either
    opt._buffer("momentum_buffer").fill_(0.5)
    opt._steps = 3
    sd = opt.state_dict()
    assert len(sd["state"]) == len(list(model.parameters())) and set(sd["state"][0]) == {"momentum_buffer"}
    twin_params = _twin_params(model)
    ref = torch.optim.SGD(twin_params)
    ref.load_state_dict(copy.deepcopy(sd))  # (torch adopts the tensors it is given and steps them in place)
    before = twin_params[0].detach().clone()
    ref.step()  # buf = 0.9 * 0.5 + 0.25 = 0.7
    torch.testing.assert_close(twin_params[0].detach(), before - 1e-3 * 0.7, rtol=0, atol=1e-9)
    opt2 = FusedSGD(model)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["momentum"] == 0.9
    assert opt2._steps >= 1  # not the first step: the buffers exist
    assert _same_state(opt2, opt, "momentum_buffer")
    # a torch state whose buffers are still None: the next step is the first
    for st in sd["state"].values():
        st["momentum_buffer"] = None
    opt3 = FusedSGD(model, momentum=0.9)
    opt3.load_state_dict(sd)
    assert opt3._steps == 0


def test_unsupported_options_raise(model):
    from robot_aware_control_amd import RacError
    from robot_aware_control_amd.optim import FusedRMSprop, FusedSGD
    for cls, kw in ((FusedRMSprop, dict(weight_decay=1e-4)), (FusedRMSprop, dict(centered=True)),
                    (FusedRMSprop, dict(maximize=True)), (FusedSGD, dict(weight_decay=1e-4)),
                    (FusedSGD, dict(maximize=True)), (FusedSGD, dict(nesterov=True))):
        with pytest.raises(ValueError):
            cls(model, **kw)
    for opt in (FusedRMSprop(model), FusedSGD(model)):
        with pytest.raises(RacError):  # no CPU fallback
            opt.step()
        opt.wait_params()
        opt.wait_params(upto=10)
        p = next(model.parameters())
        opt.wait_for(p)
        assert opt.ready(p) is True


def test_make_optimizer_follows_the_reference():
    from robot_aware_control_amd.model import SVGConvModel
    from robot_aware_control_amd.optim import FusedAdam, FusedRMSprop, FusedSGD, ShardedAdam, make_optimizer
    m = SVGConvModel(_ns())
    cf = argparse.Namespace(optimizer="rmsprop", lr=1e-4, beta1=0.8)
    opt = make_optimizer(cf, m, False)
    assert type(opt) is FusedRMSprop and not isinstance(opt, FusedAdam)
    g = opt.param_groups[0]
    assert (g["lr"], g["alpha"], g["eps"], g["momentum"]) == (0.01, 0.99, 1e-8, 0)  # torch's defaults: --lr is not applied
    cf.optimizer = "sgd"
    opt = make_optimizer(cf, m, False)
    assert type(opt) is FusedSGD and not isinstance(opt, FusedAdam)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["nesterov"]) == (1e-3, 0, 0, False)
    with pytest.raises(ValueError, match="ddp_shard_optimizer.*optimizer sgd"):
        make_optimizer(cf, m, True)
    cf.optimizer = "adagrad"
    with pytest.raises(ValueError, match="Unknown optimizer"):
        make_optimizer(cf, m, False)
    cf.optimizer = "adam"
    opt = make_optimizer(cf, m, False)
    assert type(opt) is FusedAdam and not isinstance(opt, ShardedAdam)
    assert opt.param_groups[0]["lr"] == 1e-4 and opt.param_groups[0]["betas"] == (0.8, 0.999)
