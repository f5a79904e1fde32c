"""The deferred weight-gradient window (`ops.deferred_wgrad()`, ops._WgradWindow) on its own: early flushes by count and by
hand, `on_ready`, bias records, `wgrad_on_side_stream`, nesting, the late-record and the one-stream errors.

Two 3x3 weights (Cout 64 and 128) over B = 2, 8x8, 64-channel maps, three recorded steps with output gradients gy, 2 gy, gy:
the sum is 4 x the one-step gradient.  Bit-equality is asserted where both sides make the same single launch over the same
records in the same order; against fp64 the bound is test_wgrad_split_precision's (< 3e-6), and for the bias column sums
test_gpu_reduce's rule for rac_colsum_steps (e_gpu <= max(2e-6, 4 e_cpu32))."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.fp64_tools import Rule  # noqa: E402
from tests.test_gpu_ops import cl_weight, relerr, rnd, to_map  # noqa: E402

B, H, W, C0 = 2, 8, 8, 64
COUTS = (64, 128)
STEPS = (1.0, 2.0, 1.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def data(dev):
    """x, and per Cout the weight, gy and the fp64 one-step gradient (computed once, read only)."""
    x = rnd(1, B, C0, H, W)
    out = {"x0": to_map(x, dev)}
    for co in COUTS:
        w = (rnd(2 + co, co, C0, 3, 3) * 0.02).requires_grad_(True)
        gy = rnd(4 + co, B, co, H, W) * 1e-4
        F.conv2d(x.double(), w.double(), None, 1, 1).backward(gy.double())
        out[co] = {"w": w.detach(), "gy": gy, "ref": w.grad.double()}
    return out


def fresh(data, dev, co):
    return cl_weight(data[co]["w"]).to(dev).requires_grad_(True)


def record(ops, data, dev, wd, scale=1.0):
    co = wd.shape[0]
    ops.conv_wgrad_split_acc(to_map(scale * data[co]["gy"], dev), data["x0"], None, wd, defer=True)


def untouched(wd):
    return wd.grad is None or float(wd.grad.abs().max()) == 0.0


def test_flush_after_count_launches_inside_the_window_same_bits(dev, data):
    """flush_after=3 against no early flush: the same one launch per weight, on the side stream the moment the third record
    lands -- the gradient is there once the side stream is synchronised INSIDE the context."""
    from robot_aware_control_amd import ops
    base = [fresh(data, dev, co) for co in COUTS]
    with ops.deferred_wgrad():
        for s in STEPS:
            for wd in base:
                record(ops, data, dev, wd, s)
        assert all(untouched(wd) for wd in base)
    for wd in base:
        assert relerr(wd.grad.cpu(), 4 * data[wd.shape[0]]["ref"]) < 3e-6
    early = [fresh(data, dev, co) for co in COUTS]
    with ops.deferred_wgrad(flush_after=3):
        for s in STEPS:
            for wd in early:
                record(ops, data, dev, wd, s)
        assert not ops._WINDOW.weights
        ops._side_stream("wgrad", dev).synchronize()
        inside = [wd.grad.clone() for wd in early]
    for b, i, e in zip(base, inside, early):
        assert torch.equal(i, b.grad) and torch.equal(e.grad, b.grad)


def test_on_ready_at_exit_once_per_weight_largest_first(dev, data):
    from robot_aware_control_amd import ops
    w64, w128 = (fresh(data, dev, co) for co in COUTS)
    calls = []
    with ops.deferred_wgrad(on_ready=calls.append):
        for s in STEPS:
            record(ops, data, dev, w64, s)
            record(ops, data, dev, w128, s)
        assert calls == []
    assert len(calls) == 2 and calls[0] is w128 and calls[1] is w64
    for wd in (w64, w128):
        assert relerr(wd.grad.cpu(), 4 * data[wd.shape[0]]["ref"]) < 3e-6


def test_on_ready_with_flush_after_and_the_late_record_error(dev, data):
    """`on_ready` fires when the weight's third record lands; a fourth raises, the exception leaves no window behind, and the
    next window (and a deferred call outside any window) works."""
    from robot_aware_control_amd import _lib, ops
    w64 = fresh(data, dev, 64)
    calls = []
    with pytest.raises(_lib.RacError, match="recorded after"):
        with ops.deferred_wgrad(on_ready=calls.append, flush_after=3):
            record(ops, data, dev, w64)
            record(ops, data, dev, w64, 2.0)
            assert calls == []
            record(ops, data, dev, w64)
            assert len(calls) == 1 and calls[0] is w64
            record(ops, data, dev, w64)
    assert ops._WINDOW is None
    assert relerr(w64.grad.cpu(), 4 * data[64]["ref"]) < 3e-6  # (the launch that was enqueued; the exit joined it)
    again = fresh(data, dev, 64)
    with ops.deferred_wgrad():
        for s in STEPS:
            record(ops, data, dev, again, s)
    assert relerr(again.grad.cpu(), 4 * data[64]["ref"]) < 3e-6
    outside = fresh(data, dev, 64)
    record(ops, data, dev, outside)  # defer=True without a window: launched at once
    assert relerr(outside.grad.cpu(), data[64]["ref"]) < 3e-6


def test_bias_records_two_side_stream_launches(dev, data):
    """Three bias records leave with an early flush of a weight (a flush takes every pending bias), a fourth with a
    bias-only flush: both launches on the side stream, bias.grad = the column sums of all four."""
    from robot_aware_control_amd import ops
    w64 = fresh(data, dev, 64)
    bias = torch.zeros(64, device=dev).requires_grad_(True)
    dys = [rnd(70 + t, B, H, W, 64) + 0.25 for t in range(4)]
    dys_d = [d.to(dev) for d in dys]
    with ops.deferred_wgrad():
        record(ops, data, dev, w64)
        for d in dys_d[:3]:
            ops.bias_grad_acc(d, bias)
        assert untouched(bias) and len(ops._WINDOW.biases[id(bias)][1]) == 3
        ops.flush_deferred_wgrads_early([w64])
        assert not ops._WINDOW.biases and not ops._WINDOW.weights
        ops.bias_grad_acc(dys_d[3], bias)
        ops.flush_deferred_wgrads_early(None)
        assert not ops._WINDOW.biases and id(bias) in ops._WINDOW.on_side
    rule = Rule("wgrad window bias")
    sums = lambda dt: sum(d.to(dt).reshape(-1, 64).sum(0) for d in dys)
    rule.check("bias.grad", bias.grad, sums(torch.float64), sums(torch.float32))
    rule.done()
    assert relerr(w64.grad.cpu(), data[64]["ref"]) < 3e-6


def test_wgrad_on_side_stream_inside_and_outside_a_window(dev, data):
    from robot_aware_control_amd import ops
    dy = to_map(data[128]["gy"], dev)
    grads = []
    for inside in (False, True):
        wd = fresh(data, dev, 128)
        with (ops.deferred_wgrad() if inside else contextlib.nullcontext()):
            assert (ops._WINDOW is not None) == inside
            ops.wgrad_on_side_stream(lambda: ops.conv_wgrad_split_acc(dy, data["x0"], None, wd), (dy, data["x0"], None))
            assert (ops._WINDOW is not None and ops._WINDOW.done is not None) == inside
        grads.append(wd.grad)
    assert torch.equal(grads[0], grads[1]) and relerr(grads[0].cpu(), data[128]["ref"]) < 3e-6


def test_nested_window_records_into_the_outer_one(dev, data):
    from robot_aware_control_amd import ops
    w64 = fresh(data, dev, 64)
    with ops.deferred_wgrad():
        outer = ops._WINDOW
        with ops.deferred_wgrad(flush_after=1):  # (a nested context's arguments mean nothing)
            assert ops._WINDOW is outer
            for s in STEPS:
                record(ops, data, dev, w64, s)
        assert ops._WINDOW is outer and len(outer.weights[id(w64)][1]) == 3 and outer.done is None
        assert untouched(w64)
    assert ops._WINDOW is None
    assert relerr(w64.grad.cpu(), 4 * data[64]["ref"]) < 3e-6


@pytest.mark.parametrize("what", ["weight", "bias"])
def test_one_stream_rule_raises_at_the_exit(dev, data, what):
    """A parameter launched on the side stream by an early flush and recorded again would get its second launch on the main
    stream at the exit (no flush_after): RacError, and the exit still joins the side stream."""
    from robot_aware_control_amd import _lib, ops
    w64 = fresh(data, dev, 64)
    bias = torch.zeros(64, device=dev).requires_grad_(True)
    d = (rnd(80, B, H, W, 64) + 0.25).to(dev)
    with pytest.raises(_lib.RacError, match="side stream"):
        with ops.deferred_wgrad():
            window = ops._WINDOW
            record(ops, data, dev, w64)
            ops.bias_grad_acc(d, bias)
            ops.flush_deferred_wgrads_early([w64])
            if what == "weight":
                record(ops, data, dev, w64)
            else:
                ops.bias_grad_acc(d, bias)
    assert ops._WINDOW is None
    torch.cuda.current_stream().synchronize()  # the main stream waited for the side stream's last event: it has passed
    assert window.done is not None and window.done.query()
    assert relerr(w64.grad.cpu(), data[64]["ref"]) < 3e-6  # the early flush's launch, read on the main stream
    rule = Rule(f"one-stream rule ({what})")
    rows = d.cpu().reshape(-1, 64)
    rule.check("bias.grad", bias.grad, rows.double().sum(0), rows.sum(0))
    rule.done()
