"""The per-device registry of split-precision weight operands (ops._WeightStore behind ops.weight_parts, ops.weight_entry)
next to the two fused optimiser steps: a flat-buffer layout the steps decline, slot recycling, one store per device.

3x3 weights 32 -> 32 (9216 floats: the smallest the fragment kernels take) as views of small flat buffers.  Everything is
bit-equality: against rac_weight_frag_split / the exact maximum on the current values, as in test_weight_frag_split."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_ops import cl_weight, frag_order16, rnd, split_f16x2  # noqa: E402

CO = CI = 32
K = 3
N = CO * CI * K * K


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def view_at(flat, off):
    return torch.as_strided(flat, (CO, CI, K, K), (K * K * CI, 1, K * CI, CI), off)


def assert_parts_follow(w):
    """The registry's parts and slot of `w` are what the single-tensor kernels give for its values now."""
    from robot_aware_control_amd import _lib, ops
    parts, slot = ops.weight_parts(w)
    assert int(slot.item()) == int(w.abs().max().view(torch.int32).item())
    want = torch.empty_like(parts)
    _lib.call("rac_weight_frag_split", w.data_ptr(), slot.data_ptr(), want.data_ptr(), CO, CI, K, 0, w.numel(),
              _lib.stream_ptr())
    assert torch.equal(parts, want)


def test_fused_steps_decline_overlapping_views(dev, monkeypatch):
    """A registered view that overlaps registered weights is a layout neither range table describes: fused_adam_step and
    fused_optim_step return False, launch nothing and change nothing, the second time as the first (the memo); the lazy
    path then still follows the values."""
    from robot_aware_control_amd import _lib, ops
    gaps = (8, 12, 16)
    total = 2 * N + sum(gaps)
    flat = (rnd(11, total) * 0.05).to(dev)
    grad = (rnd(12, total) * 0.01).to(dev)
    m, v, sq = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
    ws = [view_at(flat, gaps[0]), view_at(flat, gaps[0] + N + gaps[1])]
    adam = lambda step: ops.fused_adam_step(flat, grad, m, v, 1e-3, 0.9, 0.999, 1e-8, step)
    rmsprop = lambda: ops.fused_optim_step(_lib.OPTIM_RMSPROP, flat, grad, sq, None, 1e-2, 0.0, 1 - 0.99, 0.99, 1e-8, 0)
    for w in ws:
        ops.weight_parts(w)
    assert adam(1) is True and rmsprop() is True  # this layout both steps take
    ws.append(view_at(flat, gaps[0] + N // 2))   # 16-byte aligned, over the second half of ws[0] and the start of ws[1]
    ops.weight_parts(ws[2])
    for w in ws:  # nothing but the layout stands in the way
        ent = ops.weight_entry(w)
        assert ent.current(w) and ent.exact_ok
    keep = [t.clone() for t in (flat, grad, m, v, sq)]
    keep_parts = [ops.weight_entry(w).parts[False].clone() for w in ws]
    keep_slots = [ops.weight_entry(w).slot.clone() for w in ws]
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for _ in range(2):
        assert adam(2) is False
        assert rmsprop() is False
    monkeypatch.setattr(ops, "call", real)
    assert calls == []
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((flat, grad, m, v, sq), keep))
    assert all(torch.equal(ops.weight_entry(w).parts[False], q) for w, q in zip(ws, keep_parts))
    assert all(torch.equal(ops.weight_entry(w).slot, s) for w, s in zip(ws, keep_slots))
    for w in ws:  # declined is not stale
        assert ops.weight_entry(w).current(w)
    # what the optimisers do next: the plain step, and the parts follow lazily
    _lib.call("rac_adam_step", flat.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), total, 1e-3, 0.9, 0.999, 1e-8, 2,
              _lib.stream_ptr())
    ops.params_changed()
    assert not torch.equal(flat, keep[0])
    assert not any(ops.weight_entry(w).current(w) for w in ws)
    for w in ws:  # (the first to ask refreshes all three)
        assert_parts_follow(w)


def test_slots_of_dead_weights_are_recycled(dev):
    from robot_aware_control_amd import ops
    gc.collect()  # (models of earlier tests that only a reference cycle keeps alive hold slots too)
    free = ops.free_weight_slots(dev)
    ws = [cl_weight(rnd(20 + i, CO, CI, K, K) * 0.02).to(dev) for i in range(3)]
    for w in ws:
        ops.weight_parts(w)
    dead = [ops.weight_entry(w) for w in ws]
    assert ops.free_weight_slots(dev) == free - 3 and len({e.slot.data_ptr() for e in dead}) == 3
    del w, ws
    gc.collect()
    assert ops.free_weight_slots(dev) == free
    assert not any(e is d for e, _ in ops.registered_weights(dev) for d in dead)
    w = cl_weight(rnd(5, CO, CI, K, K) * 0.02).to(dev)
    parts, slot = ops.weight_parts(w)
    ent = ops.weight_entry(w)
    assert all(ent is not e for e in dead)
    assert ops.free_weight_slots(dev) == free - 1
    assert slot.data_ptr() in {e.slot.data_ptr() for e in dead}  # a cell that was handed back
    h1, h2, _ = split_f16x2(w.cpu())
    assert int(slot.cpu()) == int(w.abs().max().cpu().view(torch.int32))
    assert torch.equal(parts[0].cpu(), frag_order16(h1).flatten()) and torch.equal(parts[1].cpu(), frag_order16(h2).flatten())
    assert int(ent.exact.cpu()) == int(slot.cpu()) and ent.current(w) and ent.exact_ok
    assert [e for e, x in ops.registered_weights(dev) if x is w] == [ent]


def test_one_store_per_device():
    """Weights of two devices never meet: each store lists, refreshes and counts its own."""
    from robot_aware_control_amd import ops
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    devs = [torch.device("cuda", i) for i in range(2)]
    gc.collect()
    free = [ops.free_weight_slots(d) for d in devs]
    ws = []
    for i, d in enumerate(devs):
        with torch.cuda.device(d):
            ws.append(cl_weight(rnd(30 + i, CO, CI, K, K) * 0.02).to(d))
            assert_parts_follow(ws[i])
    for i, d in enumerate(devs):
        mine = [w for _, w in ops.registered_weights(d)]
        assert any(w is ws[i] for w in mine) and all(w.device == d for w in mine)
        assert ops.free_weight_slots(d) == free[i] - 1
    with torch.cuda.device(devs[1]):  # a change on one device: its store alone has something to refresh
        ws[1].mul_(2.0)
        assert not ops.weight_entry(ws[1]).current(ws[1]) and ops.weight_entry(ws[0]).current(ws[0])
        assert_parts_follow(ws[1])
    with torch.cuda.device(devs[0]):
        assert_parts_follow(ws[0])
