"""GPU: the deterministic baselines' kernels against fp64 (tests/fp64_tools.py inputs) -- rac_det_pack_fwd,
rac_det_pack_bwd, rac_copy_baseline.

Bounds (u = 2^-24, the fp32 unit roundoff):
  * pack forward, Linear lanes: y = b + sum_{k<5} w_k a_k is a 5-term fp32 dot product plus the bias, at most 6 roundings
    whatever the association and with or without FMA: |y - y64| <= 6 u (sum_k |w_k a_k| + |b|) per element;
  * pack backward, dW / db: a B-term sum in a fixed order, products and adds rounded once each (or once per FMA), then
    added to the gradient buffer: |v - v64| <= (B + 1) u sum_b |term_b| per element;
  * everything that is a copy (encoder lanes, padding, the encoder-map gradient, the masked select) is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from robot_aware_control_amd import ops  # noqa: E402
from robot_aware_control_amd._lib import call, ptr, stream_ptr  # noqa: E402
from tests.fp64_tools import rnd  # noqa: E402

U = 2.0 ** -24
# (g, B, h, w, with state): one block / several blocks, a non-square map, the full-size width (516 -> 576)
SHAPES = [(32, 2, 8, 8, True), (64, 3, 6, 8, False), (512, 4, 8, 8, True)]
A = R = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def padded(g, with_state):
    from robot_aware_control_amd.model import det_padded_width
    return det_padded_width(g + 2 + (2 if with_state else 0))


def inputs(seed, g, B, h, w, with_state):
    hw = h * w
    t = dict(enc=rnd(seed, B, h, w, g), act=rnd(seed + 1, B, A), wa=rnd(seed + 2, 2 * hw, A, scale=A ** -0.5),
             ba=rnd(seed + 3, 2 * hw, scale=0.05))
    if with_state:
        t.update(st=rnd(seed + 4, B, R), ws=rnd(seed + 5, 2 * hw, R, scale=R ** -0.5), bs=rnd(seed + 6, 2 * hw, scale=0.05))
    return t


def linear64(w, b, v, B, h, wd):
    """(value, sum of |terms|) of b + w v in fp64, as (B, h, w, 2) lanes."""
    terms = w.double()[None] * v.double()[:, None]                       # (B, 2hw, k)
    val = terms.sum(-1) + b.double()[None]
    mag = terms.abs().sum(-1) + b.double().abs()[None]
    lanes = lambda t: t.view(B, 2, h, wd).permute(0, 2, 3, 1)
    return lanes(val), lanes(mag)


@pytest.mark.parametrize("g,B,h,w,with_state", SHAPES)
def test_det_pack_fwd_vs_fp64(dev, g, B, h, w, with_state):
    gp = padded(g, with_state)
    t = inputs(11, g, B, h, w, with_state)
    d = {k: v.to(dev) for k, v in t.items()}
    out = torch.full((B, h, w, gp), float("nan"), device=dev)
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    call("rac_det_pack_fwd", ptr(d["enc"]), g, ptr(d["act"]), A, ptr(d["wa"]), ptr(d["ba"]), ptr(d.get("st")),
         R if with_state else 0, ptr(d.get("ws")), ptr(d.get("bs")), ptr(out), gp, B, h * w, ptr(slot), stream_ptr())
    got = out.cpu()
    assert torch.equal(got[..., :g], t["enc"])                           # encoder lanes: the input's bits
    used = g + (4 if with_state else 2)
    assert bool((got[..., used:] == 0).all()) and used < gp              # padding: exact zeros
    lanes = [("action", t["wa"], t["ba"], t["act"], g)]
    if with_state:
        lanes.append(("state", t["ws"], t["bs"], t["st"], g + 2))
    for name, wt, b, v, c0 in lanes:
        ref, mag = linear64(wt, b, v, B, h, w)
        err = (got[..., c0:c0 + 2].double() - ref).abs()
        worst = float((err / (6 * U * mag)).max())
        print(f"[det_pack_fwd g{g} B{B} {h}x{w}] {name}: max err / bound = {worst:.3f}")
        assert worst <= 1.0, name
    true_max = float(got.abs().max())
    amax = float(slot.cpu().view(torch.float32))
    assert true_max <= amax <= true_max * (1 + 2.0 ** -23), (true_max, amax)


def run_bwd(d, dout, g, gp, B, hw, with_state):
    dev = dout.device
    denc = torch.full((B, hw, g), float("nan"), device=dev)
    dwa, dba = torch.zeros(2 * hw, A, device=dev), torch.zeros(2 * hw, device=dev)
    dws = torch.zeros(2 * hw, R, device=dev) if with_state else None
    dbs = torch.zeros(2 * hw, device=dev) if with_state else None
    call("rac_det_pack_bwd", ptr(dout), gp, g, ptr(d["act"]), A, ptr(d.get("st")), R if with_state else 0, ptr(denc),
         ptr(dwa), ptr(dba), ptr(dws), ptr(dbs), B, hw, stream_ptr())
    return denc, dwa, dba, dws, dbs


@pytest.mark.parametrize("g,B,h,w,with_state", SHAPES)
def test_det_pack_bwd_vs_fp64(dev, g, B, h, w, with_state):
    gp, hw = padded(g, with_state), h * w
    t = inputs(21, g, B, h, w, with_state)
    d = {k: v.to(dev) for k, v in t.items()}
    dout_h = rnd(29, B, h, w, gp)
    dout = dout_h.to(dev)
    first = run_bwd(d, dout, g, gp, B, hw, with_state)
    second = run_bwd(d, dout, g, gp, B, hw, with_state)
    for a_, b_ in zip(first, second):                                    # a fixed summation order: the same bits
        assert (a_ is None and b_ is None) or torch.equal(a_, b_)
    denc, dwa, dba, dws, dbs = [None if x is None else x.cpu() for x in first]
    assert torch.equal(denc.view(B, h, w, g), dout_h[..., :g])           # encoder-map gradient: a copy
    cases = [("action", dwa, dba, t["act"], g)]
    if with_state:
        cases.append(("state", dws, dbs, t["st"], g + 2))
    for name, dw, db, v, c0 in cases:
        # d[b, o] with o = ch * hw + p
        dl = dout_h[..., c0:c0 + 2].permute(0, 3, 1, 2).reshape(B, 2 * hw).double()
        terms = dl[:, :, None] * v.double()[:, None, :]                  # (B, 2hw, k)
        for what, got, ref, mag in ((f"{name} dW", dw, terms.sum(0), terms.abs().sum(0)),
                                    (f"{name} db", db, dl.sum(0), dl.abs().sum(0))):
            worst = float(((got.double() - ref).abs() / ((B + 1) * U * mag)).max())
            print(f"[det_pack_bwd g{g} B{B} {h}x{w}] {what}: max err / bound = {worst:.3f}")
            assert worst <= 1.0, what


def test_det_pack_autograd_wrapper(dev):
    """ops.DetPack: the forward launch tags its output's maximum, the backward launch adds into the Linears' .grad
    (twice: two time steps of a window) and hands the encoder map its gradient; action and state get none."""
    g, B, h, w = 32, 2, 8, 8
    gp, hw = padded(g, True), h * w
    t = inputs(31, g, B, h, w, True)
    d = {k: v.to(dev) for k, v in t.items()}
    enc = d["enc"].clone().requires_grad_(True)
    params = {k: d[k].clone().requires_grad_(True) for k in ("wa", "ba", "ws", "bs")}
    for p in params.values():
        p.grad = torch.zeros_like(p)
    act, st = d["act"].clone().requires_grad_(True), d["st"].clone().requires_grad_(True)
    out = ops.DetPack.apply(enc, act, params["wa"], params["ba"], st, params["ws"], params["bs"], gp)
    assert tuple(out.shape) == (B, h, w, gp)
    slot = ops.amax_tag(out)
    assert slot is not None and float(slot.cpu().view(torch.float32)) == float(out.detach().abs().max())
    dout = rnd(33, B, h, w, gp).to(dev)
    out.backward(dout, retain_graph=True)
    once = run_bwd(d, dout, g, gp, B, hw, True)
    assert torch.equal(enc.grad, dout[..., :g]) and act.grad is None and st.grad is None
    for p, ref in zip(params.values(), once[1:]):
        assert torch.equal(p.grad, ref)
    out.backward(dout)
    for p, ref in zip(params.values(), once[1:]):
        assert torch.equal(p.grad, ref + ref)                            # accumulated, x + x is exact


@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (3, 48, 64)])
@pytest.mark.parametrize("mask_kind", ["zeros", "ones", "mixed"])
def test_copy_baseline_is_the_masked_select(dev, B, H, W, mask_kind):
    g = np.random.Generator(np.random.Philox(key=[41, B]))
    image = torch.from_numpy(g.random((B, 3, H, W), dtype=np.float32))
    nxt = torch.from_numpy(g.random((B, 3, H, W), dtype=np.float32))
    mask = {"zeros": torch.zeros(B, 1, H, W), "ones": torch.ones(B, 1, H, W),
            "mixed": torch.from_numpy((g.random((B, 1, H, W)) < 0.3).astype(np.float32))}[mask_kind]
    want = torch.where(mask.bool().repeat(1, 3, 1, 1), nxt, image)
    got = ops.copy_baseline(image.to(dev), nxt.to(dev), mask.to(dev))
    assert torch.equal(got.cpu(), want)
    from robot_aware_control_amd.model import CopyModel
    model = CopyModel()
    model.init_hidden(B)
    assert torch.equal(model(image.to(dev), None, nxt.to(dev), mask.to(dev).bool()).cpu(), want)
