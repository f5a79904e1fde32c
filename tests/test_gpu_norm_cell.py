"""The GroupNorm LSTM cell's kernels (NormConvLSTMCell, `--lstm_group_norm True`, lstm.py:151-198) against torch on the CPU
in fp64, at every width the fused kernels admit and in both of their launch forms.

Tolerance rule of every comparison here: with e_gpu = relerr(kernel, fp64 reference) and e_cpu32 = relerr(the same formula
in fp32 on the CPU with torch, fp64 reference), e_gpu <= max(2e-6, 4 * e_cpu32) -- 2e-6 is this suite's fp32-kernel-vs-fp64
bound, 4x its margin over a yardstick (test_gpu_ops.py); where a comparison passes through the split-precision gate convs
the floor is 5e-6, the suite's form-to-form bound.  Every case prints both figures; nothing is excluded."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import svg_oracle as orc  # noqa: E402
from tests.fp64_tools import Rule, relerr, rnd  # noqa: E402

EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to_map(x, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(dev)


def from_map(m):
    return m.permute(0, 3, 1, 2).cpu()


def leaf(t, dt, grad=True):
    """A fresh copy of `t` in precision `dt` as an autograd leaf (`t.to(dt)` is `t` itself where the type already fits)."""
    return t.detach().clone().to(dt).requires_grad_(grad)


def grads_of(outs, seeds, leaves):
    """d(sum_i <outs_i, seeds_i>) / d leaves on the CPU (autograd), None -> zeros."""
    got = torch.autograd.grad(outs, leaves, seeds, retain_graph=True, allow_unused=True)
    return [torch.zeros_like(lf) if g is None else g for g, lf in zip(got, leaves)]


# --------------------------------------------------------------------------- 1. GroupNorm
GN_SHAPES = [(3, 6, 8, 16, 16), (3, 6, 8, 32, 16), (2, 8, 8, 64, 16), (5, 6, 8, 1024, 16), (2, 8, 8, 4096, 16),
             (2, 5, 7, 64, 16), (2, 12, 16, 128, 16), (130, 2, 4, 64, 16), (2, 8, 8, 64, 4)]


def gn_input(kind, B, H, W, C, G):
    x = rnd(1, B, C, H, W)
    Cg = C // G
    if kind == "offset":  # a per-group offset of 50 (alternating sign, growing a little with the group) under a spread of 1.3
        off = torch.tensor([50.0 * (1 + 0.01 * j) * (1 if j % 2 == 0 else -1) for j in range(G)])
        x = x * 1.3 + off.repeat_interleave(Cg).view(1, C, 1, 1)
    if kind == "zero_group":
        zg = min(3, G - 1)
        x[0, zg * Cg:(zg + 1) * Cg] = 0.0
    return x


@pytest.mark.parametrize("kind", ["plain", "offset", "zero_group"])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_vs_fp64(dev, shape, kind):
    """ops.GroupNorm (rac_groupnorm_fwd / _bwd) against F.group_norm and autograd in fp64: y, dx, dgamma, dbeta; a second
    backward adds the same affine gradients again (+=); without affine gradients dx is the same bits; an all-zero group
    gives y = beta to the bit and finite gradients; a group offset of 50 under a spread of 1.3 (two-pass variance)."""
    from robot_aware_control_amd import ops
    B, H, W, C, G = shape
    Cg = C // G
    x = gn_input(kind, B, H, W, C, G)
    gamma, beta = 1 + rnd(2, C, scale=0.1), rnd(3, C, scale=0.1)
    dy = rnd(4, B, C, H, W)
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = [leaf(t, dt) for t in (x, gamma, beta)]
        y = F.group_norm(leaves[0], G, leaves[1], leaves[2], EPS)
        ref[dt] = [y.detach()] + grads_of([y], [dy.to(dt)], leaves)
    xm = to_map(x, dev).requires_grad_(True)
    gm, bm = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    dym = to_map(dy, dev)
    y = ops.GroupNorm.apply(xm, gm, bm, G)
    y.backward(dym)
    torch.cuda.synchronize()
    rule = Rule(f"groupnorm {shape} {kind}")
    got = [from_map(y), from_map(xm.grad), gm.grad.cpu(), bm.grad.cpu()]
    for name, a, r64, r32 in zip(("y", "dx", "dgamma", "dbeta"), got, ref[torch.float64], ref[torch.float32]):
        rule.check(name, a, r64, r32)
    if kind == "zero_group":
        zg = min(3, G - 1)
        sl = slice(zg * Cg, (zg + 1) * Cg)
        assert torch.equal(y[0, :, :, sl].cpu(), beta[sl].view(1, 1, Cg).expand(H, W, Cg)), "all-zero group: y != beta"
        assert all(bool(torch.isfinite(t).all()) for t in got)
    # += : a second pass over the same graph leaves twice the affine gradients
    dx_first = xm.grad.clone()
    xm.grad = None
    ops.GroupNorm.apply(xm, gm, bm, G).backward(dym)
    torch.cuda.synchronize()
    assert torch.equal(xm.grad, dx_first)
    rule.check("dgamma twice", gm.grad, 2 * ref[torch.float64][2], 2 * ref[torch.float32][2])
    rule.check("dbeta twice", bm.grad, 2 * ref[torch.float64][3], 2 * ref[torch.float32][3])
    # no affine gradients wanted: only dx, the same bits
    g0, b0 = gamma.to(dev), beta.to(dev)
    x0 = to_map(x, dev).requires_grad_(True)
    y0 = ops.GroupNorm.apply(x0, g0, b0, G)
    y0.backward(dym)
    torch.cuda.synchronize()
    assert torch.equal(y0, y) and torch.equal(x0.grad, dx_first) and g0.grad is None and b0.grad is None
    rule.done()


# --------------------------------------------------------------------------- the cell's pointwise part, on the CPU
def cell_inputs(B, H, W, g):
    """Planes (NCHW, fp32, CPU) of the two gate convs' outputs, the previous cell and the three norms' affines."""
    g_ih = rnd(1, B, 4 * g, H, W) * 1.3 + 0.2
    g_hh = rnd(2, B, 4 * g, H, W) * 0.7 - 0.1
    c_prev = rnd(3, B, g, H, W)
    gn = [(1 + rnd(10 + i, n, scale=0.1), rnd(20 + i, n, scale=0.1)) for i, n in enumerate((4 * g, 4 * g, g))]
    return g_ih, g_hh, c_prev, gn


def group_stats(x, G=16):
    """mean and 1 / std of every (image, group) of an NCHW map: [2][B][G]."""
    B = x.shape[0]
    v = x.reshape(B, G, -1)
    return torch.stack([v.mean(2), 1.0 / torch.sqrt(v.var(2, unbiased=False) + EPS)])


def cell_ref(g_ih, g_hh, c_prev, gn, dt, grad=False):
    """lstm.py:174-198 behind the gate convs in precision `dt`: dict of h, c, act, c_raw, the stats, and the leaves."""
    leaves = [leaf(t, dt, grad) for t in (g_ih, g_hh, c_prev, gn[0][0], gn[0][1], gn[1][0], gn[1][1], gn[2][0], gn[2][1])]
    a, b, cp, ga, ba, gb, bb, gc, bc = leaves
    gates = F.group_norm(a, 16, ga, ba, EPS) + F.group_norm(b, 16, gb, bb, EPS)
    i_, f_, o_, gg = gates.chunk(4, 1)
    act = torch.cat([torch.sigmoid(i_), torch.sigmoid(f_), torch.sigmoid(o_), torch.tanh(gg)], 1)
    gi, gf, go, gt = act.chunk(4, 1)
    c_raw = gf * cp + gi * gt
    c = F.group_norm(c_raw, 16, gc, bc, EPS)
    h = go * torch.tanh(c)
    return dict(h=h, c=c, act=act, c_raw=c_raw, stat_ih=group_stats(a.detach()), stat_hh=group_stats(b.detach()),
                stat_c=group_stats(c_raw.detach()), leaves=leaves)


def unfused_pointwise(ops, g_ih, g_hh, c_prev, gn):
    """The seven-node form's pointwise kernels on device maps: (h, c, act, c_raw)."""
    n_ih = ops.GroupNorm.apply(g_ih, gn[0][0], gn[0][1], 16)
    n_hh = ops.GroupNorm.apply(g_hh, gn[1][0], gn[1][1], 16)
    c_raw, act = ops.NormCellCore.apply(n_ih, n_hh, c_prev)
    c = ops.GroupNorm.apply(c_raw, gn[2][0], gn[2][1], 16)
    return ops.LstmOut.apply(act, c), c, act, c_raw


# --------------------------------------------------------------------------- 2. cell core and output kernels
@pytest.mark.parametrize("g", [16, 64, 256])
def test_norm_cell_core_and_out_vs_fp64(dev, g):
    """ops.NormCellCore (rac_lstm_cell_fwd on two slabs / rac_lstm_core_bwd) and ops.LstmOut (rac_lstm_out_fwd / _bwd) around
    ops.GroupNorm of the cell, against fp64 autograd: c_raw, act, h and every input gradient with the gradient on h only, on
    c only and on both; then rac_lstm_core_bwd itself with dc_raw == NULL and with d_act == NULL (autograd hands the node
    zeros, never None) against the closed form and against the same call with explicit zeros."""
    from robot_aware_control_amd import ops
    from robot_aware_control_amd._lib import call, ptr, stream_ptr
    B, H, W = 3, 6, 8
    n_ih, n_hh, c_prev, gn = cell_inputs(B, H, W, g)
    gam_c, bet_c = gn[2]
    seed_h, seed_c = rnd(5, B, g, H, W), rnd(6, B, g, H, W)
    rule = Rule(f"core+out g={g}")
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = [leaf(t, dt) for t in (n_ih, n_hh, c_prev, gam_c, bet_c)]
        a, b, cp, gc, bc = leaves
        i_, f_, o_, gg = (a + b).chunk(4, 1)
        act = torch.cat([torch.sigmoid(i_), torch.sigmoid(f_), torch.sigmoid(o_), torch.tanh(gg)], 1)
        c_raw = act[:, g:2 * g] * cp + act[:, :g] * act[:, 3 * g:]
        c = F.group_norm(c_raw, 16, gc, bc, EPS)
        h = act[:, 2 * g:3 * g] * torch.tanh(c)
        ref[dt] = dict(c_raw=c_raw.detach(), act=act.detach(), c=c.detach(), h=h.detach(),
                       on_h=grads_of([h], [seed_h.to(dt)], leaves), on_c=grads_of([c], [seed_c.to(dt)], leaves),
                       on_both=grads_of([h, c], [seed_h.to(dt), seed_c.to(dt)], leaves))
    for which in ("on_h", "on_c", "on_both"):
        leaves = [to_map(t, dev).requires_grad_(True) for t in (n_ih, n_hh, c_prev)] + [gam_c.to(dev).requires_grad_(True),
                                                                                         bet_c.to(dev).requires_grad_(True)]
        c_raw, act = ops.NormCellCore.apply(leaves[0], leaves[1], leaves[2])
        c = ops.GroupNorm.apply(c_raw, leaves[3], leaves[4], 16)
        h = ops.LstmOut.apply(act, c)
        if which == "on_h":
            h.backward(to_map(seed_h, dev))
        elif which == "on_c":
            c.backward(to_map(seed_c, dev))
        else:
            torch.autograd.backward([h, c], [to_map(seed_h, dev), to_map(seed_c, dev)])
        torch.cuda.synchronize()
        if which == "on_h":
            for name, t in (("c_raw", c_raw), ("act", act), ("c", c), ("h", h)):
                rule.check(name, from_map(t), ref[torch.float64][name], ref[torch.float32][name])
        for name, lf, r64, r32 in zip(("d n_ih", "d n_hh", "d c_prev", "d gamma_c", "d beta_c"), leaves,
                                      ref[torch.float64][which], ref[torch.float32][which]):
            got = lf.grad if lf.grad.dim() == 1 else from_map(lf.grad)
            rule.check(f"{which} {name}", got, r64, r32)
    # rac_lstm_core_bwd with NULL operands, on the activations of the last forward pass
    M = B * H * W
    act_d, cp_d = act.detach(), to_map(c_prev, dev)
    dcr_d, dact_d = to_map(seed_c, dev), to_map(rnd(7, B, 4 * g, H, W), dev)

    def core_bwd(dc_raw, d_act):
        dgates, dcp = torch.full_like(act_d, float("nan")), torch.full_like(cp_d, float("nan"))
        call("rac_lstm_core_bwd", ptr(dc_raw), ptr(d_act), ptr(act_d), ptr(cp_d), ptr(dgates), ptr(dcp), M, g, stream_ptr())
        torch.cuda.synchronize()
        return dgates, dcp

    def core_closed(dc_raw, d_act, dt):
        a, cp = from_map(act_d).to(dt), c_prev.to(dt)
        gi, gf, go, gt = a.chunk(4, 1)
        dc = from_map(dc_raw).to(dt) if dc_raw is not None else torch.zeros_like(cp)
        e = (from_map(d_act).to(dt) if d_act is not None else torch.zeros_like(a)).chunk(4, 1)
        dg = torch.cat([(dc * gt + e[0]) * gi * (1 - gi), (dc * cp + e[1]) * gf * (1 - gf), e[2] * go * (1 - go),
                        (dc * gi + e[3]) * (1 - gt * gt)], 1)
        return dg, dc * gf

    for name, dc_raw, d_act in (("dc_raw NULL", None, dact_d), ("d_act NULL", dcr_d, None), ("both given", dcr_d, dact_d)):
        dgates, dcp = core_bwd(dc_raw, d_act)
        r64, r32 = core_closed(dc_raw, d_act, torch.float64), core_closed(dc_raw, d_act, torch.float32)
        rule.check(f"core_bwd {name} dgates", from_map(dgates), r64[0], r32[0])
        rule.check(f"core_bwd {name} dc_prev", from_map(dcp), r64[1], r32[1])
        z_gates, z_cp = core_bwd(dc_raw if dc_raw is not None else torch.zeros_like(cp_d),
                                 d_act if d_act is not None else torch.zeros_like(act_d))
        assert torch.equal(z_gates, dgates) and torch.equal(z_cp, dcp), name
    rule.done()


# --------------------------------------------------------------------------- 3. the fused forward kernel
WIDTHS = (16, 32, 64, 128, 256, 1024)
FWD_CASES = ([(B, H, W, g) for g in WIDTHS for (B, H, W) in ((5, 6, 8), (1, 8, 8), (2, 12, 16))]
             + [(B, H, W, g) for g in (64, 256) for (B, H, W) in ((130, 2, 4), (128, 6, 8))])  # ... and its 256-thread form


@pytest.mark.parametrize("B,H,W,g", FWD_CASES)
def test_fused_forward_every_width_and_both_forms(dev, B, H, W, g):
    """rac_norm_lstm_cell_fwd against fp64 at every width ops.norm_cell_frozen_ok admits: h and c of the frozen form, and
    of the training form also the activated gates, the raw cell and the three norms' mean and 1 / std of every
    (image, group).  A width the predicate rejects runs the unfused kernels (what the module then takes) under the same rule."""
    from robot_aware_control_amd import ops
    g_ih, g_hh, c_prev, gn = cell_inputs(B, H, W, g)
    r64, r32 = cell_ref(g_ih, g_hh, c_prev, gn, torch.float64), cell_ref(g_ih, g_hh, c_prev, gn, torch.float32)
    d_ih, d_hh, d_cp = to_map(g_ih, dev), to_map(g_hh, dev), to_map(c_prev, dev)
    d_gn = [(w.to(dev), b.to(dev)) for w, b in gn]
    rule = Rule(f"fused fwd {(B, H, W, g)}")
    if not ops.norm_cell_frozen_ok(g):
        with torch.no_grad():
            h, c, act, c_raw = unfused_pointwise(ops, d_ih, d_hh, d_cp, d_gn)
        torch.cuda.synchronize()
        for name, t in (("unfused h", h), ("unfused c", c), ("unfused act", act), ("unfused c_raw", c_raw)):
            rule.check(name, from_map(t), r64[name.split()[1]].detach(), r32[name.split()[1]].detach())
        rule.done()
        return
    h, c = ops.norm_cell_frozen(d_ih, d_hh, d_cp, *d_gn)
    torch.cuda.synchronize()
    rule.check("frozen h", from_map(h), r64["h"], r32["h"])
    rule.check("frozen c", from_map(c), r64["c"], r32["c"])
    h, c, act, c_raw, stats = ops._norm_cell_launch(d_ih, d_hh, d_cp, *d_gn, True)[:5]
    torch.cuda.synchronize()
    for name, t in (("h", h), ("c", c), ("act", act), ("c_raw", c_raw)):
        rule.check(f"training {name}", from_map(t), r64[name].detach(), r32[name].detach())
    for i, name in enumerate(("stat_ih", "stat_hh", "stat_c")):
        rule.check(f"training {name} mean", stats[i, 0], r64[name][0], r32[name][0])
        rule.check(f"training {name} rstd", stats[i, 1], r64[name][1], r32[name][1])
    rule.done()


@pytest.mark.parametrize("B,H,W,g", [(5, 6, 8, 64), (3, 6, 8, 128), (2, 8, 8, 1024), (130, 2, 4, 64), (128, 6, 8, 256)])
@pytest.mark.parametrize("seeds", ["h_c", "h", "c"])
def test_fused_backward_vs_fp64(dev, B, H, W, g, seeds):
    """rac_norm_lstm_cell_bwd through the C ABI against fp64 autograd of the pointwise part: dg_ih, dg_hh, dc_prev, the six
    affine gradients and the two max |.| slots, with both incoming gradients, with dc == NULL and with dh == NULL (autograd
    hands a node zeros, so only a direct call reaches those branches); a second call adds the affine gradients again (+=);
    without affine gradients the three maps are the same bits."""
    from robot_aware_control_amd import ops
    from robot_aware_control_amd._lib import call, ptr, stream_ptr
    if not ops.norm_cell_frozen_ok(g):
        pytest.fail(f"g = {g} is a width the fused kernels must admit")
    g_ih, g_hh, c_prev, gn = cell_inputs(B, H, W, g)
    seed_h, seed_c = rnd(5, B, g, H, W), rnd(6, B, g, H, W)
    ref = {}
    for dt in (torch.float64, torch.float32):
        r = cell_ref(g_ih, g_hh, c_prev, gn, dt, grad=True)
        outs = [r[k] for k in ("h", "c") if k in seeds.split("_")]
        sd = [s.to(dt) for s, k in ((seed_h, "h"), (seed_c, "c")) if k in seeds.split("_")]
        ref[dt] = grads_of(outs, sd, r["leaves"])
    d_ih, d_hh, d_cp = to_map(g_ih, dev), to_map(g_hh, dev), to_map(c_prev, dev)
    d_gn = [(w.to(dev), b.to(dev)) for w, b in gn]
    h, c, act, c_raw, stats = ops._norm_cell_launch(d_ih, d_hh, d_cp, *d_gn, True)[:5]
    dh = to_map(seed_h, dev) if "h" in seeds.split("_") else None
    dc = to_map(seed_c, dev) if "c" in seeds.split("_") else None

    def bwd(aff):
        dg_ih, dg_hh, dcp = (torch.full_like(act, float("nan")), torch.full_like(act, float("nan")),
                             torch.full_like(c, float("nan")))
        slots = torch.zeros(2, device=dev, dtype=torch.int32)
        a = [ptr(t) for t in aff] if aff is not None else [None] * 6
        call("rac_norm_lstm_cell_bwd", ptr(dh), ptr(dc), ptr(act), ptr(c), ptr(c_raw), ptr(d_cp), ptr(d_ih), ptr(d_hh),
             ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(d_gn[0][0]), ptr(d_gn[1][0]), ptr(d_gn[2][0]), ptr(dg_ih),
             ptr(dg_hh), ptr(dcp), a[0], a[1], a[2], a[3], a[4], a[5], ptr(slots[0:1]), ptr(slots[1:2]), B, H * W, g,
             stream_ptr())
        torch.cuda.synchronize()
        return dg_ih, dg_hh, dcp, slots

    # (dgamma_ih, dbeta_ih, dgamma_hh, dbeta_hh, dgamma_c, dbeta_c), zeroed: the kernel adds
    aff = [torch.zeros(n, device=dev) for n in (4 * g, 4 * g, 4 * g, 4 * g, g, g)]
    dg_ih, dg_hh, dcp, slots = bwd(aff)
    rule = Rule(f"fused bwd {(B, H, W, g)} seeds {seeds}")
    r64, r32 = ref[torch.float64], ref[torch.float32]
    names = ("dg_ih", "dg_hh", "dc_prev", "dgamma_ih", "dbeta_ih", "dgamma_hh", "dbeta_hh", "dgamma_c", "dbeta_c")
    got = [from_map(dg_ih), from_map(dg_hh), from_map(dcp)] + [t.cpu() for t in aff]
    for name, a, x64, x32 in zip(names, got, r64, r32):
        rule.check(name, a, x64, x32)
    assert int(slots[0].item()) == int(dg_ih.abs().max().view(torch.int32).item()), "max |dg_ih| slot"
    assert int(slots[1].item()) == int(dg_hh.abs().max().view(torch.int32).item()), "max |dg_hh| slot"
    again = bwd(aff)
    assert all(torch.equal(a, b) for a, b in zip(again[:3], (dg_ih, dg_hh, dcp)))
    for name, a, x64, x32 in zip(names[3:], aff, r64[3:], r32[3:]):
        rule.check(f"{name} twice", a, 2 * x64, 2 * x32)
    plain = bwd(None)
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], (dg_ih, dg_hh, dcp))), "no-affine-gradient path: other bits"
    rule.done()


# --------------------------------------------------------------------------- 4. batch invariance across the launch forms
@pytest.mark.parametrize("g", [64, 256])
def test_fused_cell_is_batch_invariant_across_launch_forms(dev, g):
    """include/rac_hip.h: "an image's result does not depend on the batch" -- the frozen form of rac_norm_lstm_cell_fwd gives
    the same bits for an image in a batch of 130 (past the workgroup count at which the launcher's thread count used to
    change), alone, in a pair and among the first 12; images of magnitudes 1, 3e-4, 2e3, 0.07, 11 in rotation."""
    from robot_aware_control_amd import ops
    B, H, W = 130, 6, 8
    g_ih, g_hh, c_prev, gn = cell_inputs(B, H, W, g)
    mags = torch.tensor([1.0, 3e-4, 2e3, 0.07, 11.0])[torch.arange(B) % 5].view(B, 1, 1, 1)
    d_ih, d_hh, d_cp = to_map(g_ih * mags, dev), to_map(g_hh * mags, dev), to_map(c_prev * mags, dev)
    d_gn = [(w.to(dev), b.to(dev)) for w, b in gn]
    h_full, c_full = ops.norm_cell_frozen(d_ih, d_hh, d_cp, *d_gn)
    assert bool(torch.isfinite(h_full).all()) and bool(torch.isfinite(c_full).all())
    for idx in ([0], [1], [7], [129], [3, 77], [128, 2], list(range(12))):
        ix = torch.tensor(idx, device=dev)
        h, c = ops.norm_cell_frozen(d_ih[ix].contiguous(), d_hh[ix].contiguous(), d_cp[ix].contiguous(), *d_gn)
        torch.cuda.synchronize()
        assert torch.equal(h, h_full[ix]), ("h", g, idx, relerr(h, h_full[ix]))
        assert torch.equal(c, c_full[ix]), ("c", g, idx, relerr(c, c_full[ix]))


# --------------------------------------------------------------------------- 5. the module against the oracle
MODULE_CASES = [(32, 3, 3, 8, 8), (32, 5, 130, 2, 4), (64, 5, 2, 8, 8), (128, 3, 4, 6, 8), (64, 3, 130, 6, 8)]
LOSSES = {"h2_c2_h1": ("h2", "c2", "h1"), "h2": ("h2",), "c2": ("c2",)}
_MODULE_REF = {}


def module_problem(g, k, B, H, W):
    params = {}
    for i, (name, shape) in enumerate((("ih_gates.0.weight", (4 * g, g, k, k)), ("ih_gates.0.bias", (4 * g,)),
                                       ("ih_gates.1.weight", (4 * g,)), ("ih_gates.1.bias", (4 * g,)),
                                       ("hh_gates.0.weight", (4 * g, g, k, k)), ("hh_gates.0.bias", (4 * g,)),
                                       ("hh_gates.1.weight", (4 * g,)), ("hh_gates.1.bias", (4 * g,)),
                                       ("c_norm.weight", (g,)), ("c_norm.bias", (g,)))):
        p = rnd(40 + i, *shape, scale=(1.0 / np.sqrt(g * k * k)) if len(shape) == 4 else 0.1)
        params[name] = p + 1.0 if name in ("ih_gates.1.weight", "hh_gates.1.weight", "c_norm.weight") else p
    inputs = dict(x1=rnd(1, B, g, H, W), x2=rnd(2, B, g, H, W), h0=rnd(3, B, g, H, W) * 0.5, c0=rnd(4, B, g, H, W))
    seeds = dict(h2=rnd(5, B, g, H, W), c2=rnd(6, B, g, H, W), h1=0.3 * rnd(5, B, g, H, W))
    return params, inputs, seeds


def module_reference(case):
    """The oracle's two chained steps in fp64 and fp32: outputs, and per loss the gradients of inputs and parameters;
    the frozen first step from a zero state with a zero hh bias."""
    if case in _MODULE_REF:
        return _MODULE_REF[case]
    g, k, B, H, W = case
    layer = 0 if k == 5 else 1  # (the oracle pads 2 in layer 0, 1 in layer 1)
    params, inputs, seeds = module_problem(*case)
    out = {}
    for dt in (torch.float64, torch.float32):
        sd = {f"p.lstm.{layer}.{n}": leaf(v, dt) for n, v in params.items()}
        inp = {n: leaf(v, dt) for n, v in inputs.items()}
        h1, c1 = orc.norm_convlstm_cell(sd, "p", layer, inp["x1"], (inp["h0"], inp["c0"]))
        h2, c2 = orc.norm_convlstm_cell(sd, "p", layer, inp["x2"], (h1, c1))
        outs = dict(h1=h1, c1=c1, h2=h2, c2=c2)
        leaves = list(inp.values()) + list(sd.values())
        names = list(inp) + list(params)
        r = dict(outs={n: v.detach() for n, v in outs.items()}, grads={})
        for key, terms in LOSSES.items():
            r["grads"][key] = dict(zip(names, grads_of([outs[t] for t in terms], [seeds[t].to(dt) for t in terms], leaves)))
        with torch.no_grad():
            sd0 = {n: v.detach().clone() for n, v in sd.items()}
            sd0[f"p.lstm.{layer}.hh_gates.0.bias"].zero_()
            zero = torch.zeros_like(inp["x1"])
            r["first"] = dict(zip(("h", "c"), orc.norm_convlstm_cell(sd0, "p", layer, inp["x1"].detach(), (zero, zero))))
        out[dt] = r
    _MODULE_REF[case] = out
    return out


def make_cell(mdl, case, dev):
    g, k = case[:2]
    params = module_problem(*case)[0]
    cell = mdl._NormLstmCell(g, k).to(dev)
    with torch.no_grad():
        for name, p in cell.named_parameters():
            p.copy_(params[name].to(dev))
    return cell


@pytest.mark.parametrize("mode", ["default", "bwd_unfused", "node_off"])
@pytest.mark.parametrize("case", MODULE_CASES, ids=lambda c: "g{}k{}_{}x{}x{}".format(*c))
def test_norm_cell_module_vs_fp64_oracle(dev, monkeypatch, case, mode):
    """model._NormLstmCell against oracle.norm_convlstm_cell in fp64 over two chained steps, through whichever path
    model.py selects (and with the one-launch backward / the one-node form switched off): training -- h1, c1, h2, c2, the four
    input gradients and every parameter's gradient, with the loss on (h2, c2, h1), on h2 alone and on c2 alone; frozen -- the
    outputs, and a first step from the zero state with a zero hh bias (every hh group all zeros)."""
    from robot_aware_control_amd import model as mdl, ops
    if mode == "bwd_unfused":
        monkeypatch.setattr(ops, "NORM_CELL_BWD_FUSED", False)
    if mode == "node_off":
        monkeypatch.setattr(ops, "NORM_CELL_NODE", False)
        monkeypatch.setattr(ops, "NORM_CELL_BWD_FUSED", False)
    g, k, B, H, W = case
    ref = module_reference(case)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    _, inputs, seeds = module_problem(*case)
    rule = Rule(f"module {case} {mode}", floor=5e-6)
    for key, terms in LOSSES.items():
        cell = make_cell(mdl, case, dev)
        inp = {n: to_map(v, dev).requires_grad_(True) for n, v in inputs.items()}
        with ops.deferred_wgrad():
            h1, c1 = cell(inp["x1"], (ops.tag_amax(inp["h0"], ops.amax_of(inp["h0"])), inp["c0"]))
            h2, c2 = cell(inp["x2"], (h1, c1))
            outs = dict(h1=h1, c1=c1, h2=h2, c2=c2)
            torch.autograd.backward([outs[t] for t in terms], [to_map(seeds[t], dev) for t in terms])
        torch.cuda.synchronize()
        if key == "h2_c2_h1":
            for n, t in outs.items():
                rule.check(f"train {n}", from_map(t), r64["outs"][n], r32["outs"][n])
        for n, t in inp.items():
            assert t.grad is not None, (key, n)
            rule.check(f"loss {key}: d {n}", from_map(t.grad), r64["grads"][key][n], r32["grads"][key][n])
        for n, p in cell.named_parameters():
            assert p.grad is not None, (key, n)
            rule.check(f"loss {key}: d {n}", p.grad, r64["grads"][key][n], r32["grads"][key][n])
    if mode == "default":
        cell = make_cell(mdl, case, dev)
        with torch.no_grad():
            inp = {n: to_map(v, dev) for n, v in inputs.items()}
            h1, c1 = cell(inp["x1"], (inp["h0"], inp["c0"]))
            h2, c2 = cell(inp["x2"], (h1, c1))
            for n, t in dict(h1=h1, c1=c1, h2=h2, c2=c2).items():
                rule.check(f"frozen {n}", from_map(t), r64["outs"][n], r32["outs"][n])
            cell.hh_gates[0].bias.zero_()
            z0 = ops.tag_amax(torch.zeros(B, H, W, g, device=dev), ops.amax_one(dev))
            z0._rac_zero = True  # (as _ConvLSTM.init_hidden marks a rollout's initial state)
            h, c = cell(inp["x1"], (z0, z0))
            rule.check("frozen first step h", from_map(h), r64["first"]["h"], r32["first"]["h"])
            rule.check("frozen first step c", from_map(c), r64["first"]["c"], r32["first"]["c"])
        torch.cuda.synchronize()
    rule.done()


# --------------------------------------------------------------------------- 6. what the launchers refuse
def test_fused_cell_launchers_refuse_what_the_kernels_cannot_do(dev):
    """A width ops.norm_cell_frozen_ok rejects is refused by rac_norm_lstm_cell_fwd and rac_norm_lstm_cell_bwd in their
    host-side argument check (the package's error; the outputs keep their fill), and the predicate and both launchers agree
    on every g in 16 .. 4096 step 16 (an admitted width is launched on one pixel of one image)."""
    from robot_aware_control_amd import ops
    from robot_aware_control_amd._lib import RacError, call, ptr, stream_ptr

    def launch(g, B, HW):
        z = lambda *s: torch.zeros(s, device=dev)
        fill = lambda *s: torch.full(s, 7.0, device=dev)
        g_ih, g_hh, c_prev = z(B, HW, 4 * g), z(B, HW, 4 * g), z(B, HW, g)
        gam4, bet4, gam1, bet1 = torch.ones(4 * g, device=dev), z(4 * g), torch.ones(g, device=dev), z(g)
        h, c, act, c_raw, stats = fill(B, HW, g), fill(B, HW, g), fill(B, HW, 4 * g), fill(B, HW, g), fill(3, 2, B, 16)
        res = {}
        try:
            call("rac_norm_lstm_cell_fwd", ptr(g_ih), ptr(g_hh), ptr(c_prev), ptr(gam4), ptr(bet4), ptr(gam4), ptr(bet4),
                 ptr(gam1), ptr(bet1), ptr(h), ptr(c), ptr(act), ptr(c_raw), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]),
                 B, HW, g, 1e-5, stream_ptr())
            res["fwd"] = True
        except RacError as e:
            assert "rac_norm_lstm_cell_fwd" in str(e)
            res["fwd"] = False
        torch.cuda.synchronize()
        if not res["fwd"]:
            assert all(bool((t == 7.0).all()) for t in (h, c, act, c_raw, stats)), g
            act, c_raw, c = z(B, HW, 4 * g), z(B, HW, g), z(B, HW, g)
            stats = torch.ones(3, 2, B, 16, device=dev)
        dg_ih, dg_hh, dcp = fill(B, HW, 4 * g), fill(B, HW, 4 * g), fill(B, HW, g)
        dh, dc = z(B, HW, g), z(B, HW, g)
        slots = torch.zeros(2, device=dev, dtype=torch.int32)
        try:
            call("rac_norm_lstm_cell_bwd", ptr(dh), ptr(dc), ptr(act), ptr(c), ptr(c_raw), ptr(c_prev), ptr(g_ih), ptr(g_hh),
                 ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(gam4), ptr(gam4), ptr(gam1), ptr(dg_ih), ptr(dg_hh),
                 ptr(dcp), None, None, None, None, None, None, ptr(slots[0:1]), ptr(slots[1:2]), B, HW, g, stream_ptr())
            res["bwd"] = True
        except RacError as e:
            assert "rac_norm_lstm_cell_bwd" in str(e)
            res["bwd"] = False
        torch.cuda.synchronize()
        if not res["bwd"]:
            assert all(bool((t == 7.0).all()) for t in (dg_ih, dg_hh, dcp)), g
        return res

    for g in (16, 32, 48, 96):
        if not ops.norm_cell_frozen_ok(g):
            assert launch(g, 2, 8) == {"fwd": False, "bwd": False}, g
    for g in range(16, 4097, 16):
        ok = ops.norm_cell_frozen_ok(g)
        assert launch(g, 1, 1) == {"fwd": ok, "bwd": ok}, g
