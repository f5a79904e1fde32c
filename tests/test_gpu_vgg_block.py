"""The vgg block around its conv -- training-mode BatchNorm + LeakyReLU(0.2) forward and backward, the 2x2 max pool and the
nearest x2 upsample -- driven through the C ABI (include/rac_hip.h) and compared with tests/bn_refs.py (plain torch on the
CPU in fp64, itself checked against torch's operators and autograd in tests/test_bn_refs_host.py), in every launch form an
entry point picks by channel count, pointer alignment or size.

Pass rule (tests/fp64_tools.py): e_gpu <= max(2e-6, 4 * e_cpu32) for arithmetic results; torch.equal for copies, maxima and
routed gradients; a max |v| slot that starts at zero holds the bits of the kernel's own output's max |v|, one that starts
higher keeps its value.  Every case prints its figures; nothing is excluded: the inputs of the BatchNorm cases keep every
pre-activation 1e-2 away from the LeakyReLU's kink (bn_refs.make_inputs), so no kernel can rightly take the other slope.

Every output is a view inside a sentinel-filled buffer that must survive on both sides; `+=` outputs start non-zero; the row
groups have means 3 apart.  Each BatchNorm kernel is judged alone: its inputs (statistics, scale / shift / mean / invstd,
sums) come from the CPU, not from the kernel before it; only the chain test strings the kernels together.

Launch form reached, by case group (shape or alignment alone, never the environment):

  case group                                          form
  --------------------------------------------------  ---------------------------------------------------------------
  bn_finalize C 3 / 64 | 300                          bn_finalize_kernel, one | two workgroups; G 1 / 3, n_updates 0 / 1 / 2,
                                                      running statistics given / NULL, count 1, constant channels (var 0
                                                      or a residue of 1e-17: the same invstd with or without the clamp)
  affine_act vec_C8 / vec_C128 / wrap_C128            affine_act_kernel4 (16-byte); wrap_C128 (M 4200) with a slot wraps the
                                                      512-workgroup loop
  affine_act C6 / x_misaligned / y_misaligned /       affine_act_kernel1 (element-indexed): C % 4, x or y one float into its
             wrap_C128_misaligned                     allocation; the last (M 4200) without a slot wraps the 2048-workgroup loop
  bn_apply_act C 4 .. 1024                            bn_apply_act_rows_kernel: pass heights 256 .. 1 rows, ragged last row
                                                      block in every group; bit-equal to bn_finalize_kernel + affine_act_kernel4
  bn_apply_act C 96 / misaligned x, y / one pointer   refused in the host check (no launch)
  bn_bwd_reduce rows_C4 / rows_C64 | rows_C128 |      bn_bwd_reduce_rows_kernel: 1 | 2 | 16 channel slices; Mg 5 / 37 / 1030:
                rows_C1024                            less than one pass, ragged last pass, several row blocks
  bn_bwd_reduce elem_C6 / elem_C96 /                  bn_bwd_reduce_kernel (element-indexed): C not 4 * 2^k, dy one float into
                elem_C64_dy_misaligned                its allocation
  bn_bwd_apply rows_*                                 bn_bwd_apply_rows_kernel
  bn_bwd_apply elem_C6 / elem_C96 /                   bn_bwd_apply_kernel (element-indexed): C not 4 * 2^k, dy or dx one float
               elem_C64_dy_misaligned / _dx_          into its allocation
  bn_bwd_apply one of dgamma / dbeta                  refused in the host check (no launch)
  chain (3, 203, 64) / (1, 37, 1024)                  col_stats_kernel -> bn_apply_act_rows_kernel -> bn_bwd_reduce_rows_kernel
                                                      -> bn_bwd_apply_rows_kernel
  maxpool2_fwd vec_C8 / big_vec                       maxpool2_fwd_kernel<f32x4>; big_vec wraps the 2048-workgroup loop
  maxpool2_fwd C6 / x_, y_misaligned / big_scalar     maxpool2_fwd_kernel<float>; big_scalar wraps the 2048-workgroup loop
  maxpool2_fwd odd H / W                              refused in the host check (no launch)
  maxpool2_bwd (the same shapes)                      maxpool2_bwd_kernel (one form); the big cases wrap its loop
  upsample2 vec_C8 / big_vec                          upsample2_fwd_kernel<f32x4>, upsample2_bwd_kernel<f32x4>
  upsample2 C6 / in_, out_misaligned / big_scalar     upsample2_fwd_kernel<float>, upsample2_bwd_kernel<float>

The (1030, 1024, 3) case of the backward kernels runs in well under a second and is kept.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import bn_refs as br  # noqa: E402
from tests.fp64_tools import F32, F64, Rule, assert_intact, guarded, refused, rnd, slot_modes, sptr  # noqa: E402

EPS, MOM = float(np.float32(1e-5)), float(np.float32(0.1))  # as the C ABI's float arguments carry them
GROUPS = (1, 3)
SEED, TIE_SEED = 7, 601

# ---- case tables (tests/test_bn_refs_host.py imports them: make_inputs must converge on every one)
FINALIZE_C = (3, 64, 300)
FINALIZE_MG = (37, 1)
# name -> (C, rows per group at G = 1 and at G = 3, x lead, y lead); lead 1 = one float past 16-byte alignment
AFFINE_FORMS = {"vec_C8": (8, (37, 37), 0, 0), "vec_C128": (128, (37, 37), 0, 0), "C6": (6, (37, 37), 0, 0),
                "x_misaligned": (8, (37, 37), 1, 0), "y_misaligned": (8, (37, 37), 0, 1),
                "wrap_C128": (128, (4200, 1400), 0, 0), "wrap_C128_misaligned": (128, (4200, 1400), 1, 0)}
APPLY_ACT_C = (4, 8, 64, 256, 1024)
APPLY_ACT_MG = (37, 203)
BWD_MG = (5, 37, 1030)
# name -> (C, dy lead, dx lead)
BWD_REDUCE_FORMS = {"rows_C4": (4, 0, 0), "rows_C64": (64, 0, 0), "rows_C128": (128, 0, 0), "rows_C1024": (1024, 0, 0),
                    "elem_C6": (6, 0, 0), "elem_C96": (96, 0, 0), "elem_C64_dy_misaligned": (64, 1, 0)}
BWD_APPLY_FORMS = dict(BWD_REDUCE_FORMS, elem_C64_dx_misaligned=(64, 0, 1))
CHAIN_CASES = [(3, 203, 64), (1, 37, 1024)]  # (G, Mg, C)
# name -> (C, input lead, output lead); the big_ forms run the big maps
MAP_FORMS = {"vec_C8": (8, 0, 0), "C6": (6, 0, 0), "in_misaligned": (8, 1, 0), "out_misaligned": (8, 0, 1),
             "big_vec": (512, 0, 0), "big_scalar": (130, 0, 0)}
POOL_MAPS = {"small": [(3, 12, 16), (3, 2, 2)], "big": [(5, 64, 64)]}    # (B, H, W) of the pool's input
UPSAMPLE_MAPS = {"small": [(3, 3, 4), (3, 1, 1)], "big": [(5, 32, 32)]}  # (B, h, w) of the upsample's input


def bn_input_cases():
    """Every (G, Mg, C) this module asks bn_refs.make_inputs for."""
    cases = {(G, Mgs[GROUPS.index(G)], C) for C, Mgs, _, _ in AFFINE_FORMS.values() for G in GROUPS}
    cases |= {(G, Mg, C) for C in APPLY_ACT_C for Mg in APPLY_ACT_MG for G in GROUPS}
    cases |= {(G, Mg, C) for C, _, _ in BWD_APPLY_FORMS.values() for Mg in BWD_MG for G in GROUPS}
    return sorted(cases | set(CHAIN_CASES))


@functools.lru_cache(maxsize=None)
def inputs(G, Mg, C):
    """(x, dy, gamma, beta) of bn_refs.make_inputs, drawn once per shape and shared; nobody writes to them."""
    return br.make_inputs(SEED, G, Mg, C)


@functools.lru_cache(maxsize=None)
def aff32(G, Mg, C):
    """fp32 (scale, shift, mean, invstd) [G][C] of inputs(G, Mg, C): what rac_bn_finalize hands the other kernels."""
    x, _, gamma, beta = inputs(G, Mg, C)
    return br.finalize(br.stats_of(x, G), Mg, gamma, beta, None, None, 0.0, EPS, 0, G, F32)[:4]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rac(dev):
    """(ops, call, ptr, stream_ptr, RacError) of the package."""
    from robot_aware_control_amd import _lib, ops
    assert (ops.ACT_NONE, ops.ACT_LEAKY, ops.ACT_SIGMOID) == (br.ACT_NONE, br.ACT_LEAKY, br.ACT_SIGMOID)
    return ops, ops.call, ops.ptr, ops.stream_ptr, _lib.RacError


def put(dev, t, lead=0):
    """A CPU tensor on the device, `lead` floats past 16-byte alignment."""
    buf = torch.empty(t.numel() + lead, dtype=t.dtype, device=dev)
    view = buf[lead:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * lead) % 16 or t.dtype != F32
    return view


def check_rows(rule, what, got, r64, r32, names):
    """[G][k][C] under the rule, every [C] row held to its own largest value."""
    got = got.detach().cpu()
    assert got.shape == r64.shape, (what, tuple(got.shape), tuple(r64.shape))
    for g in range(got.shape[0]):
        for k, name in enumerate(names):
            rule.check(f"{what} group {g} {name}", got[g, k], r64[g, k], r32[g, k])


# =========================================================================== 1. rac_bn_finalize
def finalize_rows(G, Mg, C, const):
    """[G * Mg][C] rows, group k shifted by 3 k, per-channel spreads 0.5 .. 2; `const`: channels 1 and 2 hold 0.25 and 0.1
    (the first exact in the sums, so var = 0 to the bit; the second not, so var is a rounding residue of either sign)."""
    x = rnd(200 + C, G, Mg, C) * (0.5 + 1.5 * torch.arange(C, dtype=F32) / C) + 3.0 * torch.arange(G, dtype=F32).view(G, 1, 1)
    if const:
        x[:, :, 1], x[:, :, 2] = 0.25, 0.1
    return x.view(G * Mg, C)


@pytest.mark.parametrize("C", FINALIZE_C)
def test_bn_finalize_vs_fp64(dev, rac, C):
    """rac_bn_finalize from fp64 statistics summed on the CPU: scale, shift, mean, invstd [G][C] and the running statistics
    after n_updates = 0, 1, 2 updates per group in group order, from non-trivial starting values; running statistics NULL;
    count = 1 (var = 0, invstd = 1 / sqrt(eps), the unbiased variance is the biased one); constant channels, judged apart
    from the others (their invstd of 316 would otherwise hide the rest)."""
    ops, call, ptr, stream, _ = rac
    rule = Rule(f"v1 bn_finalize C{C}")
    gamma, beta = 1.0 + 0.3 * rnd(201, C), 0.3 * rnd(202, C)
    rm0, rv0 = rnd(203, C), 1.0 + 0.5 * rnd(204, C).abs()
    gamma_d, beta_d = put(dev, gamma), put(dev, beta)
    for G in GROUPS:
        for Mg, const in ((FINALIZE_MG[0], False), (FINALIZE_MG[0], True), (FINALIZE_MG[1], False)):
            x = finalize_rows(G, Mg, C, const)
            stats = br.stats_of(x, G)
            stats_d = put(dev, stats)
            parts = [("const", [1, 2]), ("rest", [0] + list(range(3, C)))] if const else [("all", list(range(C)))]
            for n_updates, running in ((0, True), (1, True), (2, True), (2, False)):
                what = f"G{G} Mg{Mg} const{int(const)} n_updates{n_updates} running{int(running)}"
                r64 = br.finalize(stats, Mg, gamma, beta, rm0 if running else None, rv0, MOM, EPS, n_updates, G, F64)
                r32 = br.finalize(stats, Mg, gamma, beta, rm0 if running else None, rv0, MOM, EPS, n_updates, G, F32)
                abuf, aff = guarded(dev, (4, G, C))
                rbuf, run = guarded(dev, (2, C), torch.stack([rm0, rv0]))
                call("rac_bn_finalize", ptr(stats_d), Mg, ptr(gamma_d), ptr(beta_d), ptr(run[0]) if running else None,
                     ptr(run[1]) if running else None, MOM, EPS, n_updates, ptr(aff[0]), ptr(aff[1]), ptr(aff[2]),
                     ptr(aff[3]), C, G, stream())
                torch.cuda.synchronize()
                for pname, cols in parts:
                    for k, name in enumerate(("scale", "shift", "mean", "invstd")):
                        rule.check(f"{what} {name} {pname}", aff[k][:, cols], r64[k][:, cols], r32[k][:, cols])
                    if running:
                        rule.check(f"{what} running_mean {pname}", run[0][cols], r64[4][cols], r32[4][cols])
                        rule.check(f"{what} running_var {pname}", run[1][cols], r64[5][cols], r32[5][cols])
                if not running or n_updates == 0:
                    assert torch.equal(run.cpu(), torch.stack([rm0, rv0])), f"{what}: running statistics changed"
                assert_intact(abuf, aff, what + " aff")
                assert_intact(rbuf, run, what + " running")
    rule.done()


# =========================================================================== 2. rac_affine_act
@pytest.mark.parametrize("form", list(AFFINE_FORMS))
def test_affine_act_vs_fp64(dev, rac, form):
    """rac_affine_act: y = act(x * scale[g] + shift[g]) for the three activations, G = 1 and 3 (a row that took its
    neighbouring group's scale shows: the groups' means are 3 apart), in the three slot modes."""
    ops, call, ptr, stream, _ = rac
    C, Mgs, x_lead, y_lead = AFFINE_FORMS[form]
    rule = Rule(f"v2 affine_act {form}")
    for G, Mg in zip(GROUPS, Mgs):
        x = inputs(G, Mg, C)[0]
        sc, sh, _, _ = aff32(G, Mg, C)
        x_d, sc_d, sh_d = put(dev, x, x_lead), put(dev, sc), put(dev, sh)
        for aname, act in (("none", br.ACT_NONE), ("leaky", br.ACT_LEAKY), ("sigmoid", br.ACT_SIGMOID)):
            r64, r32 = br.affine_act(x, sc, sh, act, G, F64), br.affine_act(x, sc, sh, act, G, F32)
            for sname, slot in slot_modes(ops, dev):
                what = f"G{G} {aname} {sname}"
                ybuf, y = guarded(dev, (G * Mg, C), lead=y_lead)
                call("rac_affine_act", ptr(x_d), ptr(sc_d), ptr(sh_d), act, ptr(y), G * Mg, C, G, sptr(slot), stream())
                torch.cuda.synchronize()
                rule.check(what, y, r64, r32)
                assert_intact(ybuf, y, what)
                if slot is not None:
                    slot.check(y, what)
    rule.done()


# =========================================================================== 3. rac_bn_apply_act
@pytest.mark.parametrize("C", APPLY_ACT_C)
def test_bn_apply_act_vs_fp64_and_two_launches(dev, rac, C):
    """rac_bn_apply_act (n_updates 2) at row counts that are no multiple of the pass height 1024 / C: the map, scale / shift /
    mean / invstd, the running statistics and the slot are the bits of rac_bn_finalize + rac_affine_act, and within the rule
    of the fp64 chain from the statistics."""
    ops, call, ptr, stream, _ = rac
    rule = Rule(f"v3 bn_apply_act C{C}")
    for Mg in APPLY_ACT_MG:
        for G in GROUPS:
            M = G * Mg
            x, _, gamma, beta = inputs(G, Mg, C)
            rm0, rv0 = rnd(301, C), 1.0 + 0.5 * rnd(302, C).abs()
            stats = br.stats_of(x, G)
            x_d, stats_d, gamma_d, beta_d = put(dev, x), put(dev, stats), put(dev, gamma), put(dev, beta)
            r64 = br.finalize(stats, Mg, gamma, beta, rm0, rv0, MOM, EPS, 2, G, F64)
            r32 = br.finalize(stats, Mg, gamma, beta, rm0, rv0, MOM, EPS, 2, G, F32)
            y64, y32 = br.affine_act(x, r64[0], r64[1], br.ACT_LEAKY, G, F64), br.affine_act(x, r32[0], r32[1], br.ACT_LEAKY, G, F32)
            for (sname, slot), (_, slot2) in zip(slot_modes(ops, dev), slot_modes(ops, dev)):
                what = f"Mg{Mg} G{G} {sname}"
                abuf, aff = guarded(dev, (4, G, C))
                rbuf, run = guarded(dev, (2, C), torch.stack([rm0, rv0]))
                ybuf, y = guarded(dev, (M, C))
                call("rac_bn_apply_act", ptr(stats_d), Mg, ptr(gamma_d), ptr(beta_d), ptr(run[0]), ptr(run[1]), MOM, EPS, 2,
                     ptr(x_d), br.ACT_LEAKY, ptr(y), ptr(aff[0]), ptr(aff[1]), ptr(aff[2]), ptr(aff[3]), M, C, G, sptr(slot),
                     stream())
                abuf2, aff2 = guarded(dev, (4, G, C))
                rbuf2, run2 = guarded(dev, (2, C), torch.stack([rm0, rv0]))
                ybuf2, y2 = guarded(dev, (M, C))
                call("rac_bn_finalize", ptr(stats_d), Mg, ptr(gamma_d), ptr(beta_d), ptr(run2[0]), ptr(run2[1]), MOM, EPS, 2,
                     ptr(aff2[0]), ptr(aff2[1]), ptr(aff2[2]), ptr(aff2[3]), C, G, stream())
                call("rac_affine_act", ptr(x_d), ptr(aff2[0]), ptr(aff2[1]), br.ACT_LEAKY, ptr(y2), M, C, G, sptr(slot2), stream())
                torch.cuda.synchronize()
                assert torch.equal(y, y2), f"{what}: other bits than rac_bn_finalize + rac_affine_act"
                assert torch.equal(aff, aff2), f"{what}: scale / shift / mean / invstd differ from rac_bn_finalize's"
                assert torch.equal(run, run2), f"{what}: running statistics differ from rac_bn_finalize's"
                rule.check(f"{what} y", y, y64, y32)
                for k, name in enumerate(("scale", "shift", "mean", "invstd", "running_mean", "running_var")):
                    rule.check(f"{what} {name}", aff[k] if k < 4 else run[k - 4], r64[k], r32[k])
                for buf, view, name in ((abuf, aff, "aff"), (rbuf, run, "running"), (ybuf, y, "y"), (abuf2, aff2, "aff2"),
                                        (rbuf2, run2, "running2"), (ybuf2, y2, "y2")):
                    assert_intact(buf, view, f"{what} {name}")
                if slot is not None:
                    slot.check(y, what)
                    slot2.check(y2, what + " two launches")
                    assert torch.equal(slot.three, slot2.three), what
    rule.done()


def test_bn_apply_act_refuses_what_it_cannot_do(dev, rac):
    """C = 96 (not 4 * 2^k), x or y one float into its allocation, and one running pointer without the other are refused in
    the host check, without a launch; nothing is written."""
    ops, call, ptr, stream, RacError = rac
    rows = "C must be 4 * 2^k"
    for C, x_lead, y_lead, rmean, rvar, message in ((96, 0, 0, 1, 1, rows), (64, 1, 0, 1, 1, rows), (64, 0, 1, 1, 1, rows),
                                                    (64, 0, 0, 1, 0, "rac_bn_apply_act: bad args"),
                                                    (64, 0, 0, 0, 1, "rac_bn_apply_act: bad args")):
        M = 48
        x_d = put(dev, rnd(310, M, C), x_lead)
        stats_d, gamma_d, beta_d = put(dev, br.stats_of(x_d.cpu(), 1)), put(dev, torch.ones(C)), put(dev, torch.zeros(C))
        abuf, aff = guarded(dev, (4, 1, C), 7.0)
        rbuf, run = guarded(dev, (2, C), 7.0)
        ybuf, y = guarded(dev, (M, C), 7.0, lead=y_lead)
        refused(RacError, lambda: call("rac_bn_apply_act", ptr(stats_d), M, ptr(gamma_d), ptr(beta_d),
                                       ptr(run[0]) if rmean else None, ptr(run[1]) if rvar else None, MOM, EPS, 2, ptr(x_d),
                                       br.ACT_LEAKY, ptr(y), ptr(aff[0]), ptr(aff[1]), ptr(aff[2]), ptr(aff[3]), M, C, 1, None,
                                       stream()), message)
        for buf, view, name in ((abuf, aff, "aff"), (rbuf, run, "running"), (ybuf, y, "y")):
            assert bool((view == 7.0).all()), (C, x_lead, y_lead, rmean, rvar, name)
            assert_intact(buf, view, name)


# =========================================================================== 4. rac_bn_bwd_reduce / rac_bn_bwd_apply
@pytest.mark.parametrize("form", list(BWD_REDUCE_FORMS))
def test_bn_bwd_reduce_vs_fp64(dev, rac, form):
    """rac_bn_bwd_reduce into zeroed sums [G][2][C]: (sum dz, sum dz * xhat) of every group on its own, against the fp64 sums
    over the same fp32 scale / shift / mean / invstd; the fp32 side adds the rows in index order."""
    ops, call, ptr, stream, _ = rac
    C, dy_lead, _ = BWD_REDUCE_FORMS[form]
    rule = Rule(f"v4 bn_bwd_reduce {form}")
    for Mg in BWD_MG:
        for G in GROUPS:
            what = f"Mg{Mg} G{G}"
            x, dy, _, _ = inputs(G, Mg, C)
            aff = aff32(G, Mg, C)
            r64, r32 = br.bwd_sums(dy, x, *aff, G, F64), br.bwd_sums(dy, x, *aff, G, F32)
            x_d, dy_d = put(dev, x), put(dev, dy, dy_lead)
            aff_d = [put(dev, a) for a in aff]
            sbuf, sums = guarded(dev, (G, 2, C), 0.0, dtype=F64)
            call("rac_bn_bwd_reduce", ptr(dy_d), ptr(x_d), *(ptr(a) for a in aff_d), ptr(sums), G * Mg, C, G, stream())
            torch.cuda.synchronize()
            check_rows(rule, what, sums, r64, r32, ("sum dz", "sum dz xhat"))
            assert_intact(sbuf, sums, what)
    rule.done()


@pytest.mark.parametrize("form", list(BWD_APPLY_FORMS))
def test_bn_bwd_apply_vs_fp64(dev, rac, form):
    """rac_bn_bwd_apply with the fp64 reference's sums: dx with dgamma / dbeta given (non-zero on entry: the kernel adds) and
    as a NULL pair (dx the same bits), each in the three slot modes."""
    ops, call, ptr, stream, _ = rac
    C, dy_lead, dx_lead = BWD_APPLY_FORMS[form]
    rule = Rule(f"v4 bn_bwd_apply {form}")
    dg0, db0 = rnd(401, C) * 5.0, rnd(402, C) * 5.0
    for Mg in BWD_MG:
        for G in GROUPS:
            M = G * Mg
            x, dy, _, _ = inputs(G, Mg, C)
            aff = aff32(G, Mg, C)
            sums = br.bwd_sums(dy, x, *aff, G, F64)
            r64 = br.bwd_apply(dy, x, *aff, sums, G, dg0, db0, F64)
            r32 = br.bwd_apply(dy, x, *aff, sums, G, dg0, db0, F32)
            x_d, dy_d, sums_d = put(dev, x), put(dev, dy, dy_lead), put(dev, sums)
            aff_d = [put(dev, a) for a in aff]
            with_pair = None
            for (sname, slot_pair), (_, slot_null) in zip(slot_modes(ops, dev), slot_modes(ops, dev)):
                for pair, slot in ((True, slot_pair), (False, slot_null)):
                    what = f"Mg{Mg} G{G} {sname} pair{int(pair)}"
                    xbuf, dx = guarded(dev, (M, C), lead=dx_lead)
                    gbuf, dgb = guarded(dev, (2, C), torch.stack([dg0, db0]))
                    call("rac_bn_bwd_apply", ptr(dy_d), ptr(x_d), *(ptr(a) for a in aff_d), ptr(sums_d), ptr(dx),
                         ptr(dgb[0]) if pair else None, ptr(dgb[1]) if pair else None, M, C, G, sptr(slot), stream())
                    torch.cuda.synchronize()
                    rule.check(f"{what} dx", dx, r64[0], r32[0])
                    if slot is not None:
                        slot.check(dx, what)
                    if pair:
                        rule.check(f"{what} dgamma", dgb[0], r64[1], r32[1])
                        rule.check(f"{what} dbeta", dgb[1], r64[2], r32[2])
                        with_pair = dx
                    else:
                        assert torch.equal(dgb.cpu(), torch.stack([dg0, db0])), f"{what}: dgamma / dbeta written"
                        assert torch.equal(dx, with_pair), f"{what}: dx differs without dgamma / dbeta"
                    assert_intact(xbuf, dx, what + " dx")
                    assert_intact(gbuf, dgb, what + " dgamma/dbeta")
    rule.done()


def test_bn_bwd_apply_refuses_half_a_pair(dev, rac):
    """dgamma without dbeta, and dbeta without dgamma, are refused in the host check; nothing is written."""
    ops, call, ptr, stream, RacError = rac
    G, Mg, C = 1, 37, 64
    x, dy, _, _ = inputs(G, Mg, C)
    aff = aff32(G, Mg, C)
    x_d, dy_d, sums_d = put(dev, x), put(dev, dy), put(dev, br.bwd_sums(dy, x, *aff, G, F64))
    aff_d = [put(dev, a) for a in aff]
    for has_g, has_b in ((True, False), (False, True)):
        xbuf, dx = guarded(dev, (Mg, C), 7.0)
        gbuf, dgb = guarded(dev, (2, C), 7.0)
        refused(RacError, lambda: call("rac_bn_bwd_apply", ptr(dy_d), ptr(x_d), *(ptr(a) for a in aff_d), ptr(sums_d), ptr(dx),
                                       ptr(dgb[0]) if has_g else None, ptr(dgb[1]) if has_b else None, Mg, C, G, None,
                                       stream()), "dgamma/dbeta must come together")
        assert bool((dx == 7.0).all()) and bool((dgb == 7.0).all())
        assert_intact(xbuf, dx, "dx")
        assert_intact(gbuf, dgb, "dgamma/dbeta")


# =========================================================================== 5. the chain
@pytest.mark.parametrize("G,Mg,C", CHAIN_CASES)
def test_bn_chain_vs_fp64_autograd(dev, rac, G, Mg, C):
    """rac_col_stats -> rac_bn_apply_act -> rac_bn_bwd_reduce -> rac_bn_bwd_apply, every kernel fed by the one before it,
    against F.batch_norm(training) + F.leaky_relu(0.2) per group and their autograd in fp64: y, dx, dgamma, dbeta and the
    running statistics after two updates per group.  The fp32 side takes its statistics in rac_col_stats' own order
    (bn_refs.stats_of: fp32 inside a block of 16 or 13 rows, fp64 across the blocks): with a group mean of 6 over a spread of
    0.5 that, not the BatchNorm kernels behind it, sets the chain's error (2e-6 to 3e-6 at (3, 203, 64))."""
    ops, call, ptr, stream, _ = rac
    rule = Rule(f"v5 chain G{G} Mg{Mg} C{C}")
    M = G * Mg
    x, dy, gamma, beta = inputs(G, Mg, C)
    rm0, rv0 = rnd(501, C), 1.0 + 0.5 * rnd(502, C).abs()
    rm64, rv64 = rm0.double().clone(), rv0.double().clone()
    r64 = br.autograd_chain(x, dy, gamma, beta, G, EPS, rm64, rv64, MOM, 2) + (rm64, rv64)
    r32 = br.chain(x, dy, gamma, beta, G, EPS, F32) + br.finalize(br.stats_of(x, G, F32), Mg, gamma, beta, rm0, rv0, MOM, EPS, 2,
                                                                  G, F32)[4:]
    x_d, dy_d, gamma_d, beta_d = put(dev, x), put(dev, dy), put(dev, gamma), put(dev, beta)
    stbuf, stats = guarded(dev, (G, 2, C), 0.0, dtype=F64)
    sbuf, sums = guarded(dev, (G, 2, C), 0.0, dtype=F64)
    abuf, aff = guarded(dev, (4, G, C))
    rbuf, run = guarded(dev, (2, C), torch.stack([rm0, rv0]))
    ybuf, y = guarded(dev, (M, C))
    xbuf, dx = guarded(dev, (M, C))
    gbuf, dgb = guarded(dev, (2, C), 0.0)
    affp = [ptr(aff[k]) for k in range(4)]
    call("rac_col_stats", ptr(x_d), ptr(stats), M, C, G, stream())
    call("rac_bn_apply_act", ptr(stats), Mg, ptr(gamma_d), ptr(beta_d), ptr(run[0]), ptr(run[1]), MOM, EPS, 2, ptr(x_d),
         br.ACT_LEAKY, ptr(y), *affp, M, C, G, None, stream())
    call("rac_bn_bwd_reduce", ptr(dy_d), ptr(x_d), *affp, ptr(sums), M, C, G, stream())
    call("rac_bn_bwd_apply", ptr(dy_d), ptr(x_d), *affp, ptr(sums), ptr(dx), ptr(dgb[0]), ptr(dgb[1]), M, C, G, None, stream())
    torch.cuda.synchronize()
    for k, (name, got) in enumerate((("y", y), ("dx", dx), ("dgamma", dgb[0]), ("dbeta", dgb[1]), ("running_mean", run[0]),
                                     ("running_var", run[1]))):
        rule.check(name, got, r64[k], r32[k])
    for buf, view, name in ((stbuf, stats, "stats"), (sbuf, sums, "sums"), (abuf, aff, "aff"), (rbuf, run, "running"),
                            (ybuf, y, "y"), (xbuf, dx, "dx"), (gbuf, dgb, "dgamma/dbeta")):
        assert_intact(buf, view, name)
    rule.done()


# =========================================================================== 6. max pool and upsample
def map_cases(form, table):
    return table["big" if form.startswith("big") else "small"]


@pytest.mark.parametrize("form", list(MAP_FORMS))
def test_maxpool2_fwd_and_bwd(dev, rac, form):
    """rac_maxpool2_fwd equals the window maximum, and rac_maxpool2_bwd (dx starts NaN: every element is written) equals the
    fp64 autograd gradient of F.max_pool2d, on continuous maps and on maps of {-1, 0, 1}, where the gradient must go to the
    FIRST maximum in scan order."""
    ops, call, ptr, stream, _ = rac
    C, in_lead, out_lead = MAP_FORMS[form]
    for B, H, W in map_cases(form, POOL_MAPS):
        for kind, x in (("continuous", rnd(600, B, H, W, C)), ("ties", br.tie_map(TIE_SEED, B, H, W, C))):
            what = f"{form} {B}x{H}x{W} {kind}"
            dy = rnd(602, B, H // 2, W // 2, C)
            y_ref, dx_ref = br.maxpool2_autograd(x, dy)
            x_d, dy_d = put(dev, x, in_lead), put(dev, dy, in_lead)
            ybuf, y = guarded(dev, (B, H // 2, W // 2, C), lead=out_lead)
            call("rac_maxpool2_fwd", ptr(x_d), ptr(y), B, H, W, C, stream())
            xbuf, dx = guarded(dev, (B, H, W, C), lead=out_lead)
            call("rac_maxpool2_bwd", ptr(x_d), ptr(dy_d), ptr(dx), B, H, W, C, stream())
            torch.cuda.synchronize()
            assert torch.equal(y.cpu(), br.maxpool2_fwd(x)) and torch.equal(y.cpu(), y_ref.float()), what + " y"
            assert torch.equal(dx.cpu(), dx_ref.float()), what + " dx"
            assert torch.equal(dx.cpu(), br.maxpool2_bwd(x, dy)), what + " dx (reference)"
            assert_intact(ybuf, y, what + " y")
            assert_intact(xbuf, dx, what + " dx")


def test_maxpool2_refuses_odd_maps(dev, rac):
    """An odd H or W is refused by both entry points in the host check; nothing is written."""
    ops, call, ptr, stream, RacError = rac
    for H, W in ((5, 4), (4, 5)):
        x_d, dy_d = put(dev, rnd(610, 2, H, W, 8)), put(dev, rnd(611, 2, H // 2, W // 2, 8))
        ybuf, y = guarded(dev, (2, H, W, 8), 7.0)
        refused(RacError, lambda: call("rac_maxpool2_fwd", ptr(x_d), ptr(y), 2, H, W, 8, stream()), "rac_maxpool2_fwd: bad args")
        refused(RacError, lambda: call("rac_maxpool2_bwd", ptr(x_d), ptr(dy_d), ptr(y), 2, H, W, 8, stream()),
                "rac_maxpool2_bwd: bad args")
        assert bool((y == 7.0).all())
        assert_intact(ybuf, y, "y")


@pytest.mark.parametrize("form", list(MAP_FORMS))
def test_upsample2_fwd_and_bwd(dev, rac, form):
    """rac_upsample2_fwd equals the nearest x2 copy; rac_upsample2_bwd is the sum of every 2x2 block under the rule, the fp32
    side in the kernel's association (p00 + p01) + (p10 + p11)."""
    ops, call, ptr, stream, _ = rac
    C, in_lead, out_lead = MAP_FORMS[form]
    rule = Rule(f"v6 upsample2_bwd {form}")
    for B, h, w in map_cases(form, UPSAMPLE_MAPS):
        what = f"{B}x{h}x{w}"
        x, dy = rnd(620, B, h, w, C), rnd(621, B, 2 * h, 2 * w, C)
        x_d, dy_d = put(dev, x, in_lead), put(dev, dy, in_lead)
        ybuf, y = guarded(dev, (B, 2 * h, 2 * w, C), lead=out_lead)
        call("rac_upsample2_fwd", ptr(x_d), ptr(y), B, h, w, C, stream())
        xbuf, dx = guarded(dev, (B, h, w, C), lead=out_lead)
        call("rac_upsample2_bwd", ptr(dy_d), ptr(dx), B, h, w, C, stream())
        torch.cuda.synchronize()
        assert torch.equal(y.cpu(), br.upsample2_fwd(x)), what + " y"
        rule.check(what + " dx", dx, br.upsample2_bwd(dy, F64), br.upsample2_bwd(dy, F32))
        assert_intact(ybuf, y, what + " y")
        assert_intact(xbuf, dx, what + " dx")
    rule.done()
