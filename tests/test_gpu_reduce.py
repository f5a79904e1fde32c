"""The reduction and routing kernels between the convolutions -- split-K combines, per-channel column sums, gradient maps
given as sums of sources, channel plumbing -- driven through the C ABI (include/rac_hip.h) and compared with torch on the
CPU in fp64, in every launch form an entry point picks by divisibility, pointer alignment or size.

Pass rule (tests/fp64_tools.py, the rule of test_gpu_norm_cell.py): e_gpu <= max(2e-6, 4 * e_cpu32) for arithmetic results;
torch.equal for pure copies; a max |v| slot that starts at zero holds the bits of the kernel's own output's max |v|, one that
starts higher keeps its value (the kernels fold with atomicMax).  Every case prints its figures; nothing is excluded.

Every output is a view inside a buffer filled with a sentinel that must survive on both sides (slots: the middle one of
three); gaps between slabs and the columns outside a source's window hold NaN; `+=` outputs start non-zero; the row groups of
a statistics call have means 3 apart.

Launch form reached, by case group (shape or alignment alone, never the environment):

  case group                                          form
  --------------------------------------------------  ---------------------------------------------------------------
  slab_reduce  vec64 / vec512                         slab_reduce_kernel4 (16-byte); vec512 wraps the 512-workgroup loop
  slab_reduce  N74 / stride / misaligned-out          slab_reduce_kernel (element-indexed): N % 4, slab_stride % 4, out one
                                                      float into its allocation; the last wraps the 2048-workgroup loop
  slab_reduce2 (32,16) (128,64) (192,64)              slab_reduce2_kernel4; (128,64) M 4200 wraps the 512-workgroup loop
  slab_reduce2 (138,10)                               slab_reduce2_kernel; M 3800 wraps the 2048-workgroup loop
  slab_reduce_stats C 4 .. 1024                       slab_reduce_stats_rows_kernel: 1 .. 16 channel slices, pass heights
                                                      256 .. 16 rows, ragged last row block in every group
  slab_reduce_stats C 96 / misaligned out             refused in the host check (no launch)
  slab_accumulate n_slabs 1, 63 | 64, 200             slab_accumulate_kernel | slab_accumulate_many_kernel
  col_stats                                           col_stats_kernel, 1 .. 8 channel groups, ragged last row block
  colsum_acc / colsum_steps, parts NULL | given       fp32 atomics | stored row-block sums + colsum_parts_add_kernel
  grad_sum / lstm_cell_bwd_srcs / reparam_head_bwd    one kernel each; sources: plain, 3 slabs, column window at 4-byte
                                                      alignment; grad_sum M 4200 / 16400 wrap the 512 / 2048 loops
  pad_rows, unpad_add, slice_channels, cat2_channels, one element-indexed kernel each; the large case of each wraps the
  act_bwd                                             2048-workgroup loop (cat2 with a slot: the 512-workgroup loop)
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.fp64_tools import (BIG, F32, F64, NAN, Rule, Slot, assert_intact, guarded, refused, rnd,  # noqa: E402
                               slot_modes, sptr)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rac(dev):
    """(ops, call, ptr, stream_ptr, GradSrc, RacError) of the package."""
    from robot_aware_control_amd import _lib, ops
    return ops, ops.call, ops.ptr, ops.stream_ptr, _lib.GradSrc, _lib.RacError


def slab_stack(dev, data, stride):
    """[S][n] CPU slabs -> one device buffer, slab s at s * stride, NaN in the gaps."""
    S, n = data.shape
    buf = torch.full((S * stride,), NAN, device=dev)
    buf.view(S, stride)[:, :n] = data.to(dev)
    return buf


def seq_sum(parts, start=None):
    """start + parts[0] + parts[1] + ... in the parts' own precision, in index order."""
    acc = parts[0].clone() if start is None else start + parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


# =========================================================================== 1. split-K combines
# (M, N, slab_stride - n, out one float into its allocation)
SLAB_REDUCE_FORMS = {"vec64": (48, 64, 64, 0), "vec512": (1030, 512, 64, 0), "N74": (48, 74, 64, 0),
                     "stride": (48, 64, 65, 0), "misaligned_out": (1030, 512, 64, 1)}


@pytest.mark.parametrize("form", list(SLAB_REDUCE_FORMS))
def test_slab_reduce_vs_fp64(dev, rac, form):
    """rac_slab_reduce: out[i] = sum_s slabs[s][i] + bias[i % N] against the fp64 sum, n_slabs 1 / 3 / 8, with and without
    bias and slot, in the 16-byte form and in the element-indexed form reached three ways."""
    ops, call, ptr, stream, _, _ = rac
    M, N, gap, lead = SLAB_REDUCE_FORMS[form]
    n = M * N
    rule = Rule(f"s1 slab_reduce {form}")
    bias = rnd(9, N)
    bbuf, bias_d = guarded(dev, (N,), bias)
    for S in (1, 3, 8):
        data = rnd(10 + S, S, n)
        slabs = slab_stack(dev, data, n + gap)
        for with_bias in (False, True):
            r64 = seq_sum(list(data.double())).view(M, N) + (bias.double() if with_bias else 0)
            r32 = seq_sum(list(data), bias.repeat(M) if with_bias else None).view(M, N)
            for sname, slot in slot_modes(ops, dev):
                what = f"S{S} bias{int(with_bias)} {sname}"
                obuf, out = guarded(dev, (M, N), lead=lead)
                call("rac_slab_reduce", ptr(slabs), S, n + gap, ptr(bias_d) if with_bias else None, ptr(out), n, N,
                     sptr(slot), stream())
                torch.cuda.synchronize()
                rule.check(what, out, r64, r32)
                assert_intact(obuf, out, what)
                if slot is not None:
                    slot.check(out, what)
    assert_intact(bbuf, bias_d, "bias")
    rule.done()


# (N, o_split) -> row counts
REDUCE2_CASES = {(32, 16): (37,), (128, 64): (37, 4200), (192, 64): (37,), (138, 10): (37, 3800)}


@pytest.mark.parametrize("N,o_split", list(REDUCE2_CASES), ids=lambda v: str(v))
def test_slab_reduce2_vs_fp64(dev, rac, N, o_split):
    """rac_slab_reduce2: columns [0, o_split) to out0 (row stride o_split), the rest to out1 (row stride N - o_split), with
    no slot, one on either output alone, both, and both pre-filled; the second half is three times as large as the first,
    so a slot that takes the other output's maximum cannot pass.  out1's guard is wide enough for any row stride up to N."""
    ops, call, ptr, stream, _, _ = rac
    rule = Rule(f"s1 slab_reduce2 N{N} o{o_split}")
    bias = rnd(9, N)
    bbuf, bias_d = guarded(dev, (N,), bias)
    for M in REDUCE2_CASES[(N, o_split)]:
        n, gap = M * N, 64 if N % 4 == 0 else 61
        for S in (1, 4):
            data = rnd(20 + S, S, M, N)
            data[:, :, o_split:] *= 3.0
            slabs = slab_stack(dev, data.view(S, n), n + gap)
            for with_bias in ((False, True) if M < 1000 else (True,)):
                r64 = seq_sum(list(data.double())) + (bias.double() if with_bias else 0)
                r32 = seq_sum(list(data), bias.expand(M, N) if with_bias else None)
                for sname in ("noslot", "slot0", "slot1", "both", "both_big"):
                    s0 = Slot(ops, dev, BIG if sname == "both_big" else 0) if sname in ("slot0", "both", "both_big") else None
                    s1 = Slot(ops, dev, BIG if sname == "both_big" else 0) if sname in ("slot1", "both", "both_big") else None
                    what = f"M{M} S{S} bias{int(with_bias)} {sname}"
                    b0, out0 = guarded(dev, (M, o_split), tail=M * N)
                    b1, out1 = guarded(dev, (M, N - o_split), tail=M * N)
                    call("rac_slab_reduce2", ptr(slabs), S, n + gap, ptr(bias_d) if with_bias else None, ptr(out0), ptr(out1),
                         M, N, o_split, sptr(s0), sptr(s1), stream())
                    torch.cuda.synchronize()
                    rule.check(f"{what} out0", out0, r64[:, :o_split], r32[:, :o_split])
                    rule.check(f"{what} out1", out1, r64[:, o_split:], r32[:, o_split:])
                    assert_intact(b0, out0, what + " out0")
                    assert_intact(b1, out1, what + " out1")
                    if s0 is not None:
                        s0.check(out0, what + " out0")
                    if s1 is not None:
                        s1.check(out1, what + " out1")
    assert_intact(bbuf, bias_d, "bias")
    rule.done()


STATS_SHAPES = [(100, 3), (144, 3), (40, 5), (333, 1), (1030, 1)]  # (rows per group, groups)


def grouped_rows(seed, Mg, G, C, kind="zero"):
    """[G * Mg][C] rows, group k shifted by 3 k; kind "offset": a per-channel offset of +-50 as well."""
    x = rnd(seed, G, Mg, C) + 3.0 * torch.arange(G, dtype=F32).view(G, 1, 1)
    if kind == "offset":
        x = x + (50.0 * (1 + 0.01 * torch.arange(C)) * (1 - 2 * (torch.arange(C) % 2))).to(F32).view(1, 1, C)
    return x.view(G * Mg, C)


def group_sums(x, G):
    """[G][2][C]: per-group column sums and sums of squares of [M][C] rows, in x's precision."""
    v = x.view(G, -1, x.shape[-1])
    return torch.stack([v.sum(1), (v * v).sum(1)], 1)


def check_stats(rule, what, got, r64, r32):
    """[G][2][C] statistics under the rule, every group's sums and sums of squares on their own: each [C] row is held to its
    own largest value, not to the largest sum of squares of the highest group."""
    got = got.detach().cpu()
    assert got.shape == r64.shape, (what, tuple(got.shape), tuple(r64.shape))
    for k in range(got.shape[0]):
        rule.check(f"{what} group {k} sum", got[k, 0], r64[k, 0], r32[k, 0])
        rule.check(f"{what} group {k} sum of squares", got[k, 1], r64[k, 1], r32[k, 1])


@pytest.mark.parametrize("C", [4, 32, 64, 512, 1024])
def test_slab_reduce_stats_vs_fp64_and_slab_reduce(dev, rac, C):
    """rac_slab_reduce_stats at row counts that are no multiple of the pass height 256 / min(C / 4, 16): `out` is the fp64
    sum of slabs under the rule and the same bits as rac_slab_reduce without bias (both add the slabs in index order);
    stats [G][2][C], every group's sums and sums of squares on their own, against the fp64 per-group sums of the fp64 sum
    of slabs, and against those of the map the kernel wrote (a reference that leans on the two assertions on `out` just
    before it: what it adds is that the statistics are those of the written values); rows taken from a neighbouring group
    (means 3 apart) show."""
    ops, call, ptr, stream, _, _ = rac
    rule = Rule(f"s1 slab_reduce_stats C{C}")
    for Mg, G in STATS_SHAPES:
        M = Mg * G
        n, gap = M * C, 64
        for S in (1, 4):
            data = rnd(30 + S, S, M, C)
            data[0] += (3.0 * torch.arange(G, dtype=F32)).repeat_interleave(Mg).view(M, 1)  # group k shifted by 3 k
            slabs = slab_stack(dev, data.view(S, n), n + gap)
            r64, r32 = seq_sum(list(data.double())), seq_sum(list(data))
            plain = torch.full((M, C), NAN, device=dev)
            call("rac_slab_reduce", ptr(slabs), S, n + gap, None, ptr(plain), n, C, None, stream())
            for sname, slot in slot_modes(ops, dev):
                what = f"Mg{Mg} G{G} S{S} {sname}"
                obuf, out = guarded(dev, (M, C))
                sbuf, stats = guarded(dev, (G, 2, C), 0.0, dtype=F64)
                call("rac_slab_reduce_stats", ptr(slabs), S, n + gap, ptr(out), ptr(stats), M, C, G, sptr(slot), stream())
                torch.cuda.synchronize()
                rule.check(f"{what} out", out, r64, r32)
                assert torch.equal(out, plain), f"{what}: other bits than rac_slab_reduce"
                o = out.cpu()
                check_stats(rule, f"{what} stats", stats, group_sums(r64, G), group_sums(r32, G))
                check_stats(rule, f"{what} stats of out", stats, group_sums(o.double(), G), group_sums(o, G))
                assert_intact(obuf, out, what + " out")
                assert_intact(sbuf, stats, what + " stats")
                if slot is not None:
                    slot.check(out, what)
    rule.done()


def test_slab_reduce_stats_refuses_what_it_cannot_do(dev, rac):
    """C = 96 (not 4 * 2^k) and an `out` one float into its allocation are refused in the host check, without a launch:
    "use rac_slab_reduce + rac_col_stats"."""
    ops, call, ptr, stream, _, RacError = rac
    for C, lead in ((96, 0), (64, 1)):
        M = 48
        slabs = torch.zeros(M * C, device=dev)
        obuf, out = guarded(dev, (M, C), 7.0, lead=lead)
        sbuf, stats = guarded(dev, (1, 2, C), 7.0, dtype=F64)
        refused(RacError, lambda: call("rac_slab_reduce_stats", ptr(slabs), 1, M * C, ptr(out), ptr(stats), M, C, 1, None,
                                       stream()), "C must be 4 * 2^k")
        assert bool((out == 7.0).all()) and bool((stats == 7.0).all()), (C, lead)
        assert_intact(obuf, out, "out")
        assert_intact(sbuf, stats, "stats")


@pytest.mark.parametrize("n", [4 * 37, 4 * 4096])
@pytest.mark.parametrize("S", [1, 63, 64, 200])
def test_slab_accumulate_vs_fp64(dev, rac, S, n):
    """rac_slab_accumulate: out[i] += sum_s slabs[s][i] onto a non-zero `out`, on both sides of the many-slabs switch
    (n_slabs >= 64), with n / 4 no multiple of that form's 16 columns per workgroup; n % 4 != 0 is refused."""
    ops, call, ptr, stream, _, RacError = rac
    rule = Rule(f"s1 slab_accumulate S{S} n{n}")
    data, start = rnd(40, S, n), rnd(41, n)
    slabs = slab_stack(dev, data, n + 64)
    obuf, out = guarded(dev, (n,), start)
    call("rac_slab_accumulate", ptr(slabs), S, n + 64, ptr(out), n, stream())
    torch.cuda.synchronize()
    rule.check("out", out, seq_sum(list(data.double()), start.double()), seq_sum(list(data), start))
    assert_intact(obuf, out, "out")
    obuf, out = guarded(dev, (n + 2,), 7.0)
    refused(RacError, lambda: call("rac_slab_accumulate", ptr(slabs), S, n + 64, ptr(out), n + 2, stream()),
            "rac_slab_accumulate: alignment")
    assert bool((out == 7.0).all())
    assert_intact(obuf, out, "refused out")
    rule.done()


# =========================================================================== 2. column reductions
COL_STATS_SHAPES = [(100, 4, 3), (100, 96, 3), (144, 64, 3), (7, 20, 2), (40, 512, 5), (4100, 64, 1)]  # (Mg, C, groups)


@pytest.mark.parametrize("kind", ["zero", "offset"])
@pytest.mark.parametrize("Mg,C,G", COL_STATS_SHAPES)
def test_col_stats_vs_fp64(dev, rac, Mg, C, G, kind):
    """rac_col_stats: stats [G][2][C] (fp64) against the fp64 per-group sums of zero-mean rows and of rows with a +-50
    per-channel offset, every group's sums and sums of squares on their own; and, where C = 4 * 2^k, against
    rac_slab_reduce_stats of the same rows under the same rule."""
    ops, call, ptr, stream, _, _ = rac
    rule = Rule(f"s2 col_stats Mg{Mg} C{C} G{G} {kind}")
    x = grouped_rows(50, Mg, G, C, kind)
    x_d = x.to(dev)
    r64, r32 = group_sums(x.double(), G), group_sums(x, G)
    sbuf, stats = guarded(dev, (G, 2, C), 0.0, dtype=F64)
    call("rac_col_stats", ptr(x_d), ptr(stats), G * Mg, C, G, stream())
    torch.cuda.synchronize()
    check_stats(rule, "stats", stats, r64, r32)
    assert_intact(sbuf, stats, "stats")
    if (C & (C - 1)) == 0:
        out = torch.empty_like(x_d)
        sbuf2, stats2 = guarded(dev, (G, 2, C), 0.0, dtype=F64)
        call("rac_slab_reduce_stats", ptr(x_d), 1, G * Mg * C, ptr(out), ptr(stats2), G * Mg, C, G, None, stream())
        torch.cuda.synchronize()
        assert torch.equal(out, x_d)
        check_stats(rule, "stats of slab_reduce_stats", stats2, r64, r32)
        check_stats(rule, "stats vs slab_reduce_stats", stats, stats2.cpu(), r32)
        assert_intact(sbuf2, stats2, "stats2")
    rule.done()


COLSUM_CASES = [(5, 16, (1, 5, 16)), (130, 74, (1, 5, 16)), (1000, 2048, (1, 5, 16)), (48, 256, (1, 5, 16))]  # (M, C, T list)


@pytest.mark.parametrize("M,C,Ts", COLSUM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_colsum_acc_and_steps_vs_fp64(dev, rac, M, C, Ts):
    """rac_colsum_acc and rac_colsum_steps (T = 1, 5, 16) onto a non-zero `out`: the fp32-atomic form (parts NULL) under the
    rule; with `parts` (sized exactly rac_colsum_blocks(M, C) * C, guarded) under the rule and bit-reproducible over two
    runs; rac_colsum_steps with T = 1 gives rac_colsum_acc's bits; T = 17 is refused."""
    ops, call, ptr, stream, _, RacError = rac
    from robot_aware_control_amd import _lib
    rule = Rule(f"s2 colsum M{M} C{C}")
    start = rnd(60, C) * 5.0
    xs = [rnd(61 + t, M, C) + 0.25 for t in range(max(Ts))]
    xs_d = [x.to(dev) for x in xs]
    nblk = int(_lib.load().rac_colsum_blocks(M, C))
    assert 1 <= nblk <= 1024

    def steps_arr(T):
        arr = (ctypes.c_void_p * T)()
        for t in range(T):
            arr[t] = xs_d[t].data_ptr()
        return arr

    def run(T, with_parts, acc):
        obuf, out = guarded(dev, (C,), start)
        pbuf, parts = guarded(dev, (nblk, C)) if with_parts else (None, None)
        if acc:
            call("rac_colsum_acc", ptr(xs_d[0]), ptr(out), ptr(parts), M, C, stream())
        else:
            call("rac_colsum_steps", steps_arr(T), T, ptr(out), ptr(parts), M, C, stream())
        torch.cuda.synchronize()
        assert_intact(obuf, out, "out")
        if with_parts:
            assert_intact(pbuf, parts, "parts")
            assert bool(torch.isfinite(parts).all()), "a row block's sums were not stored"
        return out

    def ref(T, dt):
        return seq_sum([x.to(dt).sum(0) for x in xs[:T]], start.to(dt))

    acc_bits = None
    for with_parts in (False, True):
        tag = "parts" if with_parts else "atomics"
        out = run(1, with_parts, True)
        rule.check(f"acc {tag}", out, ref(1, F64), ref(1, F32))
        if with_parts:
            acc_bits = out
            assert torch.equal(run(1, True, True), out), "rac_colsum_acc with parts: two runs, other bits"
        for T in Ts:
            out = run(T, with_parts, False)
            rule.check(f"steps T{T} {tag}", out, ref(T, F64), ref(T, F32))
            if with_parts:
                assert torch.equal(run(T, True, False), out), f"rac_colsum_steps T{T} with parts: two runs, other bits"
                if T == 1:
                    assert torch.equal(out, acc_bits), "rac_colsum_steps T1 != rac_colsum_acc in bits"
    obuf, out = guarded(dev, (C,), 7.0)
    big = (ctypes.c_void_p * 17)(*([xs_d[0].data_ptr()] * 17))
    refused(RacError, lambda: call("rac_colsum_steps", big, 17, ptr(out), None, M, C, stream()), "rac_colsum_steps: bad args")
    assert bool((out == 7.0).all())
    assert_intact(obuf, out, "refused out")
    rule.done()


# =========================================================================== 3. gradient maps as sums of sources
SRC_COMBOS = [("plain",), ("slabs",), ("window",), ("plain", "window"), ("plain", "slabs", "window")]


class Sources:
    """Gradient sources of an [M][C] map: `plain` [M][C]; `slabs` three K-split slabs, slab_stride > M * row_stride, NaN in
    the gaps; `window` columns [10, 10 + C) of rows of max(138, C + 14) floats, NaN outside the window (the 16-byte loads
    start at 4-byte alignment).  .total(dt) is their sum in precision dt, sources and slabs in index order."""

    def __init__(self, GradSrc, dev, kinds, M, C, seed=70):
        self.keep, self.terms, self.arr = [], [], (GradSrc * max(1, len(kinds)))()
        for i, kind in enumerate(kinds):
            if kind == "plain":
                v = rnd(seed + i, 1, M, C)
                t, n_slabs, slab_stride, row, col = v.to(dev), 1, M * C, C, 0
            elif kind == "slabs":
                v = rnd(seed + i, 3, M, C)
                slab_stride = M * C + 20
                t, n_slabs, row, col = slab_stack(dev, v.view(3, M * C), slab_stride), 3, C, 0
            else:
                v = rnd(seed + i, 1, M, C)
                row, col = max(138, C + 14), 10
                t = torch.full((M, row), NAN, device=dev)
                t[:, col:col + C] = v[0].to(dev)
                n_slabs, slab_stride = 1, M * row
            self.keep.append(t)
            self.terms.extend(v)
            self.arr[i] = GradSrc(p=t.data_ptr(), slab_stride=slab_stride, n_slabs=n_slabs, row_stride=row, col_off=col,
                                  reserved=0)
        self.n = len(kinds)

    def total(self, dt):
        return seq_sum([t.to(dt) for t in self.terms])


GRAD_SUM_CASES = [(C, M) for C in (4, 64, 128) for M in (3, 320, 2100)] + [(128, 4200), (128, 16400)]


@pytest.mark.parametrize("C,M", GRAD_SUM_CASES)
def test_grad_sum_vs_fp64(dev, rac, C, M):
    """rac_grad_sum over 1, 2 and 3 sources of the three kinds, slot given and NULL; M = 4200 wraps the 512-workgroup loop
    of the slot form, M = 16400 (plain source, no slot) the 2048-workgroup loop."""
    ops, call, ptr, stream, GradSrc, _ = rac
    rule = Rule(f"s3 grad_sum C{C} M{M}")
    combos = SRC_COMBOS if M < 16000 else [("plain",)]
    for kinds in combos:
        src = Sources(GradSrc, dev, kinds, M, C)
        r64, r32 = src.total(F64), src.total(F32)
        for sname, slot in slot_modes(ops, dev) if M < 16000 else (("noslot", None),):
            what = f"{'+'.join(kinds)} {sname}"
            obuf, out = guarded(dev, (M, C))
            call("rac_grad_sum", src.arr, src.n, ptr(out), M, C, sptr(slot), stream())
            torch.cuda.synchronize()
            rule.check(what, out, r64, r32)
            assert_intact(obuf, out, what)
            if slot is not None:
                slot.check(out, what)
    rule.done()


def test_grad_sum_refuses_bad_windows(dev, rac):
    """C % 4 != 0 (the entry point's argument check) and a window that leaves its row (row_stride < col_off + C: the sources'
    own check) are refused without a launch, each by the check meant for it."""
    ops, call, ptr, stream, GradSrc, RacError = rac
    M = 5
    t = torch.zeros(M, 138, device=dev)
    obuf, out = guarded(dev, (M, 64), 7.0)
    for C, row, col, message in ((6, 138, 10, "rac_grad_sum: bad args"), (64, 70, 10, "source 0 out of its rows")):
        arr = (GradSrc * 1)(GradSrc(p=t.data_ptr(), slab_stride=M * row, n_slabs=1, row_stride=row, col_off=col, reserved=0))
        refused(RacError, lambda: call("rac_grad_sum", arr, 1, ptr(out), M, C, None, stream()), message)
        assert bool((out == 7.0).all())
    assert_intact(obuf, out, "out")


def lstm_bwd_ref(pre, c_prev, dh, dc_next, dt):
    """(dgates [M][4g], dc_prev [M][g]) by autograd through the header's cell formulas in precision dt; gate order i, f, o, g~."""
    p, cp = pre.to(dt).clone().requires_grad_(True), c_prev.to(dt).clone().requires_grad_(True)
    i_, f_, o_, g_ = p.chunk(4, 1)
    c = torch.sigmoid(f_) * cp + torch.sigmoid(i_) * torch.tanh(g_)
    h = torch.sigmoid(o_) * torch.tanh(c)
    loss = (h * dh.to(dt)).sum() + (c * dc_next.to(dt)).sum()
    return torch.autograd.grad(loss, [p, cp])


@pytest.mark.parametrize("M", [3, 128])
@pytest.mark.parametrize("g", [12, 64, 512])
def test_lstm_cell_bwd_srcs_vs_fp64(dev, rac, g, M):
    """rac_lstm_cell_bwd_srcs (dh = sum of sources) against fp64 autograd from the gate pre-activations, the kernel's
    activations and cell taken from the fp32 forward pass on the CPU at the same point: dgates, dc_prev and the slot, with
    n_srcs = 0 and dc_next, with sources and dc_next NULL, and with both; then against rac_lstm_cell_bwd fed the
    rac_grad_sum of the same sources, under the same rule."""
    ops, call, ptr, stream, GradSrc, _ = rac
    rule = Rule(f"s3 lstm_cell_bwd_srcs g{g} M{M}")
    pre, c_prev, dcn = rnd(80, M, 4 * g) * 1.5, rnd(81, M, g), rnd(82, M, g)
    i_, f_, o_, g_ = pre.chunk(4, 1)
    act = torch.cat([torch.sigmoid(i_), torch.sigmoid(f_), torch.sigmoid(o_), torch.tanh(g_)], 1)
    c_new = act[:, g:2 * g] * c_prev + act[:, :g] * act[:, 3 * g:]
    act_d, cp_d, cn_d, dcn_d = act.to(dev), c_prev.to(dev), c_new.to(dev), dcn.to(dev)
    zero = torch.zeros(M, g)
    modes = [((), True)] + [(k, d) for k in (("window",), ("plain", "slabs", "window")) for d in (False, True)]
    for kinds, with_dc in modes:
        src = Sources(GradSrc, dev, kinds, M, g)
        dh64, dh32 = (src.total(F64), src.total(F32)) if kinds else (zero.double(), zero)
        r64 = lstm_bwd_ref(pre, c_prev, dh64, dcn if with_dc else zero, F64)
        r32 = lstm_bwd_ref(pre, c_prev, dh32, dcn if with_dc else zero, F32)
        dh_d = None
        if kinds:
            dh_d = torch.empty(M, g, device=dev)
            call("rac_grad_sum", src.arr, src.n, ptr(dh_d), M, g, None, stream())
        dg2, dcp2 = torch.full((M, 4 * g), NAN, device=dev), torch.full((M, g), NAN, device=dev)
        call("rac_lstm_cell_bwd", ptr(dh_d), ptr(dcn_d) if with_dc else None, ptr(act_d), ptr(cp_d), ptr(cn_d), ptr(dg2),
             ptr(dcp2), M, g, None, stream())
        for sname, slot in slot_modes(ops, dev):
            what = f"{'+'.join(kinds) or 'nosrc'} dc{int(with_dc)} {sname}"
            gbuf, dgates = guarded(dev, (M, 4 * g))
            cbuf, dcp = guarded(dev, (M, g))
            call("rac_lstm_cell_bwd_srcs", src.arr, src.n, ptr(dcn_d) if with_dc else None, ptr(act_d), ptr(cp_d), ptr(cn_d),
                 ptr(dgates), ptr(dcp), M, g, sptr(slot), stream())
            torch.cuda.synchronize()
            rule.check(f"{what} dgates", dgates, r64[0], r32[0])
            rule.check(f"{what} dc_prev", dcp, r64[1], r32[1])
            rule.check(f"{what} dgates vs cell_bwd(grad_sum)", dgates, dg2.cpu(), r32[0])
            rule.check(f"{what} dc_prev vs cell_bwd(grad_sum)", dcp, dcp2.cpu(), r32[1])
            assert_intact(gbuf, dgates, what + " dgates")
            assert_intact(cbuf, dcp, what + " dc_prev")
            if slot is not None:
                slot.check(dgates, what)
    rule.done()


@pytest.mark.parametrize("M", [3, 130])
@pytest.mark.parametrize("z", [4, 16, 64])
def test_reparam_head_bwd_vs_fp64(dev, rac, z, M):
    """rac_reparam_head_bwd: dy[m] = [dz + dmu_add | dz * eps * 0.5 * exp(0.5 * logvar) + dlogvar_add] with logvar in [-6, 2],
    dz a sum of sources, every combination of the two addends, against the fp64 formula; and the slot."""
    ops, call, ptr, stream, GradSrc, _ = rac
    rule = Rule(f"s3 reparam_head_bwd z{z} M{M}")
    u = torch.from_numpy(np.random.Generator(np.random.Philox(key=[90, 77])).random((M, z)))
    logvar = (-6.0 + 8.0 * u).to(F32)
    eps, dmu, dlv = rnd(91, M, z), rnd(92, M, z), rnd(93, M, z)
    lv_d, eps_d, dmu_d, dlv_d = logvar.to(dev), eps.to(dev), dmu.to(dev), dlv.to(dev)

    def ref(dz, a_mu, a_lv, dt):
        b = dz * eps.to(dt) * (0.5 * torch.exp(0.5 * logvar.to(dt)))
        return torch.cat([dz + dmu.to(dt) if a_mu else dz, b + dlv.to(dt) if a_lv else b], 1)

    for kinds in (("plain",), ("window",), ("plain", "slabs", "window")):
        src = Sources(GradSrc, dev, kinds, M, z)
        for a_mu in (False, True):
            for a_lv in (False, True):
                r64, r32 = ref(src.total(F64), a_mu, a_lv, F64), ref(src.total(F32), a_mu, a_lv, F32)
                for sname, slot in slot_modes(ops, dev):
                    what = f"{'+'.join(kinds)} mu{int(a_mu)} lv{int(a_lv)} {sname}"
                    obuf, dy = guarded(dev, (M, 2 * z))
                    call("rac_reparam_head_bwd", src.arr, src.n, ptr(lv_d), ptr(eps_d), ptr(dmu_d) if a_mu else None,
                         ptr(dlv_d) if a_lv else None, ptr(dy), M, z, sptr(slot), stream())
                    torch.cuda.synchronize()
                    rule.check(what, dy, r64, r32)
                    assert_intact(obuf, dy, what)
                    if slot is not None:
                        slot.check(dy, what)
    rule.done()


# =========================================================================== 4. channel plumbing
@pytest.mark.parametrize("C,Cpad,R", [(5, 8, 37), (74, 76, 37), (64, 64, 37), (74, 76, 7200)])
def test_pad_rows_and_unpad_add(dev, rac, C, Cpad, R):
    """rac_pad_rows: dst[r] = [src[r] | 0] exactly, the padding 0 even over a NaN-filled dst; rac_unpad_add, its inverse, onto
    a non-zero destination under the rule.  R = 7200 wraps the 2048-workgroup loop."""
    ops, call, ptr, stream, _, _ = rac
    src = rnd(100, R, C)
    dbuf, dst = guarded(dev, (R, Cpad))
    call("rac_pad_rows", ptr(src.to(dev)), C, ptr(dst), Cpad, R, stream())
    torch.cuda.synchronize()
    want = torch.zeros(R, Cpad)
    want[:, :C] = src
    assert torch.equal(dst.cpu(), want)
    assert_intact(dbuf, dst, "pad_rows")
    rule = Rule(f"s4 unpad_add C{C} Cpad{Cpad} R{R}")
    wide = torch.full((R, Cpad), NAN)
    wide[:, :C] = rnd(101, R, C)
    start = rnd(102, R, C)
    obuf, out = guarded(dev, (R, C), start)
    call("rac_unpad_add", ptr(wide.to(dev)), Cpad, ptr(out), C, R, stream())
    torch.cuda.synchronize()
    rule.check("dst", out, start.double() + wide[:, :C].double(), start + wide[:, :C])
    assert_intact(obuf, out, "unpad_add")
    rule.done()


@pytest.mark.parametrize("Csrc,off,n,M", [(74, 10, 64, 37), (22, 0, 3, 37), (128, 64, 64, 37), (128, 64, 64, 8200)])
def test_slice_channels(dev, rac, Csrc, off, n, M):
    """rac_slice_channels: dst[m] = src[m][off : off + n], equal to the torch slice; M = 8200 wraps the 2048-workgroup loop."""
    ops, call, ptr, stream, _, _ = rac
    src = rnd(110, M, Csrc)
    dbuf, dst = guarded(dev, (M, n))
    call("rac_slice_channels", ptr(src.to(dev)), Csrc, off, n, ptr(dst), M, stream())
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), src[:, off:off + n])
    assert_intact(dbuf, dst, "slice_channels")


@pytest.mark.parametrize("Ca,Cb,M", [(16, 16, 37), (10, 64, 37), (3, 5, 37), (10, 64, 7100)])
def test_cat2_channels(dev, rac, Ca, Cb, M):
    """rac_cat2_channels: dst[m] = [a[m] | b[m]], equal to torch.cat, with a NULL and with b NULL (zeros), and the slot;
    M = 7100 wraps the 2048-workgroup loop (with a slot: the 512-workgroup loop)."""
    ops, call, ptr, stream, _, _ = rac
    a, b = rnd(120, M, Ca), rnd(121, M, Cb) * 3.0
    a_d, b_d = a.to(dev), b.to(dev)
    for has_a, has_b in ((True, True), (False, True), (True, False)):
        want = torch.cat([a if has_a else torch.zeros(M, Ca), b if has_b else torch.zeros(M, Cb)], 1)
        for sname, slot in slot_modes(ops, dev):
            what = f"a{int(has_a)} b{int(has_b)} {sname}"
            dbuf, dst = guarded(dev, (M, Ca + Cb))
            call("rac_cat2_channels", ptr(a_d) if has_a else None, Ca, ptr(b_d) if has_b else None, Cb, ptr(dst), M,
                 sptr(slot), stream())
            torch.cuda.synchronize()
            assert torch.equal(dst.cpu(), want), what
            assert_intact(dbuf, dst, what)
            if slot is not None:
                slot.check(dst, what)


@pytest.mark.parametrize("n", [1000, 2048 * 256 + 300])
def test_act_bwd_vs_fp64(dev, rac, n):
    """rac_act_bwd through the activation OUTPUT y: sigmoid dy * y (1 - y); LeakyReLU(0.2) dy * (y > 0 ? 1 : 0.2), with
    outputs of exactly 0 (the slope of a zero pre-activation is 0.2, as torch's); no activation: a copy."""
    ops, call, ptr, stream, _, _ = rac
    rule = Rule(f"s4 act_bwd n{n}")
    dy, x = rnd(130, n), rnd(131, n)
    x[::7] = 0.0
    y_leaky, y_sig = torch.where(x > 0, x, 0.2 * x), torch.sigmoid(x)
    assert int((y_leaky == 0).sum()) >= n // 7
    dy_d = dy.to(dev)
    for name, act, y, f in (("leaky", ops.ACT_LEAKY, y_leaky, lambda d, v: d * torch.where(v > 0, torch.ones_like(v), torch.full_like(v, 0.2))),
                            ("sigmoid", ops.ACT_SIGMOID, y_sig, lambda d, v: d * (v * (1 - v))),
                            ("none", ops.ACT_NONE, x, lambda d, v: d.clone())):
        obuf, dx = guarded(dev, (n,))
        call("rac_act_bwd", ptr(dy_d), ptr(y.to(dev)), act, ptr(dx), n, stream())
        torch.cuda.synchronize()
        rule.check(name, dx, f(dy.double(), y.double()), f(dy, y))
        assert_intact(obuf, dx, name)
    rule.done()
