"""GPU: every forward instance of the split-precision conv launcher (`conv16_launch`, csrc/rac_split16.hip), every
workgroup-id remap on a ragged grid and every K-split edge, one launch at a time through ops._split_launch so that the
test owns `split_k` and the output buffer (tests/conv_instance_cases.py holds the table and the launch helper).

Per case: the output (or the K-split slabs, or the pooled map) is a view into a NaN-filled buffer with 4096 guard floats
either side -- afterwards no NaN is left inside and every float outside is still NaN, so a tile no workgroup wrote or a
store past a ragged tile / past Cout cannot hide behind an earlier launch's values; small-integer operands must give
F.conv2d's result exactly (which pins every output element's tile, row and column); real-valued operands are held to
the bounds of tests/test_gpu_ops.py against fp64: relerr < 2e-6 and < 4 x (error of the exact-fp32 path) + 2e-7."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import conv_instance_cases as cc  # noqa: E402
from tests.fp64_tools import relerr, rnd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def conv64(x, w, bias=None):
    return F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), 1, w.shape[2] // 2)


def fp32_error(dev, c, x, w, bias, ref):
    """relerr of the exact-fp32 MFMA path (ops.conv_forward, allow_split=False) on the same operands: the yardstick."""
    from robot_aware_control_amd import ops
    x0 = cc.to_map(x[:, :c.C0], dev)
    x1 = cc.to_map(x[:, c.C0:], dev) if c.C1 else None
    y = ops.conv_forward(x0, x1, cc.cl_weight(w).to(dev), None if bias is None else bias.to(dev), allow_split=False)
    return relerr(cc.from_map(y), ref)


def held(name, e_split, e_fp32):
    print("[conv16] %s: e_split %.2e e_fp32 %.2e" % (name, e_split, e_fp32))
    assert e_split < 2e-6 and e_split < 4 * e_fp32 + 2e-7, (name, e_split, e_fp32)


@pytest.mark.parametrize("name", [c.name for c in cc.CASES if not c.big])
def test_instance_is_exact_and_accurate(dev, name):
    c = cc.BY_NAME[name]
    cc.exact_case(dev, c)
    x, w, b = cc.real_operands(c)
    b = None if c.split_k > 1 else b  # (slabs are raw partial sums: no epilogue)
    ref = conv64(x, w, b)
    got = cc.launch(dev, c, x, w, bias=b)
    held(name, relerr(got.y, ref), fp32_error(dev, c, x, w, b, ref))
    if got.slot is not None:  # the epilogue folds max |y| of what it stored into the slot
        assert int(got.slot.cpu()) == int(got.y.abs().max().view(torch.int32))


@pytest.mark.parametrize("name", [c.name for c in cc.CASES if c.big])
def test_big_grid_is_exact(dev, name):
    """The persistent kernel's smallest and ragged walks and the mode-3 remap: exactness alone (every image against the
    CPU reference; NaN and guard checks on the whole buffer)."""
    cc.exact_case(dev, cc.BY_NAME[name])


@pytest.mark.parametrize("name,over,split_k", cc.SPLIT_EDGES, ids=["%s-%s-split%d" % (n, "_".join(
    "%s%d" % kv for kv in o.items()) or "as_is", s) for n, o, s in cc.SPLIT_EDGES])
def test_split_edges(dev, name, over, split_k):
    """K splits the planner never picks but the ABI admits: a short last range, trailing EMPTY ranges (their slabs all
    zeros), 2-D tiles whose ranges are rounded to whole channel chunks.  The slab sum is exact on integers."""
    c = cc.BY_NAME[name]._replace(split_k=split_k, env={}, **over)
    ranges = cc.split_ranges(c)
    assert len(ranges) == split_k and ranges[-1][1] == c.k * c.k * (c.C0 // 32)
    got = cc.exact_case(dev, c)
    assert got.slabs.shape[0] == split_k
    x, w, _ = cc.real_operands(c)
    ref = conv64(x, w)
    held("%s split %d" % (name, split_k), relerr(cc.launch(dev, c, x, w).y, ref), fp32_error(dev, c, x, w, None, ref))


# one case per family for the feature crosses: the tile kernel (y-major short tile: the second tile's second image is
# missing; row-major ragged full tile), the rows kernel's generic loop (Cout 96: n_store < N), its unrolled 3x3 form on
# whole rows (Cout 160: two column tiles) and on 2-D tiles, and its unrolled 5x5 form
FAMILIES = ("tile_short_ym_u3", "tile_full_u3", "rows_generic_nv2_c128", "rows_fast3_nv3_c128", "rows_fast3_2d_c64", "rows_fast5")
ROWS_FAMILIES = FAMILIES[2:]


@pytest.mark.parametrize("name", FAMILIES)
def test_two_sources_and_skipped_zero_source(dev, name):
    """C1 > 0: channels [C0, Cin) come from the second tensor; and a second source that is all zeros (`_rac_zero`) is
    skipped: the conv runs over the first C0 channels of the same weight parts (w_cin > Cin)."""
    base = cc.BY_NAME[name]
    c = base._replace(C0=32, C1=32)
    cc.exact_case(dev, c)
    x, w, b = cc.real_operands(c)
    ref = conv64(x, w, b)
    held(name + " two sources", relerr(cc.launch(dev, c, x, w, bias=b).y, ref), fp32_error(dev, c, x, w, b, ref))
    # the zero source: x has C0 channels, the weight C0 + 32
    z = base._replace(C0=32, C1=0)
    xi, wi = cc.int_operands(c)
    got = cc.launch(dev, z, xi[:, :32], wi, zero_x1=True)
    assert torch.equal(got.y, F.conv2d(xi[:, :32], wi[:, :32], None, 1, c.k // 2))
    refz = conv64(x[:, :32], w[:, :32], b)
    e32 = fp32_error(dev, z, x[:, :32], w[:, :32].contiguous(), b, refz)
    held(name + " zero source", relerr(cc.launch(dev, z, x[:, :32], w, bias=b, zero_x1=True).y, refz), e32)


@pytest.mark.parametrize("name", ROWS_FAMILIES)
@pytest.mark.parametrize("C1", [0, 32])
def test_half_resolution_first_source(dev, name, C1):
    """a0_up: the first source is the [B, H/2, W/2, C0] tensor, read at (y / 2, x / 2)."""
    c = cc.BY_NAME[name]._replace(C0=32, C1=C1)
    half = c._replace(H=c.H // 2, W=c.W // 2, C1=0)
    xh, _ = cc.int_operands(half, seed=3)
    xi, wi = cc.int_operands(c)
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
    got = cc.launch(dev, c, (xh, xi[:, 32:] if C1 else None), wi, up=True)
    assert torch.equal(got.y, F.conv2d(torch.cat([up(xh), xi[:, 32:]], 1), wi, None, 1, c.k // 2))
    x, w, b = cc.real_operands(c)
    xr = rnd(7, *xh.shape)
    full = torch.cat([up(xr), x[:, 32:]], 1)
    ref = conv64(full, w, b)
    held(name + " a0_up", relerr(cc.launch(dev, c, (xr, x[:, 32:] if C1 else None), w, bias=b, up=True).y, ref),
         fp32_error(dev, c, full, w, b, ref))


@pytest.mark.parametrize("name", FAMILIES)
def test_per_image_scales_and_fused_epilogue(dev, name):
    """Every image scaled by its own maximum (images four decades apart), bias + folded BatchNorm scale / shift + leaky
    ReLU in the epilogue, against fp64 image by image; the out_amax slots hold the bit pattern of every image's max |y|
    -- also for the image a short last tile does not hold (the 3 x 6 x 8 case)."""
    c = cc.BY_NAME[name]
    x, w, b = cc.real_operands(c)
    mags = torch.tensor([1.0, 3e-4, 2e3, 0.07, 11.0])[:c.B].view(c.B, 1, 1, 1)
    x = x * mags
    scale, shift = rnd(11, c.Cout).abs() + 0.5, rnd(12, c.Cout, scale=0.2)
    ref = F.leaky_relu(conv64(x, w, b) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1), 0.2)
    from robot_aware_control_amd import ops
    got = cc.launch(dev, c, x, w, bias=b, scale=scale, shift=shift, act=ops.ACT_LEAKY, per_image=True)
    assert got.slot.numel() == c.B
    assert torch.equal(got.slot.cpu(), got.y.abs().amax((1, 2, 3)).view(torch.int32))
    # the exact-fp32 path scales nothing: its error on each image alone is the yardstick of that image
    x0 = cc.to_map(x, dev)
    y32 = cc.from_map(ops.conv_forward(x0, None, cc.cl_weight(w).to(dev), b.to(dev), act=ops.ACT_LEAKY, scale=scale.to(dev),
                                       shift=shift.to(dev), allow_split=False))
    for i in range(c.B):
        held("%s per_image %d" % (name, i), relerr(got.y[i], ref[i]), relerr(y32[i], ref[i]))
    # integers: per-image scales are powers of two, so exactness holds with them too
    xi, wi = cc.int_operands(c)
    xi = xi * torch.tensor([1.0, 4.0, 0.5, 64.0, 2.0])[:c.B].view(c.B, 1, 1, 1)
    goti = cc.launch(dev, c, xi, wi, per_image=True)
    assert torch.equal(goti.y, F.conv2d(xi, wi, None, 1, c.k // 2))
    assert torch.equal(goti.slot.cpu(), goti.y.abs().amax((1, 2, 3)).view(torch.int32))


@pytest.mark.parametrize("name,B,groups", [("tile_short_ym_u3", 4, 2), ("tile_short_ym_u3", 3, 1), ("tile_full_u3", 8, 2),
                                           ("tile_full_u3", 5, 1), ("rows_generic_nv2_c128", 2, 2),
                                           ("rows_fast3_nv3_c128", 2, 2), ("rows_fast3_2d_c64", 2, 2), ("rows_fast5", 3, 3)])
def test_batch_statistics(dev, name, B, groups):
    """`stats`: fp64 sum and sum of squares of the biased conv output per column and per group of `stats_rows` rows
    (groups 1: stats_rows 0, also over a ragged last tile), against fp64 sums of the fp64 conv.  The kernels sum a
    wave's rows in fp32 first, so the sums carry the outputs' fp32-level error: held to the suite's 2e-6 relative to the
    largest sum (the bias, of the outputs' own size, keeps the column sums from cancelling)."""
    c = cc.BY_NAME[name]._replace(B=B)
    x, w, b = cc.real_operands(c)
    ref = conv64(x, w, b)
    got = cc.launch(dev, c, x, w, bias=b, stats_groups=groups)
    e32 = fp32_error(dev, c, x, w, b, ref)
    held(name + " with stats", relerr(got.y, ref), e32)
    rg = ref.view(groups, B // groups, c.Cout, -1)
    s1, s2 = rg.sum((1, 3)), (rg * rg).sum((1, 3))
    st = got.stats.cpu()
    assert st.shape == (groups, 2, c.Cout)
    e1, e2 = relerr(st[:, 0], s1), relerr(st[:, 1], s2)
    print("[conv16] %s stats: e_sum %.2e e_sumsq %.2e" % (name, e1, e2))
    assert e1 < 2e-6 and e2 < 2e-6, (e1, e2)


@pytest.mark.parametrize("name", ["tile_full_ym_u3", "tile_short_u5", "rows_fast3_2d_c128", "rows_fast3_nv4_c128", "rows_fast5"])
@pytest.mark.parametrize("Cout", [96, 160])
def test_cout_that_does_not_fill_the_column_tile(dev, name, Cout):
    """n_store < N: 96 of a 128-column tile's columns, and 160 = one full tile + 32 columns of the second."""
    c = cc.BY_NAME[name]._replace(Cout=Cout)
    cc.exact_case(dev, c)
    x, w, b = cc.real_operands(c)
    ref = conv64(x, w, b)
    held("%s Cout %d" % (name, Cout), relerr(cc.launch(dev, c, x, w, bias=b).y, ref), fp32_error(dev, c, x, w, b, ref))


POOLING = ("rows_fast3_nv3_c64", "rows_fast3_nv3_c32", "rows_fast3_2d_c128", "rows_fast3_2d_c64", "rows_fast3_2d_c32",
           "remap2_ragged", "remap6_ragged", "persist_nv3_c64")


@pytest.mark.parametrize("name", POOLING)
def test_pool_in_the_epilogue(dev, name):
    """pool=True where the launcher admits it (`exact_case` asks the launcher and pools wherever it says yes -- here the
    answer itself is pinned): the pooled map, in its own guarded buffer, is max_pool2d of the exact output, and with a
    fused epilogue of the activated one."""
    c = cc.BY_NAME[name]
    assert cc.can_pool(dev, c)
    got = cc.exact_case(dev, c)
    assert got.pooled is not None
    if c.big:
        return
    from robot_aware_control_amd import ops
    x, w, b = cc.real_operands(c)
    scale, shift = rnd(11, c.Cout).abs() + 0.5, rnd(12, c.Cout, scale=0.2)
    got = cc.launch(dev, c, x, w, bias=b, scale=scale, shift=shift, act=ops.ACT_LEAKY, per_image=True, pool=True)
    assert torch.equal(got.pooled, F.max_pool2d(got.y, 2))
    ref = F.leaky_relu(conv64(x, w, b) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1), 0.2)
    assert relerr(got.y, ref) < 2e-6


CHILDREN = {
    # every process-wide A/B switch of the README at once: the generic tile loop, row-major 8x8 tiles, the rows kernels'
    # generic loop on whole rows, no persistent walk, hardware workgroup order
    "all_off": (dict(RAC_TILE_UNROLL3="0", RAC_TILE_UNROLL5="0", RAC_TILE_YMAJOR="0", RAC_ROWS_GENERIC="1",
                     RAC_ROWS_PERSIST="0", RAC_XCD_GROUP="0"), "all"),
    # RAC_ROWS_GENERIC=1 keeps the whole-row persistent shapes off the unrolled form altogether: RAC_ROWS_PERSIST=0 alone
    # puts their 2048- and 16 400-tile grids through the one-tile-per-workgroup unrolled kernels
    "persist_off": (dict(RAC_ROWS_PERSIST="0"), "persist"),
}


@pytest.mark.parametrize("child", sorted(CHILDREN))
def test_process_wide_switches_in_a_child(dev, child):
    """The launcher reads these switches once per process: a fresh child runs the table's exactness part under them."""
    env, which = CHILDREN[child]
    full = dict(os.environ, **env)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_instances_child.py"), which], cwd=ROOT, env=full,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    lines = [ln.split() for ln in res.stdout.splitlines() if ln.startswith("case ")]
    want = [c.name for c in cc.CASES if which == "all" or c.name.startswith(which)]
    assert [ln[1] for ln in lines] == want and all(ln[2] == "exact" for ln in lines), res.stdout[-2000:]
