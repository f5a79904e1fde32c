"""The case table of the split-precision forward conv launcher (`conv16_launch`, csrc/rac_split16.hip): one shape per
template instance the launcher can pick, per workgroup-id remap on a ragged grid, and per K-split edge.  Data and
helpers; importing it needs no GPU: tests/test_conv_instances_host.py checks the table on the CPU,
tests/test_gpu_conv_instances.py and tests/conv_instances_child.py run it on the device, tools/conv_instance_census.py
records which kernel each case really launched.

`instance` is the kernel the launcher is EXPECTED to pick (derived by reading it); the authority is
tests/conv_instance_record.json, which tools/conv_instance_census.py writes from a kernel trace on an MI355X and which
is regenerated with that tool whenever the launcher's choice changes.  The record never decides whether a GPU test
passes: it backs the claim that the table reaches every instance."""
import re
from collections import namedtuple

# env: switches the launcher reads on EVERY call (RAC_ROWS_TILE2D, RAC_ROWS_FAST5), set around the launch.
# remap: the workgroup-id remap (Conv16P::xcd_group) the grid takes by the same reading; the trace cannot confirm it.
# big: exactness only (the operands are tens of MB: no fp64 reference, no feature crosses).
Case = namedtuple("Case", "name B H W k C0 C1 Cout split_k instance env remap big")


def tile(full, ym, ku):
    return "conv16_tile_kernel<2, %s, %s, %d>" % ("true" if full else "false", "true" if ym else "false", ku)


WIDTHS = {128: (2, 2), 64: (2, 1), 32: (4, 1)}  # columns per workgroup -> (WM, NT)


def rows(nv, cols, form="generic"):
    wm, nt = WIDTHS[cols]
    tail = {"generic": "2, false, 3", "fast3": "3, true, 3", "fast5": "3, true, 5"}[form]
    return "conv16_rows_kernel<%d, %d, %d, %s>" % (nv, wm, nt, tail)


def persist(nv, cols):
    return "conv16_rows_persist_kernel<%d, %d, %d>" % ((nv,) + WIDTHS[cols])


# every forward instance conv16_launch names, written out: 12 + 9 + 9 + 3 + 6 = 39
ALL_INSTANCES = (
    [tile(full, ym, ku) for ku in (0, 3, 5) for full in (True, False) for ym in (True, False)]
    + [rows(nv, cols) for cols in (128, 64, 32) for nv in (2, 3, 4)]
    + [rows(nv, cols, "fast3") for cols in (128, 64, 32) for nv in (2, 3, 4)]
    + [rows(nv, 128, "fast5") for nv in (2, 3, 4)]
    + [persist(nv, cols) for cols in (64, 32) for nv in (2, 3, 4)])

# instances no admitted shape reaches, with the reason (nv = staged rows * 4 / 256 rounded up, at least 2)
_NV2 = ("the unrolled forms need a 128-pixel tile, and 128 pixels plus any halo stage more than 128 rows: nv >= 3 "
        "(whole rows: 128 + 2 pad W; 2-D tiles: 180)")
UNREACHABLE = {
    rows(2, 128, "fast3"): _NV2,
    rows(2, 64, "fast3"): _NV2,
    rows(2, 32, "fast3"): _NV2,
    rows(2, 128, "fast5"): _NV2,
    rows(4, 128, "fast5"): "nv 4 with a 128-pixel whole-row tile and a two-row halo means W = 32 (W = 64 stages 384 rows: "
                           "refused); its padded-row plane, 8 x 36 rows = 73 728 B, exceeds ROWS_LDS_MAX: the generic loop",
    persist(2, 64): "the persistent kernel is only taken from the unrolled 3x3 form: " + _NV2,
    persist(2, 32): "the persistent kernel is only taken from the unrolled 3x3 form: " + _NV2,
}

CASES = []


def case(name, B, H, W, k, Cin, Cout, split_k, instance, env=None, remap=0, big=False, C1=0):
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, B, H, W, k, Cin - C1, C1, Cout, split_k, instance, dict(env or {}), remap, big))


# ---- whole-image tile kernel (H W <= 128), Cout 128: (FULL, YM) x KU ----
# 8x8: one 128-row tile of two images; 6x8: 96-row tiles of two images, the second tile holds one image of two;
# 4x8: four images per tile, the second tile ragged (one image of four); 3x16: 96-row tiles, W != 8.
for form, (B, H, W, full, ym) in {"full_ym": (2, 8, 8, True, True), "short_ym": (3, 6, 8, False, True),
                                   "full": (5, 4, 8, True, False), "short": (3, 3, 16, False, False)}.items():
    case("tile_%s_u3" % form, B, H, W, 3, 64, 128, 1, tile(full, ym, 3))
    case("tile_%s_k3_split4" % form, B, H, W, 3, 64, 128, 4, tile(full, ym, 0))   # 18 chunk-taps, cps 5: 5 5 5 3
    case("tile_%s_k5_split2" % form, B, H, W, 5, 32, 128, 2, tile(full, ym, 0))   # 25 chunk-taps, cps 13: 13 12
    case("tile_%s_u5" % form, B, H, W, 5, 32, 128, 1, tile(full, ym, 5))

# ---- rows kernel, generic loop: staging depth nv x columns per workgroup ----
# nv 2: 12x16 maps take 96-pixel tiles (6 rows): not the unrolled form's 128
case("rows_generic_nv2_c128", 2, 12, 16, 3, 32, 96, 1, rows(2, 128))     # 96 of the 128 columns stored
case("rows_generic_nv2_c64", 2, 12, 16, 3, 32, 64, 1, rows(2, 64))
case("rows_generic_nv2_c32", 2, 12, 16, 3, 32, 32, 1, rows(2, 32))
# nv 3: 5x5 on 16x16; the unrolled 5x5 form is for 128 columns and whole chunks per K range (split 2: cps 13)
case("rows_generic_nv3_c128", 2, 16, 16, 5, 32, 128, 2, rows(3, 128))
case("rows_generic_nv3_c64", 2, 16, 16, 5, 32, 64, 1, rows(3, 64))
case("rows_generic_nv3_c32", 2, 16, 16, 5, 32, 32, 1, rows(3, 32))
# nv 4: 5x5 on 32x32 (4 rows + 4 halo rows = 256 staged); at 128 columns the padded-row plane exceeds ROWS_LDS_MAX
case("rows_generic_nv4_c128", 1, 32, 32, 5, 32, 128, 1, rows(4, 128))
case("rows_generic_nv4_c64", 1, 32, 32, 5, 32, 64, 1, rows(4, 64))
case("rows_generic_nv4_c32", 1, 32, 32, 5, 32, 32, 1, rows(4, 32))

# ---- rows kernel, unrolled 3x3 ----
case("rows_fast3_nv3_c128", 2, 16, 16, 3, 32, 160, 1, rows(3, 128, "fast3"))  # two column tiles, 32 of 128 in the second
case("rows_fast3_nv3_c64", 2, 16, 16, 3, 32, 64, 1, rows(3, 64, "fast3"))
case("rows_fast3_nv3_c32", 2, 16, 16, 3, 32, 32, 1, rows(3, 32, "fast3"))
case("rows_fast3_2d_c128", 1, 8, 64, 3, 32, 128, 1, rows(3, 128, "fast3"))    # 2-D tiles: 180 staged pixels, nv 3
case("rows_fast3_2d_c64", 1, 8, 64, 3, 32, 64, 1, rows(3, 64, "fast3"))
case("rows_fast3_2d_c32", 1, 8, 64, 3, 32, 32, 1, rows(3, 32, "fast3"))
case("rows_fast3_nv4_c128", 2, 4, 64, 3, 32, 128, 1, rows(4, 128, "fast3"))   # H % 8 != 0: whole rows, 2 + 2 of 64
case("rows_fast3_nv4_c64", 2, 4, 64, 3, 32, 64, 1, rows(4, 64, "fast3"))
case("rows_fast3_nv4_c32", 2, 4, 64, 3, 32, 32, 1, rows(4, 32, "fast3"))
case("rows_fast3_2d_w128", 1, 8, 128, 3, 32, 64, 1, rows(3, 64, "fast3"))     # 128 wide: 2-D tiles only
for cols in (128, 64, 32):  # the 2-D-tile shapes on whole-row tiles
    case("rows_fast3_no2d_c%d" % cols, 1, 8, 64, 3, 32, cols, 1, rows(4, cols, "fast3"), env={"RAC_ROWS_TILE2D": "0"})

# ---- rows kernel, unrolled 5x5 (padded rows), and the same conv on the generic loop ----
case("rows_fast5", 2, 16, 16, 5, 32, 128, 1, rows(3, 128, "fast5"), env={"RAC_ROWS_FAST5": "1"})
case("rows_fast5_off", 2, 16, 16, 5, 32, 128, 1, rows(3, 128), env={"RAC_ROWS_FAST5": "0"})

# ---- persistent rows kernel: 2048 tiles, the smallest grid that qualifies (4 x 512 workgroups) ----
case("persist_nv3_c64", 64, 64, 64, 3, 32, 64, 1, persist(3, 64), remap=5, big=True)
case("persist_nv3_c32", 64, 64, 64, 3, 32, 32, 1, persist(3, 32), remap=5, big=True)
case("persist_nv4_c64", 1024, 4, 64, 3, 32, 64, 1, persist(4, 64), remap=5, big=True)
case("persist_nv4_c32", 1024, 4, 64, 3, 32, 32, 1, persist(4, 32), remap=5, big=True)
# 16 400 tiles over 512 workgroups: 32 or 33 tiles each
case("persist_ragged", 8200, 16, 16, 3, 32, 32, 1, persist(3, 32), remap=5, big=True)

# ---- workgroup-id remaps on ragged grids ----
# mode 2: 78 x 2 workgroups = 156 ids: 128 in the 64-tile region, 16 in the 8-tile region, 12 in the natural tail
case("remap2_ragged", 13, 24, 32, 3, 32, 256, 1, rows(3, 128, "fast3"), remap=2)
# mode 6: 138 tiles, 128 remapped in runs of 8, 10 in the natural order
case("remap6_ragged", 23, 24, 32, 3, 32, 64, 1, rows(3, 64, "fast3"), remap=6)
# mode 3: 65 M-tiles x 16 column tiles, the last M-tile holds one image of two
case("remap3_ragged", 129, 6, 8, 3, 32, 2048, 1, tile(False, True, 3), remap=3, big=True)
case("remap1_tile", 3, 8, 8, 3, 32, 1024, 1, tile(True, True, 3), remap=1)          # 2 x 8 workgroups
case("remap1_rows", 2, 16, 16, 3, 256, 128, 8, rows(3, 128, "fast3"), remap=1)      # 4 x 1 x 8, cps 9

CASES = tuple(CASES)
BY_NAME = {c.name: c for c in CASES}


def kernel_instance(kernel_name):
    """`conv16_...<...>` of a (demangled) kernel name as the trace prints it, spelled as in this module; None for other
    kernels.  Defaulted template arguments are written out."""
    m = re.search(r"(conv16_\w+)<([^>]*)>", kernel_name)
    if m is None:
        return None
    args = [a.strip() for a in m.group(2).split(",")]
    if m.group(1) == "conv16_tile_kernel":
        args += ["false", "0"][len(args) - 2:] if len(args) < 4 else []
    elif m.group(1) == "conv16_rows_kernel":
        args += ["false", "3"][len(args) - 4:] if len(args) < 6 else []
    return "%s<%s>" % (m.group(1), ", ".join(args))


def split_ranges(c, split_k=None):
    """[(first, end)] chunk-tap ranges of the K splits as the launcher cuts them (2-D tiles: whole channel chunks per
    split), empty ranges included."""
    split_k = split_k or c.split_k
    nchunks = c.k * c.k * ((c.C0 + c.C1) // 32)
    cps = -(-nchunks // split_k)
    tm = _rows_tile_m(c.H, c.W) if c.W <= 128 else 0
    fits = tm and (tm + 2 * (c.k // 2) * c.W) * 4 <= 1024        # a whole-row tile with its halo fits the LDS image
    tile2d = c.H * c.W > 128 and c.k == 3 and c.W >= 64 and c.W % 16 == 0 and c.H % 8 == 0
    if tile2d and cps % 9 and not fits:
        cps = -(-cps // 9) * 9  # (a map that fits whole-row tiles takes the generic loop on them instead)
    return [(min(s * cps, nchunks), min((s + 1) * cps, nchunks)) for s in range(split_k)]


def _rows_tile_m(H, W):
    for r in range(128 // W, 0, -1):
        if H % r == 0 and (r * W) % 16 == 0:
            return r * W
    return 0


# K-split edges on one case of each family: (case name, shape overrides, split_k) -- a short last range, and trailing
# EMPTY ranges (their slabs must come out all zeros)
SPLIT_EDGES = (
    ("tile_full_ym_u3", {}, 4),                          # 18 chunk-taps: 5 5 5 3
    ("tile_full_ym_u3", {}, 7),                          # cps 3: six ranges of 3, the seventh empty
    ("tile_short_k5_split2", {}, 9),                     # 25 chunk-taps, cps 3: 8 x 3 + 1
    ("rows_generic_nv2_c128", {"C0": 64}, 4),            # 18: 5 5 5 3
    ("rows_generic_nv2_c128", {"C0": 64}, 7),            # 18, cps 3: an empty seventh range
    ("rows_fast3_nv3_c128", {"C0": 96}, 2),              # 27 chunk-taps, cps 14: cuts a chunk -> the generic loop, 14 13
    ("rows_fast3_nv3_c128", {"C0": 96}, 3),              # cps 9: whole chunks, the unrolled form
    ("rows_fast3_nv3_c128", {"C0": 64}, 7),              # 18, cps 3: generic loop, an empty seventh range
    # empty ranges in the UNROLLED forms (whole chunks per range): 81 chunk-taps over 10 splits, cps 9, the tenth empty
    ("tile_full_ym_u3", {"C0": 288}, 10),
    ("rows_fast3_nv3_c128", {"C0": 288}, 10),
    ("rows_fast3_2d_w128", {"C0": 64}, 4),               # 128 wide: cps 5 rounded to 9: 9 9 and two empty ranges
    ("rows_fast3_2d_c64", {"C0": 96}, 2),                # 27, cps 14: the map fits whole-row tiles -> generic loop, 14 13
    ("rows_fast3_2d_w128", {"C0": 96}, 2),               # 27, cps 14 rounded to 18: 18 9 (short last range of whole chunks)
)


# ---------------------------------------------------------------------------------------------------------------------
# Device helpers (torch and the package are imported when they run, not with this module)
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 4096     # NaN floats either side of every output the tests hand to a launch
SLAB_GAP = 32    # NaN floats between two K-split slabs (slab_stride = M Cout + SLAB_GAP)


def int_operands(c, seed=0):
    """(x [B, Cin, H, W], w [Cout, Cin, k, k]) of small integers in [-3, 3], Philox-seeded: every product and sum is
    exact in the first fp16 part and in fp32 (|sum| <= 9 K < 2^24), so the conv has ONE right answer."""
    import numpy as np
    import torch
    g = np.random.Generator(np.random.Philox(key=[seed, 23]))
    Cin = c.C0 + c.C1
    x = torch.from_numpy(g.integers(-3, 4, (c.B, Cin, c.H, c.W), dtype=np.int8).astype(np.float32))
    w = torch.from_numpy(g.integers(-3, 4, (c.Cout, Cin, c.k, c.k), dtype=np.int8).astype(np.float32))
    return x, w


def real_operands(c, seed=1):
    """(x, w, bias) real-valued, as the split-precision tests of tests/test_gpu_ops.py draw them."""
    import numpy as np
    from tests.fp64_tools import rnd
    Cin = c.C0 + c.C1
    return (rnd(seed, c.B, Cin, c.H, c.W), rnd(seed + 1, c.Cout, Cin, c.k, c.k) * (1.0 / np.sqrt(Cin * c.k * c.k)),
            rnd(seed + 2, c.Cout))


class Guarded:
    """`n` floats (or `rows` x `n` with SLAB_GAP floats between the rows) inside a NaN-filled buffer with GUARD floats
    either side: `check()` -- every float of the view was written (no NaN left), nothing outside it was touched."""

    def __init__(self, dev, n, rows=1):
        import torch
        self.n, self.rows, self.stride = n, rows, n + (SLAB_GAP if rows > 1 else 0)
        self.buf = torch.full((2 * GUARD + rows * self.stride,), float("nan"), device=dev, dtype=torch.float32)
        self.body = self.buf[GUARD:GUARD + rows * self.stride]
        self.view = self.body.view(rows, self.stride)[:, :n]  # [rows][n]

    def check(self, what=""):
        import torch
        nan = torch.isnan(self.buf)
        inside = torch.zeros_like(nan)
        inside[GUARD:GUARD + self.rows * self.stride].view(self.rows, self.stride)[:, :self.n] = True
        unwritten = int((nan & inside).sum())
        assert unwritten == 0, "%s: %d of %d output floats were never written (first at %d)" % (
            what, unwritten, self.rows * self.n, int((nan & inside).nonzero()[0]) - GUARD)
        stray = int((~nan & ~inside).sum())
        assert stray == 0, "%s: %d floats outside the output were written (first at %d)" % (
            what, stray, int((~nan & ~inside).nonzero()[0]) - GUARD)


class _Env:
    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        import os
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def to_map(x, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(dev)


def from_map(m):
    return m.permute(0, 3, 1, 2).cpu()


def cl_weight(w):
    """logical (Cout, Cin, k, k) tensor stored [Cout][k][k][Cin]."""
    return w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


Launched = namedtuple("Launched", "y slabs pooled slot stats out pool")


def launch(dev, c, x, w, *, bias=None, scale=None, shift=None, act=0, stats_groups=0, per_image=False, up=False,
           zero_x1=False, pool=False):
    """ONE rac_conv2d_fwd_split launch of case `c` through ops._split_launch, the output (or the split_k slabs) a view
    into a NaN-filled guarded buffer that is checked before anything is returned.
    x: [B, C0 + C1, H, W] on the CPU ([B, C0, H/2, W/2] stacked on nothing with `up`: then C1 must be 0, or x is a pair
    (x0 half resolution, x1)); w: [Cout, Cin_w, k, k] -- `zero_x1`: Cin_w > C0 and the second source is an all-zero
    tensor flagged `_rac_zero`, which the launch skips (w_cin = Cin_w) as ops.conv_forward_split does.
    -> Launched(y [B, Cout, H, W] on the CPU (split_k > 1: the fp64 sum of the slabs, as float32 when exact),
                slabs [split_k, B, Cout, H, W] or None, pooled or None, out_amax slots or None, stats or None, ...)"""
    import torch
    from robot_aware_control_amd import ops
    B, H, W, k, Cout, split_k = c.B, c.H, c.W, c.k, c.Cout, c.split_k
    if isinstance(x, tuple):
        x0, x1 = to_map(x[0], dev), (to_map(x[1], dev) if x[1] is not None else None)
    else:
        x0, x1 = to_map(x[:, :c.C0], dev), (to_map(x[:, c.C0:], dev) if c.C1 else None)
    wd = cl_weight(w).to(dev)
    C0, w_cin = c.C0, 0
    if zero_x1:
        x1 = torch.zeros((B, H, W, w.shape[1] - C0), device=dev)
        x1._rac_zero = True
    if ops.is_zero(x1) and C0 % 32 == 0:
        x1, w_cin = None, w.shape[1]
    Cin = C0 + (x1.shape[3] if x1 is not None else 0)
    assert Cin == w.shape[1] or w_cin
    M = B * H * W
    a0 = ops.amax_for(x0, per_image)
    a1 = ops.amax_for(x1, per_image) if x1 is not None else None
    pw, wslot = ops.weight_parts(wd)
    out = Guarded(dev, M * Cout, rows=split_k)
    pl = Guarded(dev, (M // 4) * Cout) if pool else None
    slot = ops.amax_slot(dev, B if per_image else 1) if split_k == 1 else None
    stats = torch.zeros((max(stats_groups, 1), 2, Cout), device=dev, dtype=torch.float64) if stats_groups else None
    dv = lambda t: None if t is None else t.to(dev)  # noqa: E731
    with _Env(c.env):
        ops._split_launch(x0, x1, a0, a1, pw, wslot, out.body, B=B, H=H, W=W, k=k, Cin=Cin, Cout=Cout, C0=C0, act=act,
                          bias=dv(bias), scale=dv(scale), shift=dv(shift), stats=stats, split_k=split_k,
                          slab_stride=out.stride if split_k > 1 else 0,
                          stats_rows=M // stats_groups if stats_groups > 1 else 0, out_amax=slot, w_cin=w_cin,
                          a0_up=1 if up else 0, per_image=per_image, pool=pl.body.view(B, H // 2, W // 2, Cout) if pool else None)
    torch.cuda.synchronize()
    out.check(c.name)
    if pool:
        pl.check(c.name + " (pooled)")
    maps = out.view.view(split_k, B, H, W, Cout)
    slabs = maps.permute(0, 1, 4, 2, 3).cpu() if split_k > 1 else None
    y = from_map(maps[0]) if split_k == 1 else slabs.double().sum(0)
    return Launched(y, slabs, from_map(pl.view.view(B, H // 2, W // 2, Cout)) if pool else None, slot, stats, out, pl)


def can_pool(dev, c):
    """The launcher's own answer (rac_conv2d_fwd_split_pool_ok): does this case's conv pool in its epilogue?"""
    from robot_aware_control_amd import _lib
    import ctypes as C
    if c.split_k > 1 or c.H * c.W <= 128:
        return False
    args = _lib.ConvArgs(mode=0, B=c.B, H=c.H, W=c.W, ksize=c.k, Cin=c.C0 + c.C1, Cout=c.Cout, act=0, split_k=1,
                         accumulate=0, a_split=c.C0 if c.C1 else 0, o_split=0, slab_stride=0, stats_rows=0, a0_up=0,
                         amax_per_image=0)
    args.a0, args.w, args.out0 = 0x10000, 0x20000, 0x30000  # never dereferenced: a pure host query
    args.a1 = 0x40000 if c.C1 else None
    with _Env(c.env):
        return bool(_lib.load().rac_conv2d_fwd_split_pool_ok(C.byref(args), 0))


def exact_case(dev, c, stride=1):
    """The exactness part of one case: integer operands, NaN / guard checks on the whole buffer(s), every output element
    (every `stride`-th image of a big case) equal to F.conv2d on the CPU; pooled too where the conv pools; empty K ranges
    give all-zero slabs.  -> the Launched record."""
    import torch
    import torch.nn.functional as F
    x, w = int_operands(c)
    pool = can_pool(dev, c)
    got = launch(dev, c, x, w, pool=pool)
    idx = slice(None, None, stride)
    ref = F.conv2d(x[idx], w, None, 1, c.k // 2)
    y = got.y[idx]
    assert torch.equal(y.float() if c.split_k > 1 else y, ref), "%s: %d of %d output elements differ from F.conv2d" % (
        c.name, int((y != ref).sum()), ref.numel())
    if pool:
        assert torch.equal(got.pooled[idx], F.max_pool2d(ref, 2)), c.name + ": pooled output"
    if c.split_k > 1:
        for s, (k0, k1) in enumerate(split_ranges(c)):
            assert k0 < k1 or not bool(got.slabs[s].any()), "%s: the slab of empty K range %d is not all zeros" % (c.name, s)
    return got
