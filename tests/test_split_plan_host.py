"""CPU: the host-side decisions of the split-precision conv launchers (csrc/rac_split16.hip) against recorded answers.

`rac_conv2d_split_supported` and `rac_conv2d_fwd_split_pool_ok` decide on the host which convs take the split kernels and
which of them pool in their epilogue.  Both tables below are DATA recorded from the library as it was before the
launchers' repeated host code was gathered into helpers (the first on the CPU, the second on an MI355X: that library's
pool query raised kernel attributes before it answered, so it had no answer without a device) -- not derived from the
code under test.  The pool query is a pure host query now: it runs here, with pointer values that are never dereferenced."""
import ctypes as C

import pytest

from robot_aware_control_amd import _lib
from robot_aware_control_amd.model import ENC_PLAN

SIZES = ((6, 8), (8, 8), (12, 16), (16, 16), (24, 32), (32, 32), (48, 64), (64, 64), (128, 128), (20, 20), (8, 136))
KSIZES = (3, 4, 5, 7)
CHANNELS = ((64, 64, 0), (96, 32, 32), (96, 32, 16), (48, 64, 0), (64, 40, 0))  # (Cin, Cout, a_split)

# SUPPORTED[(H, W)][ki * 5 + ci]: the answer for KSIZES[ki], CHANNELS[ci]
SUPPORTED = {
    (6, 8): "11000000001100000000",
    (8, 8): "11000000001100000000",
    (12, 16): "11000000001100000000",
    (16, 16): "11000000001100000000",
    (24, 32): "11000000001100000000",
    (32, 32): "11000000001100000000",
    (48, 64): "11000000000000000000",
    (64, 64): "11000000000000000000",
    (128, 128): "11000000000000000000",
    (20, 20): "11000000001100000000",
    (8, 136): "00000000000000000000",
}


@pytest.mark.parametrize("H,W", SIZES)
def test_split_supported_table(H, W):
    lib = _lib.load()
    got = "".join(str(lib.rac_conv2d_split_supported(H, W, k, ci, co, sp)) for k in KSIZES for ci, co, sp in CHANNELS)
    assert got == SUPPORTED[(H, W)]


def encoder_convs(H, W):
    """(H, W, Cin, Cout) of the frozen encoder's 3x3 convs (model.py ENC_PLAN; the image's channels padded to 32, the
    4x4 conv behind c4 left out)."""
    out = []
    for i, (_, widths) in enumerate(ENC_PLAN):
        widths = [32 if w is None and j == 0 else w for j, w in enumerate(widths)]
        out += [(H >> i, W >> i, ci, co) for ci, co in zip(widths, widths[1:]) if co is not None]
    return out


def pool_cases():
    """name -> keyword arguments of one query (B 2, k 3 unless said otherwise)."""
    cases = {}
    for H0, W0 in ((64, 64), (48, 64)):
        for H, W, ci, co in encoder_convs(H0, W0):
            cases["enc%dx%d_%dx%d_%d_%d" % (H0, W0, H, W, ci, co)] = dict(H=H, W=W, Cin=ci, Cout=co)
    # one shape of each refusing kind, each next to an encoder conv that pools
    cases["stats"] = dict(H=32, W=32, Cin=128, Cout=128, stats=True)
    cases["split_k2"] = dict(H=32, W=32, Cin=128, Cout=128, split_k=2)
    cases["fits_a_tile"] = dict(H=8, W=16, Cin=128, Cout=128)
    cases["odd_h"] = dict(H=15, W=16, Cin=128, Cout=128)
    cases["cout_96_of_128"] = dict(H=32, W=32, Cin=128, Cout=96)
    return cases


def pool_query(lib, H, W, Cin, Cout, B=2, k=3, split_k=1, stats=False):
    # dummy 16-byte aligned, non-null pointer values: the query reads its arguments only
    args = _lib.ConvArgs(mode=0, B=B, H=H, W=W, ksize=k, Cin=Cin, Cout=Cout, act=0, split_k=split_k, accumulate=0,
                         a_split=0, o_split=0, slab_stride=B * H * W * Cout if split_k > 1 else 0, stats_rows=0, a0_up=0,
                         amax_per_image=0)
    args.a0, args.w, args.out0 = 0x10000, 0x20000, 0x30000
    args.stats = 0x40000 if stats else None
    return int(lib.rac_conv2d_fwd_split_pool_ok(C.byref(args), 0))


# recorded on an MI355X from the library before this module existed (see the module docstring)
POOL_OK = {
    "enc64x64_64x64_32_64": 1,
    "enc64x64_64x64_64_64": 1,
    "enc64x64_32x32_64_128": 1,
    "enc64x64_32x32_128_128": 1,
    "enc64x64_16x16_128_256": 1,
    "enc64x64_16x16_256_256": 1,
    "enc64x64_8x8_256_512": 0,
    "enc64x64_8x8_512_512": 0,
    "enc48x64_48x64_32_64": 1,
    "enc48x64_48x64_64_64": 1,
    "enc48x64_24x32_64_128": 1,
    "enc48x64_24x32_128_128": 1,
    "enc48x64_12x16_128_256": 0,
    "enc48x64_12x16_256_256": 0,
    "enc48x64_6x8_256_512": 0,
    "enc48x64_6x8_512_512": 0,
    "stats": 0,
    "split_k2": 0,
    "fits_a_tile": 0,
    "odd_h": 0,
    "cout_96_of_128": 0,
}


def test_pool_cases_cover_the_encoder():
    assert len(encoder_convs(64, 64)) == 9 and encoder_convs(64, 64)[0] == (64, 64, 32, 64)
    assert encoder_convs(48, 64)[-1] == (6, 8, 512, 512)
    assert set(pool_cases()) == set(POOL_OK)


@pytest.mark.parametrize("name", sorted(pool_cases()))
def test_pool_ok_is_a_host_query(name):
    assert pool_query(_lib.load(), **pool_cases()[name]) == POOL_OK[name]
