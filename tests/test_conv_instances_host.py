"""CPU: the conv instance table (tests/conv_instance_cases.py) accounts for every forward instance of the split-precision
conv launcher, every case is a shape the library takes, and the committed census record
(tests/conv_instance_record.json, written on an MI355X by tools/conv_instance_census.py from a kernel trace) names, for
every case, the kernel the table expects."""
import json
import os
import re

import pytest

from robot_aware_control_amd import _lib
from tests import conv_instance_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(os.path.dirname(HERE), "robot_aware_control_amd", "csrc", "rac_split16.hip")


def record():
    with open(os.path.join(HERE, "conv_instance_record.json")) as f:
        return json.load(f)


def test_table_and_unreachable_list_are_the_full_instance_list():
    expected = {c.instance for c in cc.CASES}
    assert len(cc.ALL_INSTANCES) == len(set(cc.ALL_INSTANCES)) == 39
    assert not expected & set(cc.UNREACHABLE)
    assert expected | set(cc.UNREACHABLE) == set(cc.ALL_INSTANCES)
    assert len(cc.UNREACHABLE) == 7 and all(cc.UNREACHABLE.values())


def test_instance_list_is_the_launcher_s():
    """The list written out in the module against the launcher's text: every `conv16_*_kernel<...>` named inside
    conv16_launch, defaulted template arguments filled in."""
    text = open(SOURCE).read()
    body = text[text.index("static int conv16_launch("):text.index('extern "C" int rac_conv2d_fwd_split(')]
    named = {cc.kernel_instance(m.group(0)) for m in re.finditer(r"conv16_\w+<[^>]*>", body)}
    assert named == set(cc.ALL_INSTANCES)


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_case_is_a_supported_shape(name):
    c = cc.BY_NAME[name]
    assert _lib.load().rac_conv2d_split_supported(c.H, c.W, c.k, c.C0 + c.C1, c.Cout, c.C0 if c.C1 else 0) == 1
    assert c.C1 == 0 or c.C0 % 32 == 0
    ranges = cc.split_ranges(c)
    assert ranges[0][0] == 0 and ranges[-1][1] == c.k * c.k * ((c.C0 + c.C1) // 32)
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))


def test_split_edges_have_short_and_empty_ranges():
    kinds = set()
    for name, over, split_k in cc.SPLIT_EDGES:
        c = cc.BY_NAME[name]._replace(split_k=split_k, **over)
        assert _lib.load().rac_conv2d_split_supported(c.H, c.W, c.k, c.C0, c.Cout, 0) == 1
        sizes = [b - a for a, b in cc.split_ranges(c)]
        assert sum(sizes) == c.k * c.k * (c.C0 // 32) and sizes[0] > 0
        family = name.split("_")[0] + ("_2d" if "_2d" in name else "")
        kinds.add((family, "empty" if sizes[-1] == 0 else ("short" if sizes[-1] < sizes[0] else "even")))
    for family in ("tile", "rows", "rows_2d"):
        assert (family, "empty") in kinds and (family, "short") in kinds, (family, kinds)


def test_census_record_names_the_expected_instance_of_every_case():
    rec = record()
    assert list(rec) == [c.name for c in cc.CASES]
    wrong = {c.name: (c.instance, rec[c.name]) for c in cc.CASES if cc.kernel_instance(rec[c.name]) != c.instance}
    assert not wrong, wrong
    reached = {cc.kernel_instance(n) for n in rec.values()}
    assert reached == set(cc.ALL_INSTANCES) - set(cc.UNREACHABLE)


@pytest.mark.parametrize("B,H,W,stats_rows,refused", [(1, 8, 64, 256, True), (2, 16, 64, 128, True), (1, 8, 128, 512, True),
                                                      (1, 8, 64, 512, False), (2, 16, 64, 1024, False), (2, 8, 64, 0, False)])
def test_2d_tiles_refuse_statistics_groups_that_cut_a_tile(B, H, W, stats_rows, refused):
    """A 2-D tile (8 image rows x 16 pixels) adds its sums to the statistics group of its FIRST pixel: groups of fewer
    than 8 image rows would silently get their neighbours' rows, so the launcher refuses them (include/rac_hip.h,
    stats_rows).  Host checks only: every call here also asks for the pooled output, which no conv with statistics
    writes, so a call that passes the check under test is turned down by the next one and nothing is ever launched;
    the pointer values are never dereferenced."""
    import ctypes as C
    args = _lib.ConvArgs(mode=0, B=B, H=H, W=W, ksize=3, Cin=32, Cout=64, act=0, split_k=1, accumulate=0, a_split=0,
                         o_split=0, slab_stride=0, stats_rows=stats_rows, a0_up=0, amax_per_image=0)
    args.a0, args.w, args.out0, args.out1, args.stats = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    slot = (C.c_uint32 * 1)(0x3F800000)
    with pytest.raises(_lib.RacError) as e:
        _lib.call("rac_conv2d_fwd_split", C.byref(args), slot, None, 64 * 9 * 32, 0, slot, None, None)
    assert ("multiple of 8 image rows" in str(e.value)) == refused, str(e.value)
    assert refused or "cannot pool in its epilogue" in str(e.value), str(e.value)
