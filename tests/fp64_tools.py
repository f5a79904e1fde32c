"""Test helpers of the kernel-vs-fp64 modules (test_gpu_norm_cell.py, test_gpu_reduce.py, test_gpu_frame.py): seeded inputs,
the relative error they all use, and the tolerance rule

    e_gpu <= max(floor, 4 * e_cpu32),    floor = 2e-6 unless a test says otherwise

with e_gpu = relerr(kernel, fp64 reference) and e_cpu32 = relerr(the same formula in fp32 on the CPU with torch, the same
fp64 reference).  Every case prints both figures; nothing is excluded.

Also what the modules that drive the C ABI share (test_gpu_reduce.py, test_gpu_frame.py): outputs as views inside a
sentinel-filled buffer (`guarded`, `assert_intact`), the max |v| slot in its three modes (`Slot`, `slot_modes`, `sptr`) and
`refused` for calls the host check must turn down."""
import numpy as np
import pytest
import torch

NAN = float("nan")
SENT = 12345.0          # guard-band fill
GUARD = 64              # elements on either side of an output (64 floats keep the view 16-byte aligned)
BIG = 0x7F000000        # bits of 2^127: above every |v| these tests produce
F64, F32 = torch.float64, torch.float32


def rnd(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.Philox(key=[seed, 77]))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def relerr(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def guarded(dev, shape, init=None, dtype=F32, lead=0, tail=0):
    """(buffer, view): `view` of `shape` inside a sentinel-filled buffer, GUARD + lead elements in (lead = 1: one float past
    16-byte alignment), GUARD + tail elements behind it; the view starts as `init` (a CPU tensor or a number; default NaN)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + lead + n + GUARD + tail,), SENT, dtype=dtype, device=dev)
    view = buf[GUARD + lead:GUARD + lead + n].view(*shape)
    if isinstance(init, torch.Tensor):
        view.copy_(init.to(dtype))
    else:
        view.fill_(NAN if init is None else init)
    assert view.data_ptr() % 16 == (4 * lead) % 16 or dtype != F32
    return buf, view


def assert_intact(buf, view, what):
    off, n = view.storage_offset(), view.numel()
    assert bool((buf[:off] == SENT).all()), f"{what}: wrote in front of the output"
    assert bool((buf[off + n:] == SENT).all()), f"{what}: wrote behind the output"


class Slot:
    """The middle one of three max |v| slots of the package's arena; `start` = its value on entry."""

    def __init__(self, ops, dev, start=0):
        self.three, self.start = ops.amax_slot(dev, 3), start
        if start:
            self.three[1:2].fill_(start)
        self.view = self.three[1:2]

    def check(self, out, what):
        torch.cuda.synchronize()
        a, s, b = (int(v) for v in self.three.tolist())
        assert a == 0 and b == 0, f"{what}: neighbouring slots written"
        if self.start:
            assert s == self.start, f"{what}: a slot holding a larger value must keep it ({s:#x} != {self.start:#x})"
        else:
            want = int(out.abs().max().view(torch.int32).item())
            assert s == want, f"{what}: slot {s:#x} != bits of max |out| {want:#x}"


def slot_modes(ops, dev):
    """(name, Slot or None): no slot, a zeroed one, one pre-filled with a larger value."""
    return (("noslot", None), ("slot", Slot(ops, dev)), ("slot_big", Slot(ops, dev, BIG)))


def sptr(slot):
    return slot.view.data_ptr() if slot is not None else None


def refused(RacError, fn, message):
    """`fn` must raise the package's error from the host check whose message holds `message` (no launch)."""
    with pytest.raises(RacError) as e:
        fn()
    assert message in str(e.value), str(e.value)
    torch.cuda.synchronize()


class Rule:
    """Collects (name, e_gpu, e_cpu32) of one test, prints each, and fails at the end with every miss of the rule."""

    def __init__(self, label, floor=2e-6):
        self.label, self.floor, self.rows = label, floor, []

    def check(self, name, got, ref64, ref32):
        got = got.detach().cpu()
        assert got.shape == ref64.shape, (self.label, name, tuple(got.shape), tuple(ref64.shape))
        e_gpu, e_cpu = relerr(got, ref64), relerr(ref32, ref64)
        if not bool(torch.isfinite(got).all()):
            e_gpu = float("nan")
        print(f"[{self.label}] {name}: e_gpu {e_gpu:.2e} e_cpu32 {e_cpu:.2e}")
        self.rows.append((name, e_gpu, e_cpu))

    def done(self):
        bad = [(n, f"e_gpu {g:.2e}", f"e_cpu32 {c:.2e}") for n, g, c in self.rows if not g <= max(self.floor, 4 * c)]
        worst = max(self.rows, key=lambda r: (r[1] != r[1], r[1]))
        print(f"[{self.label}] WORST {worst[0]}: e_gpu {worst[1]:.2e} e_cpu32 {worst[2]:.2e} ({len(self.rows)} tensors)")
        assert not bad, (self.label, bad)
