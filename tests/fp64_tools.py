"""Test helpers of the kernel-vs-fp64 modules (test_gpu_norm_cell.py, test_gpu_reduce.py): seeded inputs, the relative error
they all use, and the tolerance rule

    e_gpu <= max(floor, 4 * e_cpu32),    floor = 2e-6 unless a test says otherwise

with e_gpu = relerr(kernel, fp64 reference) and e_cpu32 = relerr(the same formula in fp32 on the CPU with torch, the same
fp64 reference).  Every case prints both figures; nothing is excluded."""
import numpy as np
import torch


def rnd(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.Philox(key=[seed, 77]))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def relerr(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


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
