"""tests/bn_refs.py, the references of tests/test_gpu_vgg_block.py, against torch's own operators and autograd in fp64 on the
CPU: before a kernel is compared with them, they are shown to be BatchNorm, LeakyReLU, max pool and upsample."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_refs as br
from tests import test_gpu_vgg_block as gpu
from tests.fp64_tools import F32, F64, relerr, rnd

EPS = 1e-5
TOL = 1e-11


@pytest.mark.parametrize("G,Mg,C", [(1, 37, 64), (3, 203, 64), (3, 5, 6), (1, 37, 1024), (3, 37, 96)])
def test_chain_equals_fp64_autograd(G, Mg, C):
    """finalize + affine_act(leaky) + bwd_sums + bwd_apply in fp64 = F.batch_norm(training) + F.leaky_relu(0.2) per group and
    their autograd, to 1e-11 relative: y, dx, dgamma, dbeta.  The fp32 variant of the same formulas is the same to 2e-5."""
    x, dy, gamma, beta = br.make_inputs(3, G, Mg, C)
    want = br.autograd_chain(x, dy, gamma, beta, G, EPS)
    got = br.chain(x, dy, gamma, beta, G, EPS, F64)
    got32 = br.chain(x, dy, gamma, beta, G, EPS, F32)
    for name, g, g32, w in zip(("y", "dx", "dgamma", "dbeta"), got, got32, want):
        assert g.dtype == F64 and g32.dtype == F32 and g.shape == w.shape == g32.shape, name
        assert relerr(g, w) < TOL, (name, relerr(g, w))
        print(f"G{G} Mg{Mg} C{C} {name}: fp64 {relerr(g, w):.1e} fp32 {relerr(g32, w):.1e}")
        assert relerr(g32, w) < 2e-5, (name, relerr(g32, w))  # (a sanity bound: the same formulas, not another operation)


@pytest.mark.parametrize("n_updates", [0, 1, 2])
@pytest.mark.parametrize("G", [1, 3])
def test_running_statistics_equal_batch_norms(G, n_updates):
    """The running statistics of finalize = F.batch_norm's own after n_updates calls per group, in group order; with
    n_updates = 0 and with rm = None nothing is updated; scale / shift / mean / invstd do not depend on either."""
    Mg, C = 37, 12
    x, dy, gamma, beta = br.make_inputs(4, G, Mg, C)
    rm0, rv0 = rnd(1, C).double(), 1.0 + 0.5 * rnd(2, C).double().abs()
    rm, rv = rm0.clone(), rv0.clone()
    br.autograd_chain(x, dy, gamma, beta, G, EPS, rm, rv, 0.1, n_updates)
    out = br.finalize(br.stats_of(x, G), Mg, gamma, beta, rm0, rv0, 0.1, EPS, n_updates, G)
    assert relerr(out[4], rm) < TOL and relerr(out[5], rv) < TOL
    assert torch.equal(rm0, rnd(1, C).double()), "finalize wrote to its input"
    if n_updates == 0:
        assert torch.equal(out[4], rm0) and torch.equal(out[5], rv0)
    else:
        assert relerr(out[4], rm0) > 1e-3 and relerr(out[5], rv0) > 1e-3
    none = br.finalize(x, Mg, gamma, beta, None, None, 0.1, EPS, n_updates, G)
    assert none[4] is None and none[5] is None
    for a, b in zip(out[:4], none[:4]):
        assert torch.equal(a, b) and a.shape == (G, C)


def test_finalize_edges():
    """count = 1: var = 0, invstd = 1 / sqrt(eps), and the running variance takes the biased variance (0); a constant
    channel: var clamped at 0, never negative under the root."""
    C = 5
    x = rnd(5, 3, C)
    gamma, beta = torch.ones(C), torch.zeros(C)
    sc, sh, mu, istd, rm, rv = br.finalize(x, 1, gamma, beta, torch.zeros(C), torch.ones(C), 0.1, EPS, 1, 3)
    assert torch.equal(istd, torch.full((3, C), 1.0 / np.sqrt(EPS), dtype=F64)) and torch.equal(mu, x.double())
    assert relerr(rv, torch.full((C,), 0.9 ** 3, dtype=F64)) < TOL
    xc = torch.full((37, C), 0.1)
    istd = br.finalize(xc, 37, gamma, beta, None, None, 0.1, EPS, 1, 1)[3]
    assert bool(torch.isfinite(istd).all()) and relerr(istd, torch.full((1, C), 1.0 / np.sqrt(EPS), dtype=F64)) < 1e-9


@pytest.mark.parametrize("act", [br.ACT_NONE, br.ACT_LEAKY, br.ACT_SIGMOID])
def test_affine_act_is_torchs(act):
    G, Mg, C = 3, 7, 6
    x, sc, sh = rnd(6, G * Mg, C).double(), rnd(7, G, C).double(), rnd(8, G, C).double()
    z = torch.cat([x[g * Mg:(g + 1) * Mg] * sc[g] + sh[g] for g in range(G)])
    want = {br.ACT_NONE: z, br.ACT_LEAKY: F.leaky_relu(z, 0.2), br.ACT_SIGMOID: torch.sigmoid(z)}[act]
    assert torch.equal(br.affine_act(x, sc, sh, act, G), want)
    assert br.affine_act(x, sc, sh, act, G, F32).dtype == F32


def test_bwd_sums_fp32_adds_rows_in_index_order():
    G, Mg, C = 2, 9, 4
    x, dy, gamma, beta = br.make_inputs(5, G, Mg, C)
    aff = br.finalize(x, Mg, gamma, beta, None, None, 0.1, EPS, 0, G, F32)[:4]
    dz, xh = br._dz_xhat(dy, x, *aff, G, F32)
    acc = torch.zeros(G, C)
    for r in range(Mg):
        acc = acc + dz[:, r]
    assert torch.equal(br.bwd_sums(dy, x, *aff, G, F32)[:, 0], acc)


def test_fp32_statistics_follow_the_kernels_row_blocks():
    """stats_of in fp32: the row blocks of rac_col_stats' host code (16 rows at (203, 64), 13 at (37, 1024), one block of 5),
    fp32 inside a block only: against the fp64 sums the error is that of 16 fp32 additions, not of 203."""
    assert [br.col_stats_rows_per_block(*s) for s in ((203, 64), (37, 1024), (5, 6), (4100, 64))] == [16, 13, 5, 16]
    for G, Mg, C in gpu.CHAIN_CASES:
        x = br.make_inputs(gpu.SEED, G, Mg, C)[0]
        s64, s32 = br.stats_of(x, G), br.stats_of(x, G, F32)
        assert s32.dtype == F64 and s32.shape == s64.shape == (G, 2, C)
        for g in range(G):
            for k in range(2):
                assert 0 < relerr(s32[g, k], s64[g, k]) < 2e-7, (G, Mg, C, g, k, relerr(s32[g, k], s64[g, k]))
    x = rnd(20, 8, 3)  # one block of 8 rows: lanes (0, 4), (1, 5), (2, 6), (3, 7), then the tree
    want = ((x[0] + x[4]) + (x[1] + x[5])) + ((x[2] + x[6]) + (x[3] + x[7]))
    assert torch.equal(br.stats_of(x, 1, F32)[0, 0], want.double())


def test_make_inputs_reaches_its_margin_on_every_gpu_case():
    """Every (G, Mg, C) of the GPU module's case tables: make_inputs converges within its 10 rounds, min |z| >= 1e-2 in fp64,
    and the groups' means stay about 3 apart."""
    cases = gpu.bn_input_cases()
    assert len(cases) >= 50 and (3, 1030, 1024) in cases and (1, 5, 6) in cases and (1, 4200, 128) in cases
    worst = 0
    for G, Mg, C in cases:
        (x, dy, gamma, beta), rounds = br.make_inputs_rounds(gpu.SEED, G, Mg, C)
        worst = max(worst, rounds)
        assert x.dtype == dy.dtype == F32 and x.shape == dy.shape == (G * Mg, C) and gamma.shape == beta.shape == (C,)
        assert br.min_abs_z(x, gamma, beta, G) >= br.MARGIN, (G, Mg, C)
        if G > 1:
            means = x.view(G, Mg, C).mean((1, 2))
            assert float((means[1:] - means[:-1]).min()) > 2.0, (G, Mg, C)
    print(f"make_inputs: {len(cases)} cases, at most {worst} rounds")
    assert worst <= br.MAX_ROUNDS


def pool_maps():
    for form, (C, _, _) in gpu.MAP_FORMS.items():
        if not form.startswith("big"):
            for B, H, W in gpu.POOL_MAPS["small"]:
                yield B, H, W, C


def test_maxpool_references_are_torchs_also_on_ties():
    """maxpool2_fwd / maxpool2_bwd = F.max_pool2d(2, 2) and its autograd in fp64 on continuous maps and on maps of
    {-1, 0, 1}, where the gradient goes to the first maximum in scan order; the tie maps of the GPU module are tie-rich."""
    for B, H, W, C in list(pool_maps()) + [(2, 6, 10, 3)]:
        for kind, x in (("continuous", rnd(10, B, H, W, C)), ("ties", br.tie_map(gpu.TIE_SEED, B, H, W, C))):
            dy = rnd(11, B, H // 2, W // 2, C)
            y, dx = br.maxpool2_autograd(x, dy)
            assert torch.equal(br.maxpool2_fwd(x).double(), y), (kind, B, H, W, C)
            assert torch.equal(br.maxpool2_bwd(x, dy).double(), dx), (kind, B, H, W, C)
            assert int((dx != 0).sum()) == dy.numel()
            n = br.maxima_per_window(x)
            assert (n > 1.4) if kind == "ties" else (n == 1.0), (kind, B, H, W, C, n)
    x = torch.zeros(1, 2, 2, 1)  # an all-equal window: the gradient goes to element (0, 0)
    assert torch.equal(br.maxpool2_bwd(x, torch.ones(1, 1, 1, 1)).view(-1), torch.tensor([1.0, 0.0, 0.0, 0.0]))


def test_upsample_references_are_torchs():
    for B, h, w in gpu.UPSAMPLE_MAPS["small"] + [(2, 5, 3)]:
        for C in (6, 8):
            x, dy = rnd(12, B, h, w, C), rnd(13, B, 2 * h, 2 * w, C)
            y, dx = br.upsample2_autograd(x, dy)
            assert torch.equal(br.upsample2_fwd(x).double(), y)
            assert relerr(br.upsample2_bwd(dy, F64), dx) < TOL
            d32 = br.upsample2_bwd(dy, F32)
            assert d32.dtype == F32 and torch.equal(d32, (dy[:, ::2, ::2] + dy[:, ::2, 1::2]) + (dy[:, 1::2, ::2] + dy[:, 1::2, 1::2]))
