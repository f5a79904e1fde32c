"""Plain torch restatements, on the CPU, of the vgg block's BatchNorm chain, 2x2 max pool and nearest x2 upsample with the
semantics of include/rac_hip.h: the references of tests/test_gpu_vgg_block.py, validated against torch's own operators and
autograd in tests/test_bn_refs_host.py.

Maps are [M][C] rows (pool / upsample: [B][H][W][C]); the M rows are G equal row ranges of Mg rows, each one BatchNorm call.
stats / sums are [G][2][C], scale / shift / mean / invstd are [G][C].

Every function takes `dtype`: torch.float64 is the reference, torch.float32 the same formula in the kernels' precision (the
e_cpu32 side of the pass rule of tests/fp64_tools.py).  Where the C ABI itself hands a quantity over in fp64 (stats, sums)
and the kernels do that part of the arithmetic in fp64 before they round, the fp32 variants of finalize and bwd_apply do so
too: their error is then the fp32 part's alone, which makes the rule's bound tighter than an all-fp32 formula would.  The
fp32 variant of stats_of follows rac_col_stats' own summation order (fp32 inside a row block, fp64 across the blocks)."""
import numpy as np
import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
ACT_NONE, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2
MARGIN = 1e-2           # every pre-activation z of make_inputs has |z| >= MARGIN
MAX_ROUNDS = 10


def col_stats_rows_per_block(Mg, C):
    """Rows per workgroup of rac_col_stats (reduce_grid in rac_pointwise.hip): about 1024 workgroups over the row blocks and
    the 64-channel groups, at least 16 rows each."""
    nb = max(1, 1024 // ((C + 63) // 64))
    nb = min(nb, (Mg + 15) // 16)
    return (Mg + nb - 1) // nb


def stats_of(x, G, dtype=F64):
    """rac_col_stats: [G][2][C] per-group column sums and sums of squares of [G * Mg][C] rows, as fp64 values.  fp32 follows
    the kernel's order: fp32 only inside a block of col_stats_rows_per_block rows -- four row lanes add rows l, l + 4, ... of
    the block in index order and are combined as (l0 + l1) + (l2 + l3) -- and fp64 across the blocks."""
    v = x.to(dtype).view(G, -1, x.shape[-1])
    if dtype == F64:
        return torch.stack([v.sum(1), (v * v).sum(1)], 1)
    Mg, C = v.shape[1], v.shape[2]
    rpb = col_stats_rows_per_block(Mg, C)
    total = torch.zeros(G, 2, C, dtype=F64)
    for r0 in range(0, Mg, rpb):
        blk = v[:, r0:min(r0 + rpb, Mg)]
        lanes = []
        for lane in range(4):
            a1, a2 = torch.zeros(G, C), torch.zeros(G, C)
            for r in range(lane, blk.shape[1], 4):
                a1 = a1 + blk[:, r]
                a2 = a2 + blk[:, r] * blk[:, r]
            lanes.append((a1, a2))
        for k in range(2):
            total[:, k] += ((lanes[0][k] + lanes[1][k]) + (lanes[2][k] + lanes[3][k])).double()
    return total


def finalize(stats, count, gamma, beta, rm, rv, momentum, eps, n_updates, G, dtype=F64):
    """rac_bn_finalize.  `stats` [G][2][C] (or the [G * count][C] rows themselves).  Returns (scale, shift, mean, invstd)
    as [G][C] and the new (rm, rv) (None where rm is None).  Biased variance clamped at 0; scale = gamma * invstd,
    shift = beta - mean * scale; the running statistics take the groups' updates in order, n_updates times each, with the
    unbiased variance var * count / (count - 1) (var when count == 1).  mean, var and invstd are formed in fp64 from the
    fp64 statistics and then rounded to `dtype`, as in the kernels."""
    if stats.dim() == 2:
        stats = stats_of(stats, G)
    stats = stats.double().view(G, 2, -1)
    mean64 = stats[:, 0] / count
    var64 = (stats[:, 1] / count - mean64 * mean64).clamp_min(0.0)
    invstd = (1.0 / torch.sqrt(var64 + eps)).to(dtype)
    mean = mean64.to(dtype)
    scale = gamma.to(dtype) * invstd
    shift = beta.to(dtype) - mean * scale
    unbiased = (var64 * count / (count - 1) if count > 1 else var64).to(dtype)
    if rm is None:
        return scale, shift, mean, invstd, None, None
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    mom = torch.tensor(momentum, dtype=dtype)
    for g in range(G):
        for _ in range(n_updates):
            rm = (1 - mom) * rm + mom * mean[g]
            rv = (1 - mom) * rv + mom * unbiased[g]
    return scale, shift, mean, invstd, rm, rv


def _rows(t, G, dtype):
    return t.to(dtype).view(G, -1, t.shape[-1])


def _cols(t, G, dtype):
    return t.to(dtype).view(G, 1, -1)


def affine_act(x, scale, shift, act, G, dtype=F64):
    """rac_affine_act: act(x * scale + shift), scale / shift [G][C]; act none, LeakyReLU(0.2) or sigmoid."""
    z = _rows(x, G, dtype) * _cols(scale, G, dtype) + _cols(shift, G, dtype)
    if act == ACT_LEAKY:
        z = torch.where(z > 0, z, 0.2 * z)
    elif act == ACT_SIGMOID:
        z = torch.sigmoid(z)
    else:
        assert act == ACT_NONE, act
    return z.view(x.shape)


def _dz_xhat(dy, x, scale, shift, mean, invstd, G, dtype):
    xv = _rows(x, G, dtype)
    z = xv * _cols(scale, G, dtype) + _cols(shift, G, dtype)
    d = _rows(dy, G, dtype)
    dz = torch.where(z > 0, d, 0.2 * d)
    xh = (xv - _cols(mean, G, dtype)) * _cols(invstd, G, dtype)
    return dz, xh


def bwd_sums(dy, x, scale, shift, mean, invstd, G, dtype=F64):
    """rac_bn_bwd_reduce: [G][2][C] = (sum dz, sum dz * xhat) over each group's rows, with z = x * scale + shift,
    dz = dy * (z > 0 ? 1 : 0.2), xhat = (x - mean) * invstd.  fp64: torch's sum; fp32: the rows added in index order."""
    dz, xh = _dz_xhat(dy, x, scale, shift, mean, invstd, G, dtype)
    p = dz * xh
    if dtype == F64:
        return torch.stack([dz.sum(1), p.sum(1)], 1)
    a1, a2 = dz[:, 0].clone(), p[:, 0].clone()
    for r in range(1, dz.shape[1]):
        a1 = a1 + dz[:, r]
        a2 = a2 + p[:, r]
    return torch.stack([a1, a2], 1)


def bwd_apply(dy, x, scale, shift, mean, invstd, sums, G, dgamma=None, dbeta=None, dtype=F64):
    """rac_bn_bwd_apply: dx = scale * (dz - sum_dz / Mg - xhat * sum_dzx / Mg); dgamma += sum over the groups of sum_dzx,
    dbeta += that of sum_dz (None: not computed).  `sums` is fp64 in the ABI: the two means and the groups' totals are
    formed in fp64 and then rounded to `dtype`, as in the kernels."""
    dz, xh = _dz_xhat(dy, x, scale, shift, mean, invstd, G, dtype)
    Mg = dz.shape[1]
    s = sums.double().view(G, 2, -1)
    m1, m2 = (s[:, 0] / Mg).to(dtype).unsqueeze(1), (s[:, 1] / Mg).to(dtype).unsqueeze(1)
    dx = (_cols(scale, G, dtype) * (dz - m1 - xh * m2)).view(x.shape)
    if dgamma is None:
        return dx, None, None
    return dx, dgamma.to(dtype) + s[:, 1].sum(0).to(dtype), dbeta.to(dtype) + s[:, 0].sum(0).to(dtype)


def chain(x, dy, gamma, beta, G, eps, dtype=F64):
    """stats_of + finalize + affine_act(leaky) + bwd_sums + bwd_apply from zero gradients: (y, dx, dgamma, dbeta)."""
    Mg = x.shape[0] // G
    sc, sh, mu, istd, _, _ = finalize(stats_of(x, G, dtype), Mg, gamma, beta, None, None, 0.0, eps, 0, G, dtype)
    y = affine_act(x, sc, sh, ACT_LEAKY, G, dtype)
    sums = bwd_sums(dy, x, sc, sh, mu, istd, G, dtype)
    zero = torch.zeros_like(gamma)
    dx, dgamma, dbeta = bwd_apply(dy, x, sc, sh, mu, istd, sums, G, zero, zero, dtype)
    return y, dx, dgamma, dbeta


def autograd_chain(x, dy, gamma, beta, G, eps, rm=None, rv=None, momentum=0.1, n_updates=1):
    """The same through torch in fp64: F.batch_norm(training=True) then F.leaky_relu(0.2), one call per group (n_updates
    calls where running statistics are given: they are updated in place, group by group), and autograd for the upstream
    gradient dy.  Returns (y, dx, dgamma, dbeta)."""
    xs = x.double().clone().requires_grad_(True)
    ga, be = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    outs = []
    for xg in xs.view(G, -1, x.shape[-1]):
        planes = xg.t().unsqueeze(0)  # [1][C][Mg]
        for _ in range(max(n_updates, 1) if rm is not None else 1):
            o = F.batch_norm(planes, rm if n_updates else None, rv if n_updates else None, ga, be, True, momentum, eps)
        outs.append(F.leaky_relu(o, 0.2).squeeze(0).t())
    y = torch.cat(outs, 0)
    y.backward(dy.double())
    return y.detach(), xs.grad, ga.grad, be.grad


def make_inputs(seed, G, Mg, C):
    """(x, dy, gamma, beta) of make_inputs_rounds."""
    return make_inputs_rounds(seed, G, Mg, C)[0]


def make_inputs_rounds(seed, G, Mg, C):
    """((x, dy [G * Mg][C], gamma, beta [C]) in fp32, rounds it took).  x has per-(group, channel) means (the groups 3 apart) and spreads in
    [0.5, 2); every pre-activation z = gamma * xhat + beta, computed in fp64 from the batch statistics of x itself, has
    |z| >= MARGIN, so that the LeakyReLU's choice of slope is not a matter of rounding (fp32 puts z about 1e-6 off): every
    x with |z| < MARGIN is moved by 0.1 spreads away from the kink, and the statistics taken again, until none is left.
    Raises if that takes more than MAX_ROUNDS rounds.  No element is ever left out of a comparison instead."""
    g = np.random.Generator(np.random.Philox(key=[seed, 78]))
    spread = torch.from_numpy(0.5 + 1.5 * g.random((G, 1, C))).float()
    centre = torch.from_numpy(0.5 * g.standard_normal((G, 1, C))).float() + 3.0 * torch.arange(G, dtype=F32).view(G, 1, 1)
    x = (centre + spread * torch.from_numpy(g.standard_normal((G, Mg, C), dtype=np.float32))).view(G * Mg, C).contiguous()
    dy = torch.from_numpy(g.standard_normal((G * Mg, C), dtype=np.float32))
    # |gamma| in [0.5, 1.5), a quarter of the channels negative: a move of 0.1 spreads always moves z by some 0.05 or more
    gamma = torch.from_numpy((0.5 + g.random(C)) * np.where(g.random(C) < 0.25, -1.0, 1.0)).float()
    beta = torch.from_numpy(0.3 * g.standard_normal(C)).float()
    eps = float(np.float32(1e-5))
    for rounds in range(MAX_ROUNDS + 1):
        sc, sh, _, _, _, _ = finalize(stats_of(x, G), Mg, gamma, beta, None, None, 0.0, eps, 0, G, F64)
        z = _rows(x, G, F64) * sc.unsqueeze(1) + sh.unsqueeze(1)
        near = z.abs() < MARGIN
        if not bool(near.any()):
            return (x, dy, gamma, beta), rounds
        away = torch.where(z >= 0, 1.0, -1.0) * torch.where(sc.unsqueeze(1) >= 0, 1.0, -1.0)  # the x direction that grows |z|
        x = torch.where(near, x.view(G, Mg, C) + (away * 0.1).float() * spread, x.view(G, Mg, C)).view(G * Mg, C).contiguous()
    raise RuntimeError(f"make_inputs({seed}, {G}, {Mg}, {C}): |z| < {MARGIN} left after {MAX_ROUNDS} rounds")


def min_abs_z(x, gamma, beta, G):
    """min |z| of make_inputs' data, in fp64."""
    sc, sh, _, _, _, _ = finalize(stats_of(x, G), x.shape[0] // G, gamma, beta, None, None, 0.0, float(np.float32(1e-5)), 0, G)
    return float((_rows(x, G, F64) * sc.unsqueeze(1) + sh.unsqueeze(1)).abs().min())


# ----------------------------------------------------------------------------------------------- pool / upsample, [B][H][W][C]
def _windows(x):
    """The four values of every 2x2 window in scan order (0,0), (0,1), (1,0), (1,1): [4][B][H/2][W/2][C]."""
    B, H, W, C = x.shape
    v = x.view(B, H // 2, 2, W // 2, 2, C)
    return torch.stack([v[:, :, 0, :, 0], v[:, :, 0, :, 1], v[:, :, 1, :, 0], v[:, :, 1, :, 1]], 0)


def tie_map(seed, *shape):
    """A map of values in {-1, 0, 1}: most 2x2 windows hold their maximum more than once."""
    g = np.random.Generator(np.random.Philox(key=[seed, 79]))
    return torch.from_numpy(g.integers(-1, 2, shape).astype(np.float32))


def maxima_per_window(x):
    """Mean number of elements of a 2x2 window that equal its maximum (1 = no ties)."""
    return float((_windows(x) == maxpool2_fwd(x)).double().sum(0).mean())


def maxpool2_fwd(x):
    w = _windows(x)
    return torch.maximum(torch.maximum(w[0], w[1]), torch.maximum(w[2], w[3]))


def maxpool2_bwd(x, dy):
    """dx: every window's dy goes to its first maximum in scan order, the other three elements get 0."""
    w = _windows(x)
    best, arg = w[0].clone(), torch.zeros(w[0].shape, dtype=torch.long)
    for k in range(1, 4):
        better = w[k] > best
        best, arg = torch.where(better, w[k], best), torch.where(better, torch.full_like(arg, k), arg)
    B, H, W, C = x.shape
    dx = torch.zeros(B, H // 2, 2, W // 2, 2, C, dtype=dy.dtype)
    for k in range(4):
        dx[:, :, k // 2, :, k % 2] = torch.where(arg == k, dy, torch.zeros_like(dy))
    return dx.view(B, H, W, C)


def upsample2_fwd(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def upsample2_bwd(dy, dtype=F64):
    """dx = (p00 + p01) + (p10 + p11) of every 2x2 block of dy, in that association."""
    w = _windows(dy.to(dtype))
    return (w[0] + w[1]) + (w[2] + w[3])


def to_planes(x):
    """[B][H][W][C] -> torch's [B][C][H][W]."""
    return x.permute(0, 3, 1, 2).contiguous()


def from_planes(x):
    return x.permute(0, 2, 3, 1).contiguous()


def maxpool2_autograd(x, dy):
    """(y, dx) of F.max_pool2d(2, 2) and its autograd in fp64, as [B][H][W][C] maps."""
    xp = to_planes(x.double()).requires_grad_(True)
    y = F.max_pool2d(xp, 2, 2)
    y.backward(to_planes(dy.double()))
    return from_planes(y.detach()), from_planes(xp.grad)


def upsample2_autograd(x, dy):
    xp = to_planes(x.double()).requires_grad_(True)
    y = F.interpolate(xp, scale_factor=2, mode="nearest")
    y.backward(to_planes(dy.double()))
    return from_planes(y.detach()), from_planes(xp.grad)
