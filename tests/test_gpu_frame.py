"""The kernels at the model's boundary -- frame packing, compositing, the reconstruction and KL losses, PSNR / SSIM, the CEM
step tail (csrc/rac_frame.hip) and pool / upsample / tilecat / reparam (csrc/rac_pointwise.hip) -- driven through the C ABI
(include/rac_hip.h) and compared with plain torch on the CPU (tests/frame_refs.py: the oracle's expressions, shown to be
the reference project's by tests/test_frame_refs_host.py), in fp64 and in fp32, at the shapes where each launch form and
each edge of a formula is reached.

Pass rule (tests/fp64_tools.py): e_gpu <= max(2e-6, 4 * e_cpu32) for arithmetic results; torch.equal for pure copies and
selections (bit patterns where a sign or a NaN is part of the answer); a max |v| slot as in test_gpu_reduce.py.  Every case
prints its figures; nothing is excluded.  Every float output is a view inside a sentinel-filled buffer that must survive
on both sides; outputs start as NaN, `+=` outputs start non-zero.

Kernel and form reached, by case (shape or alignment alone, never the environment):

  entry point, case                                    kernel and form
  ---------------------------------------------------  ----------------------------------------------------------------
  pack_input / unpack_grad (2,8,12) (3,24,40) (1,16,16) pack_input_kernel / unpack_grad_kernel, one pass; zmask NULL | given,
                                                       Cm 0 / 1 / 2 / 5, pad 0 / 1 / 3; unpack at C 4 and 8
  pack_input / unpack_grad (130,64,64)                 the same kernels, 532 480 pixels: second pass of the 2048-workgroup loop
  zero_region (2,24,40) | (43,64,64)                   zero_region_kernel, one pass | 528 384 values: wrapped loop
  composite fwd / bwd (2,24,40) (1,16,16) | (130,64,64) composite_fwd_kernel / composite_bwd_kernel (dprev given | NULL), one pass
                                                       | wrapped loop
  recon_loss (3,24,40)                                 recon_loss_sample_kernel with HW 960 = 3.75 strides of its 256 threads
  recon_loss (1,16,16)                                 one workgroup, one stride; B 1: the final kernel's one live thread
  recon_loss (260,16,16)                               recon_loss_final_kernel: B above its 256 threads (second stride)
  recon_loss bwd, every shape                          recon_loss_bwd_kernel, one pass (the largest is 199 680 values)
  kl n 30 / 2560 | 70 000                              kl_fwd_kernel 1 / 10 workgroups | 256 workgroups of 256 threads, wrapped;
                                                       kl_final_kernel; kl_bwd_kernel one pass
  psnr_ssim (1,16,16) (2,64,64)                        psnr_ssim_kernel, whole 16 x 16 tiles (1 | 16 per plane)
  psnr_ssim (2,24,40) (3,21,35)                        ragged last tile on one | both axes; mask NULL | given, map NULL | given
  cem_step_tail (5,24,40) (3,64,64)                    cem_step_tail_kernel, HW 960 (ragged stride) | 4096; kind 0 | 1, cost_mask
                                                       / goal_mask given or NULL, next_mask NULL | given, add_cost 0 | 1
  maxpool2 fwd C 12 | C 6, or one float in             maxpool2_fwd_kernel<f32x4> | <float>
  maxpool2 fwd (33,64,64,64) | (9,64,64,64) one float in  <f32x4> | <float>, wrapped loop (the 16-byte form wraps only above
                                                       524 288 output quads: forward only, 34 MB in)
  maxpool2 bwd, every case | (9,64,64,64)              maxpool2_bwd_kernel (always element-indexed) | wrapped loop; ties
  upsample2 fwd / bwd C 8 | C 6, or one float in       upsample2_*_kernel<f32x4> | <float>
  upsample2 (9,32,32,64) aligned                       fwd <f32x4> wrapped loop (589 824 quads); bwd <f32x4> one pass
  upsample2 (9,32,32,64) one float in                  fwd and bwd <float>, wrapped loop
  tilecat 3 x 48, three slot modes | per image         tilecat_kernel | tilecat_image_kernel
  tilecat 40 x 1024                                    tilecat_kernel: no slot wraps the 2048-workgroup loop, a slot the
                                                       512-workgroup loop; tilecat_image_kernel 96 .. 128 strides per image
  reparam fwd / bwd n 37 | 2048 * 256 + 300            reparam_fwd_kernel / reparam_bwd_kernel, one pass | wrapped loop
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import frame_refs as fr  # noqa: E402
from tests.fp64_tools import F32, F64, Rule, assert_intact, guarded, rnd, slot_modes, sptr  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rac(dev):
    """(ops, call, ptr, stream_ptr) of the package."""
    from robot_aware_control_amd import ops
    return ops, ops.call, ops.ptr, ops.stream_ptr


def uniform(seed, *shape):
    """fp32 uniform on [0, 1), seeded like fp64_tools.rnd."""
    return torch.from_numpy(np.random.Generator(np.random.Philox(key=[seed, 77])).random(shape, dtype=np.float32))


def same_bits(got, want):
    """Equal bit patterns, NaN matching any NaN (the sign of 0 counts; a NaN's sign and payload do not)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape:
        return False
    nan = want.isnan()
    return bool((got.isnan() == nan).all()) and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])


def robot_mask(seed, N, H, W, thresh=0.3):
    return (rnd(seed, N, 1, H, W) > thresh).float()


def plant_specials(img, zmask):
    """A -0.0 and an inf in two pixels of `img` that `zmask` zeroes: v * 0 keeps the sign and turns inf into NaN."""
    idx = zmask[:, 0].nonzero()
    assert len(idx) >= 2
    (b0, y0, x0), (b1, y1, x1) = idx[0].tolist(), idx[-1].tolist()
    img[b0, 0, y0, x0] = -0.0
    img[b1, 1, y1, x1] = float("inf")
    img[b1, 2, y1, x1] = -3.0  # a negative value becomes -0.0 too
    return img


def x4_planes(seed, N, H, W):
    """[rgb | m] planes of a decoder output: sigmoid values, the mask channel exactly 0 and exactly 1 in some pixels."""
    x4 = torch.sigmoid(rnd(seed, N, 4, H, W))
    m = x4[:, 3].reshape(-1).clone()
    m[::7], m[3::11] = 0.0, 1.0
    x4[:, 3] = m.view(N, H, W)
    assert int((x4[:, 3] == 0).sum()) > 0 and int((x4[:, 3] == 1).sum()) > 0
    return x4


# =========================================================================== 1. frame packing and compositing
PACK_CASES = [(2, 8, 12, 0, 1, False), (3, 24, 40, 2, 3, True), (1, 16, 16, 5, 0, True), (130, 64, 64, 1, 0, True)]


@pytest.mark.parametrize("B,H,W,Cm,pad,with_z", PACK_CASES)
def test_pack_input_and_unpack_grad(dev, rac, B, H, W, Cm, pad, with_z):
    """rac_pack_input: packed[b][p] = [img * 0 where zmask, else img | mask | 0], the same bits as the torch expression,
    a -0.0 and an inf among the zeroed pixels; rac_unpack_grad at C = 4 and 8: the first 3 channels, 0 where zmask."""
    ops, call, ptr, stream = rac
    img = rnd(1, B, 3, H, W)
    zmask = robot_mask(2, B, H, W) if with_z else None
    if with_z:
        plant_specials(img, zmask)
    mask = (rnd(3, B, Cm, H, W) > 0).float() if Cm else None
    want = fr.to_map(fr.pack_input(img, zmask, mask, pad))
    if with_z:
        assert bool(want.isnan().any()) and bool((want.view(torch.int32) == -2 ** 31).any())
    img_d, z_d, m_d = img.to(dev), None if zmask is None else zmask.to(dev), None if mask is None else mask.to(dev)
    C = 3 + Cm + pad
    obuf, out = guarded(dev, (B, H, W, C))
    call("rac_pack_input", ptr(img_d), ptr(z_d), ptr(m_d), Cm, pad, ptr(out), B, H * W, stream())
    torch.cuda.synchronize()
    assert same_bits(out, want), "pack_input"
    assert_intact(obuf, out, "pack_input")
    for Cg in (4, 8):
        dpacked = rnd(4 + Cg, B, H, W, Cg)
        dp_d = dpacked.to(dev)
        gbuf, dimg = guarded(dev, (B, 3, H, W))
        call("rac_unpack_grad", ptr(dp_d), Cg, ptr(z_d), ptr(dimg), B, H * W, stream())
        torch.cuda.synchronize()
        assert torch.equal(dimg.cpu(), fr.unpack_grad(fr.from_map(dpacked), zmask)), f"unpack_grad C{Cg}"
        assert_intact(gbuf, dimg, f"unpack_grad C{Cg}")


@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (43, 64, 64)])
def test_zero_region(dev, rac, B, H, W):
    """rac_zero_region on B x 3 x HW: img * 0 where the mask is set (the sign stays, inf gives NaN), img elsewhere."""
    ops, call, ptr, stream = rac
    mask = robot_mask(10, B, H, W)
    img = plant_specials(rnd(11, B, 3, H, W), mask)
    want = fr.zero_region(mask, img)
    assert bool(want.isnan().any()) and bool((want.view(torch.int32) == -2 ** 31).any())
    img_d, m_d = img.to(dev), mask.to(dev)
    obuf, out = guarded(dev, (B, 3, H, W))
    call("rac_zero_region", ptr(img_d), ptr(m_d), ptr(out), B, H * W, stream())
    torch.cuda.synchronize()
    assert same_bits(out, want)
    assert_intact(obuf, out, "zero_region")


def composite_bwd_ref(x4, prev, dout, dt):
    a, p = x4.to(dt).clone().requires_grad_(True), prev.to(dt).clone().requires_grad_(True)
    return torch.autograd.grad((fr.composite(a, p) * dout.to(dt)).sum(), [a, p])


@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (1, 16, 16), (130, 64, 64)])
def test_composite_vs_fp64(dev, rac, B, H, W):
    """rac_composite_fwd: (1 - m) prev + m rgb with m exactly 0 and 1 in places; rac_composite_bwd: dx4 = [dout m | sum_c
    dout_c (rgb_c - prev_c)] and dprev = dout (1 - m) against fp64 autograd, with dprev given and NULL."""
    ops, call, ptr, stream = rac
    rule = Rule(f"f1 composite B{B} {H}x{W}")
    x4, prev, dout = x4_planes(20, B, H, W), torch.sigmoid(rnd(21, B, 3, H, W)), rnd(22, B, 3, H, W)
    x4_d, prev_d, dout_d = fr.to_map(x4).to(dev), prev.to(dev), dout.to(dev)
    obuf, out = guarded(dev, (B, 3, H, W))
    call("rac_composite_fwd", ptr(x4_d), ptr(prev_d), ptr(out), B, H * W, stream())
    torch.cuda.synchronize()
    rule.check("fwd", out, fr.composite(x4.double(), prev.double()), fr.composite(x4, prev))
    assert_intact(obuf, out, "fwd")
    (dx64, dp64), (dx32, dp32) = composite_bwd_ref(x4, prev, dout, F64), composite_bwd_ref(x4, prev, dout, F32)
    for with_dprev in (True, False):
        what = f"bwd dprev{int(with_dprev)}"
        xbuf, dx4 = guarded(dev, (B, H, W, 4))
        pbuf, dprev = guarded(dev, (B, 3, H, W), 7.0)
        call("rac_composite_bwd", ptr(dout_d), ptr(x4_d), ptr(prev_d), ptr(dx4), ptr(dprev) if with_dprev else None, B,
             H * W, stream())
        torch.cuda.synchronize()
        rule.check(f"{what} dx4", dx4, fr.to_map(dx64), fr.to_map(dx32))
        if with_dprev:
            rule.check(f"{what} dprev", dprev, dp64, dp32)
        else:
            assert bool((dprev == 7.0).all()), "dprev = NULL: a buffer that was not passed was written"
        assert_intact(xbuf, dx4, what + " dx4")
        assert_intact(pbuf, dprev, what + " dprev")
    rule.done()


# =========================================================================== 2. losses
def recon_masks(B, H, W):
    """Mask sets with an all-world (count of robot values 0) and an all-robot (count of world values 0) sample: one set
    with samples 0 and 1 of those kinds and the rest random; with B = 1 two sets."""
    if B == 1:
        return [torch.zeros(1, 1, H, W), torch.ones(1, 1, H, W)]
    mask = robot_mask(30, B, H, W)
    mask[0], mask[1] = 0.0, 1.0
    assert 0 < float(mask[2:].mean()) < 1
    return [mask]


@pytest.mark.parametrize("B,H,W", [(3, 24, 40), (1, 16, 16), (260, 16, 16)])
@pytest.mark.parametrize("kind", fr.LOSS_NAMES)
def test_recon_loss_vs_fp64(dev, rac, kind, B, H, W):
    """rac_recon_loss_fwd out[0..2] = [loss, robot_mse, world_mse] and rac_recon_loss_bwd's dpred (against fp64 autograd with
    gout = 1.7), batch_weight NULL and given, robot_weight 0 and 0.5, a sample without robot pixels and one without world
    pixels (the `count + 1` divisors), and for l1 / mse mask = NULL, where the two metrics are exactly 0."""
    ops, call, ptr, stream = rac
    rule = Rule(f"f2 recon_loss {kind} B{B} {H}x{W}")
    pred, target = torch.sigmoid(rnd(31, B, 3, H, W)), torch.sigmoid(rnd(32, B, 3, H, W))
    assert bool((target != pred).all())  # no l1 sign is ambiguous
    bw = rnd(33, B).abs() + 0.5
    gout = torch.tensor([1.7])
    pred_d, target_d, bw_d, gout_d = pred.to(dev), target.to(dev), bw.to(dev), gout.to(dev)
    dontcare = kind.startswith("dontcare")
    masks = recon_masks(B, H, W) + ([] if dontcare else [None])
    for mi, mask in enumerate(masks):
        mask_d = None if mask is None else mask.to(dev)
        for rw in ((0.0, 0.5) if dontcare else (0.0,)):
            for with_bw in (False, True):
                what = f"mask{'NULL' if mask is None else mi} rw{rw} bw{int(with_bw)}"

                def ref(dt):
                    p = pred.to(dt).clone().requires_grad_(True)
                    out = fr.recon_out(kind, p, target.to(dt), None if mask is None else mask.to(dt), rw,
                                       bw.to(dt) if with_bw else None)
                    (dp,) = torch.autograd.grad(out[0] * gout.to(dt)[0], [p])
                    return out.detach(), dp

                (o64, d64), (o32, d32) = ref(F64), ref(F32)
                sbuf, per = guarded(dev, (B, 8))
                obuf, out = guarded(dev, (3,))
                call("rac_recon_loss_fwd", ops.LOSS_KINDS[kind], ptr(pred_d), ptr(target_d), ptr(mask_d), rw,
                     ptr(bw_d) if with_bw else None, ptr(per), ptr(out), B, H * W, stream())
                gbuf, dpred = guarded(dev, (B, 3, H, W))
                call("rac_recon_loss_bwd", ops.LOSS_KINDS[kind], ptr(pred_d), ptr(target_d), ptr(mask_d), rw,
                     ptr(bw_d) if with_bw else None, ptr(per), ptr(gout_d), ptr(dpred), B, H * W, stream())
                torch.cuda.synchronize()
                rule.check(f"{what} loss", out[0:1], o64[0:1], o32[0:1])
                if mask is None:
                    assert float(out[1]) == 0.0 and float(out[2]) == 0.0, f"{what}: metrics without a mask must be 0"
                else:
                    rule.check(f"{what} robot_mse", out[1:2], o64[1:2], o32[1:2])
                    rule.check(f"{what} world_mse", out[2:3], o64[2:3], o32[2:3])
                rule.check(f"{what} dpred", dpred, d64, d32)
                assert_intact(sbuf, per, what + " per_sample")
                assert_intact(obuf, out, what + " out")
                assert_intact(gbuf, dpred, what + " dpred")
    rule.done()


@pytest.mark.parametrize("n,bs", [(30, 3), (4 * 10 * 8 * 8, 4), (70000, 7)])
def test_kl_vs_fp64(dev, rac, n, bs):
    """rac_kl_fwd / rac_kl_bwd with logvars of standard deviation 1.5 against the fp64 formula and its autograd (gout 0.6);
    a second forward into the same `partial` (left non-zero by the first) gives the same bits."""
    ops, call, ptr, stream = rac
    rule = Rule(f"f2 kl n{n} bs{bs}")
    cpu = [rnd(40, bs, n // bs), rnd(41, bs, n // bs) * 1.5, rnd(42, bs, n // bs), rnd(43, bs, n // bs) * 1.5]
    gout = torch.tensor([0.6])
    d = [t.to(dev) for t in cpu]
    gout_d = gout.to(dev)

    def ref(dt):
        ts = [t.to(dt).clone().requires_grad_(True) for t in cpu]
        kl = fr.kl_loss(*ts, bs)
        return kl.detach().view(1), torch.autograd.grad(kl * gout.to(dt)[0], ts)

    (k64, g64), (k32, g32) = ref(F64), ref(F32)
    pbuf, partial = guarded(dev, (1,), dtype=F64)  # starts as NaN: the entry clears it
    obuf, out = guarded(dev, (1,))
    call("rac_kl_fwd", *[ptr(t) for t in d], n, bs, ptr(partial), ptr(out), stream())
    torch.cuda.synchronize()
    rule.check("fwd", out, k64, k32)
    first = out.clone()
    assert float(partial) != 0.0
    call("rac_kl_fwd", *[ptr(t) for t in d], n, bs, ptr(partial), ptr(out), stream())
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), "the second call depends on the first one's partial"
    assert_intact(pbuf, partial, "partial")
    assert_intact(obuf, out, "out")
    outs = [guarded(dev, (bs, n // bs)) for _ in range(4)]
    call("rac_kl_bwd", *[ptr(t) for t in d], ptr(gout_d), n, bs, *[ptr(v) for _, v in outs], stream())
    torch.cuda.synchronize()
    for name, (buf, v), r64, r32 in zip(("dmu1", "dlv1", "dmu2", "dlv2"), outs, g64, g32):
        rule.check(name, v, r64, r32)
        assert_intact(buf, v, name)
    rule.done()


# =========================================================================== 3. PSNR / SSIM
def image_pair(regime, N, H, W):
    if regime == "uniform":
        return uniform(50, N, 3, H, W), uniform(51, N, 3, H, W)
    if regime == "near":
        a = uniform(52, N, 3, H, W)
        return a, (a + 0.05 * rnd(53, N, 3, H, W)).clamp(0, 1)
    a = F.interpolate(uniform(54, N, 3, 3, 5), size=(H, W), mode="bilinear", align_corners=False).clamp(0, 1)
    return a, (a + 0.02 * rnd(55, N, 3, H, W)).clamp(0, 1)


@pytest.mark.parametrize("N,H,W", [(2, 24, 40), (1, 16, 16), (3, 21, 35), (2, 64, 64)])
def test_psnr_ssim_vs_fp64(dev, rac, N, H, W):
    """rac_psnr_ssim: the SSIM map, and sq_err / ssim_sum ADDED to non-zero accumulators, on three kinds of image pair,
    with and without mask and map; a fully masked sample has SSIM exactly 1 in every pixel and adds exactly 0 to sq_err.
    On (3, 21, 35) also metrics.masked_psnr_ssim, the form the trainer calls."""
    ops, call, ptr, stream = rac
    rule = Rule(f"f3 psnr_ssim N{N} {H}x{W}")
    start = torch.stack([rnd(56, N).abs() + 0.5, rnd(57, N).abs() * 10 + 1.0])
    for regime in ("uniform", "near", "smooth"):
        a, b = image_pair(regime, N, H, W)
        assert float(a.min()) >= 0 and float(a.max()) <= 1 and float(b.min()) >= 0 and float(b.max()) <= 1
        a_d, b_d = a.to(dev), b.to(dev)
        mask = robot_mask(58, N, H, W)
        mask[N - 1] = 1.0  # the last sample fully masked
        mask_d = mask.to(dev)
        for m, m_d in ((None, None), (mask, mask_d)):
            m64 = None if m is None else m.double()
            map64, se64, ss64 = fr.psnr_ssim(a.double(), b.double(), m64)
            map32, se32, ss32 = fr.psnr_ssim(a, b, m)
            for with_map in (False, True):
                what = f"{regime} mask{int(m is not None)} map{int(with_map)}"
                abuf, acc = guarded(dev, (2, N), start)
                mbuf, smap = guarded(dev, (N, 3, H, W))
                call("rac_psnr_ssim", ptr(a_d), ptr(b_d), ptr(m_d), ptr(acc[0]), ptr(acc[1]), ptr(smap) if with_map else None,
                     N, H, W, stream())
                torch.cuda.synchronize()
                rule.check(f"{what} sq_err", acc[0], start[0].double() + se64, start[0] + se32)
                rule.check(f"{what} ssim_sum", acc[1], start[1].double() + ss64, start[1] + ss32)
                if with_map:
                    rule.check(f"{what} ssim_map", smap, map64, map32)
                else:
                    assert bool(smap.isnan().all()), f"{what}: ssim_map = NULL, a buffer that was not passed was written"
                if m is not None:
                    assert float(acc[0, N - 1]) == float(start[0, N - 1]), f"{what}: a fully masked sample has sq_err 0"
                    if with_map:
                        assert bool((smap[N - 1] == 1.0).all()), f"{what}: a fully masked sample has SSIM 1"
                assert_intact(abuf, acc, what + " accumulators")
                assert_intact(mbuf, smap, what + " ssim_map")
        if (N, H, W) == (3, 21, 35):
            from robot_aware_control_amd import metrics
            psnr, ssim = metrics.masked_psnr_ssim(b_d, a_d, mask_d.view(N, 1, H, W))
            p64, s64 = fr.masked_psnr_ssim(b.double(), a.double(), mask.double())
            p32, s32 = fr.masked_psnr_ssim(b, a, mask)
            assert float(psnr[N - 1]) == float("inf") and float(p64[N - 1]) == float("inf")
            rule.check(f"{regime} masked_psnr_ssim psnr", psnr[:N - 1], p64[:N - 1], p32[:N - 1])
            rule.check(f"{regime} masked_psnr_ssim ssim", ssim.view(1), s64.view(1), s32.view(1))
    rule.done()


# =========================================================================== 4. CEM step tail
CEM_FORMS = [(0, False, False), (1, True, True), (1, True, False), (1, False, True)]  # (kind, cost_mask, goal_mask)


@pytest.mark.parametrize("N,H,W", [(5, 24, 40), (3, 64, 64)])
def test_cem_step_tail_vs_fp64(dev, rac, N, H, W):
    """rac_cem_step_tail over three chained steps (next_out feeds curr; sum_cost starts non-zero and accumulates; the middle
    step has add_cost = 0): next_out against the composite-then-zero formula on the kernel's own previous frame; sum_cost
    against start - sum_t weight * sqrt(sum (255 (next - goal))^2) [/ n_world] of the kernel's own next_out, added in fp64."""
    ops, call, ptr, stream = rac
    rule = Rule(f"f4 cem_step_tail N{N} {H}x{W}")
    HW, T = H * W, 3
    curr0, goal = torch.sigmoid(rnd(60, N, 3, H, W)), torch.sigmoid(rnd(61, 1, 3, H, W))
    x4s = [x4_planes(62 + t, N, H, W) for t in range(T)]
    nmasks = [robot_mask(66 + t, N, H, W, 0.6) for t in range(T)]
    cmasks = [robot_mask(70 + t, N, H, W, 0.4) for t in range(T)]
    gmask = rnd(74, 1, 1, H, W) > 0.5
    for cm in cmasks:
        cm[:, 0, 0, 0] = 0.0
    gmask[0, 0, 0, 0] = False  # pixel 0 of every candidate counts: n_world > 0
    for cm in cmasks:
        assert int((~(cm.bool() | gmask)).sum((1, 2, 3)).min()) > 0
    start = rnd(75, N).double() * 10.0
    goal_d, gmask_d = goal.to(dev), gmask.to(torch.uint8).to(dev)
    x4s_d, nmasks_d, cmasks_d = [fr.to_map(v).to(dev) for v in x4s], [v.to(dev) for v in nmasks], [v.to(dev) for v in cmasks]
    for kind, with_cm, with_gm in CEM_FORMS:
        for with_nm in (False, True):
            for weight in (1.0, 0.37):
                w32 = float(np.float32(weight))
                what = f"kind{kind} cm{int(with_cm)} gm{int(with_gm)} nm{int(with_nm)} w{weight}"
                sbuf, sum_cost = guarded(dev, (N,), start, dtype=F64)
                want64, want32 = start.clone(), start.clone()
                curr_d = curr0.to(dev)
                for t in range(T):
                    add = t != 1
                    nbuf, nxt = guarded(dev, (N, 3, H, W))
                    before = sum_cost.clone()
                    call("rac_cem_step_tail", ptr(x4s_d[t]), ptr(curr_d), ptr(nmasks_d[t]) if with_nm else None, ptr(goal_d),
                         ptr(cmasks_d[t]) if with_cm else None, ptr(gmask_d) if with_gm else None, kind, weight, int(add),
                         ptr(nxt), ptr(sum_cost), N, HW, stream())
                    torch.cuda.synchronize()
                    curr, nm = curr_d.cpu(), nmasks[t] if with_nm else None
                    rule.check(f"{what} step{t} next_out", nxt, fr.cem_next(x4s[t].double(), curr.double(), nm),
                               fr.cem_next(x4s[t], curr, nm))
                    assert_intact(nbuf, nxt, f"{what} step{t} next_out")
                    if add:
                        own = nxt.cpu()

                        def cost(dt):
                            if kind == 0:
                                return fr.img_l2_cost(own.to(dt), goal.to(dt))
                            return fr.img_dontcare_cost(own.to(dt), goal.to(dt), cmasks[t] if with_cm else None,
                                                        gmask if with_gm else None)

                        want64 = want64 + w32 * cost(F64)
                        want32 = want32 + (torch.tensor(weight, dtype=F32) * cost(F32)).double()
                        rule.check(f"{what} step{t} sum_cost", sum_cost, want64, want32)
                    else:
                        assert torch.equal(sum_cost.view(torch.int64), before.view(torch.int64)), \
                            f"{what}: add_cost = 0 changed sum_cost"
                    curr_d = nxt
                assert_intact(sbuf, sum_cost, what + " sum_cost")
    rule.done()


# =========================================================================== 5. pool / upsample
def int_levels(seed, *shape):
    """Floats drawn from {0, 1, 2}: most 2 x 2 windows hold their maximum more than once."""
    return torch.from_numpy(np.random.Generator(np.random.Philox(key=[seed, 77])).integers(0, 3, shape).astype(np.float32))


# (B, H, W, C, one float into the allocations, ties, backward too)
MAXPOOL_CASES = {"vec": (2, 8, 12, 12, 0, False, True), "scalar_C6": (2, 8, 12, 6, 0, False, True),
                 "scalar_misaligned": (2, 8, 12, 12, 1, False, True), "ties": (2, 8, 12, 12, 0, True, True),
                 "wrap_bwd": (9, 64, 64, 64, 0, False, True), "wrap_scalar_fwd": (9, 64, 64, 64, 1, False, False),
                 "wrap_vec_fwd": (33, 64, 64, 64, 0, False, False)}


@pytest.mark.parametrize("case", list(MAXPOOL_CASES))
def test_maxpool2_equals_torch(dev, rac, case):
    """rac_maxpool2_fwd equals F.max_pool2d and rac_maxpool2_bwd equals its CPU autograd, bit for bit; with inputs from
    {0, 1, 2} more than half of the windows tie and the gradient goes to the first maximum in scan order, as ATen's does."""
    ops, call, ptr, stream = rac
    B, H, W, C, lead, ties, bwd = MAXPOOL_CASES[case]
    x = int_levels(80, B, H, W, C) if ties else rnd(80, B, H, W, C)
    if ties:
        win = fr.from_map(x).view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
        assert float(((win == win.max(1, keepdim=True).values).sum(1) > 1).float().mean()) > 0.5
    xbuf, x_d = guarded(dev, (B, H, W, C), x, lead=lead)
    ybuf, y = guarded(dev, (B, H // 2, W // 2, C), lead=lead)
    call("rac_maxpool2_fwd", ptr(x_d), ptr(y), B, H, W, C, stream())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), fr.maxpool2(x)), "forward"
    assert_intact(ybuf, y, "forward")
    if not bwd:
        return
    dy = rnd(81, B, H // 2, W // 2, C)
    xp = fr.from_map(x).requires_grad_(True)
    (want,) = torch.autograd.grad((F.max_pool2d(xp, 2, 2) * fr.from_map(dy)).sum(), [xp])
    dbuf, dy_d = guarded(dev, dy.shape, dy, lead=lead)
    gbuf, dx = guarded(dev, (B, H, W, C), lead=lead)
    call("rac_maxpool2_bwd", ptr(x_d), ptr(dy_d), ptr(dx), B, H, W, C, stream())
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), fr.to_map(want)), "backward"
    assert_intact(gbuf, dx, "backward")
    assert_intact(xbuf, x_d, "input")


# (B, h, w, C, one float into the allocations)
UPSAMPLE_CASES = {"vec": (2, 4, 6, 8, 0), "scalar_C6": (2, 4, 6, 6, 0), "scalar_misaligned": (2, 4, 6, 8, 1),
                  "wrap_vec": (9, 32, 32, 64, 0), "wrap_scalar": (9, 32, 32, 64, 1)}


@pytest.mark.parametrize("case", list(UPSAMPLE_CASES))
def test_upsample2_vs_fp64(dev, rac, case):
    """rac_upsample2_fwd equals nearest-neighbour interpolation bit for bit; rac_upsample2_bwd, the sum of each 2 x 2 block of
    dy, under the rule."""
    ops, call, ptr, stream = rac
    B, h, w, C, lead = UPSAMPLE_CASES[case]
    rule = Rule(f"f5 upsample2 {case}")
    x, dy = rnd(82, B, h, w, C), rnd(83, B, 2 * h, 2 * w, C)
    xbuf, x_d = guarded(dev, x.shape, x, lead=lead)
    ybuf, y = guarded(dev, dy.shape, lead=lead)
    call("rac_upsample2_fwd", ptr(x_d), ptr(y), B, h, w, C, stream())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), fr.upsample2(x)), "forward"
    assert_intact(ybuf, y, "forward")
    dbuf, dy_d = guarded(dev, dy.shape, dy, lead=lead)
    gbuf, dx = guarded(dev, x.shape, lead=lead)
    call("rac_upsample2_bwd", ptr(dy_d), ptr(dx), B, h, w, C, stream())
    torch.cuda.synchronize()
    rule.check("bwd", dx, dy.double().view(B, h, 2, w, 2, C).sum((2, 4)), dy.view(B, h, 2, w, 2, C).sum((2, 4)))
    assert_intact(gbuf, dx, "backward")
    rule.done()


# =========================================================================== 6. tilecat, reparam
TILECAT_WIDTHS = [(5, 5, 0, 8, 4, 2), (4, 0, 0, 0, 10, 18), (2, 3, 4, 64, 10, 13)]  # (n0, n1, n2, c0, c1, pad)
TILECAT_CASES = [(w, 3, 48) for w in TILECAT_WIDTHS] + [(w, 40, 1024) for w in TILECAT_WIDTHS[:2]]


@pytest.mark.parametrize("widths,B,HW", TILECAT_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tilecat_equals_torch(dev, rac, widths, B, HW):
    """rac_tilecat_fwd: out[b][p] = [v0[b] | v1[b] | v2[b] | m0[b][p] | m1[b][p] | 0], equal to the torch expression, a source
    of width 0 passed as NULL; the plain kernel with the three slot modes; the per-image kernel with amax[b] = the bits of
    image b's own max |v| (image b is scaled by b + 1) between two untouched slots; both kernels write the same bits."""
    ops, call, ptr, stream = rac
    n0, n1, n2, c0, c1, pad = widths
    scale = torch.arange(1, B + 1, dtype=F32)
    vs = [rnd(90 + k, B, n) * scale.view(B, 1) if n else None for k, n in enumerate((n0, n1, n2))]
    ms = [rnd(93 + k, B, HW, c) * scale.view(B, 1, 1) if c else None for k, c in enumerate((c0, c1))]
    want = fr.tilecat(vs, ms, pad, B, HW)
    Ct = want.shape[2]
    vs_d, ms_d = [None if v is None else v.to(dev) for v in vs], [None if m is None else m.to(dev) for m in ms]

    def run(out, amax, per_image):
        call("rac_tilecat_fwd", ptr(vs_d[0]), n0, ptr(vs_d[1]), n1, ptr(vs_d[2]), n2, ptr(ms_d[0]), c0, ptr(ms_d[1]), c1, pad,
             ptr(out), B, HW, amax, per_image, stream())
        torch.cuda.synchronize()

    plain = None
    for sname, slot in slot_modes(ops, dev):
        obuf, out = guarded(dev, (B, HW, Ct))
        run(out, sptr(slot), 0)
        assert torch.equal(out.cpu(), want), sname
        assert_intact(obuf, out, sname)
        if slot is not None:
            slot.check(out, sname)
        plain = out
    slots = ops.amax_slot(dev, B + 2)
    obuf, out = guarded(dev, (B, HW, Ct))
    run(out, slots[1:].data_ptr(), 1)
    assert torch.equal(out, plain), "per-image kernel: other bits than the plain kernel"
    assert_intact(obuf, out, "per image")
    got = slots.cpu()
    assert int(got[0]) == 0 and int(got[B + 1]) == 0, "per image: neighbouring slots written"
    assert torch.equal(got[1:B + 1], want.view(B, -1).abs().max(1).values.view(torch.int32)), "per image: amax[b]"
    assert len(set(got[1:B + 1].tolist())) == B


@pytest.mark.parametrize("n", [37, 2048 * 256 + 300])
def test_reparam_vs_fp64(dev, rac, n):
    """rac_reparam_fwd z = eps exp(logvar / 2) + mu and rac_reparam_bwd dlogvar = dz eps exp(logvar / 2) / 2 under the rule;
    through ops.Reparam the gradient of mu is dz itself and that of logvar the kernel's dlogvar."""
    ops, call, ptr, stream = rac
    rule = Rule(f"f6 reparam n{n}")
    mu, lv, eps, dz = rnd(100, n), rnd(101, n) * 1.5, rnd(102, n), rnd(103, n)
    mu_d, lv_d, eps_d, dz_d = mu.to(dev), lv.to(dev), eps.to(dev), dz.to(dev)
    zbuf, z = guarded(dev, (n,))
    call("rac_reparam_fwd", ptr(mu_d), ptr(lv_d), ptr(eps_d), ptr(z), n, stream())
    gbuf, dlv = guarded(dev, (n,))
    call("rac_reparam_bwd", ptr(dz_d), ptr(lv_d), ptr(eps_d), ptr(dlv), n, stream())
    torch.cuda.synchronize()
    rule.check("fwd", z, fr.reparam(mu.double(), lv.double(), eps.double()), fr.reparam(mu, lv, eps))
    rule.check("bwd dlogvar", dlv, fr.reparam_dlogvar(dz.double(), lv.double(), eps.double()), fr.reparam_dlogvar(dz, lv, eps))
    assert_intact(zbuf, z, "z")
    assert_intact(gbuf, dlv, "dlogvar")
    mu_g, lv_g = mu_d.clone().requires_grad_(True), lv_d.clone().requires_grad_(True)
    z2 = ops.Reparam.apply(mu_g, lv_g, eps_d)
    assert torch.equal(z2.detach(), z)
    z2.backward(dz_d)
    assert torch.equal(mu_g.grad, dz_d) and torch.equal(lv_g.grad, dlv)
    rule.done()
