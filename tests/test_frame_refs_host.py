"""tests/frame_refs.py, the reference of tests/test_gpu_frame.py, is the oracle's operations (oracle/svg_oracle.py, the
reference project's expressions): in fp32 it gives the oracle's values -- the same bits where the expressions are the
same, rtol 1e-6 where only the order of a sum differs -- and it reproduces the values stored in tests/golden/losses.npz
at the tolerances test_gpu_ops.py holds the kernels to.  Runs on the CPU."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import svg_oracle as orc
from tests import frame_refs as fr
from tests.fp64_tools import rnd

N, H, W = 3, 21, 35


def frames(seed):
    pred, target = torch.sigmoid(rnd(seed, N, 3, H, W)), torch.sigmoid(rnd(seed + 1, N, 3, H, W))
    mask = (rnd(seed + 2, N, 1, H, W) > 0.3).float()
    mask[0], mask[1] = 0.0, 1.0  # an all-world and an all-robot sample
    return pred, target, mask


def test_composite_and_zero_region_are_the_oracles():
    x4, prev = torch.sigmoid(rnd(1, N, 4, H, W)), torch.sigmoid(rnd(2, N, 3, H, W))
    mask = (rnd(3, N, 1, H, W) > 0).float()
    assert torch.equal(fr.composite(x4, prev), orc.composite(x4, prev))
    assert torch.equal(fr.zero_region(mask, prev), orc.zero_robot_region(mask, prev))
    assert torch.equal(fr.cem_next(x4, prev, mask), orc.zero_robot_region(mask, orc.composite(x4, prev)))
    assert torch.equal(fr.cem_next(x4, prev), orc.composite(x4, prev))
    packed = fr.pack_input(prev, mask, torch.cat([mask, 1 - mask], 1), 3)
    assert torch.equal(packed[:, :5], torch.cat([orc.zero_robot_region(mask, prev), mask, 1 - mask], 1))
    assert packed.shape[1] == 8 and float(packed[:, 5:].abs().max()) == 0.0
    # in fp64 the same expressions run in fp64
    assert fr.composite(x4.double(), prev.double()).dtype == torch.float64
    assert fr.zero_region(mask.double(), prev.double()).dtype == torch.float64


@pytest.mark.parametrize("with_bw", [False, True])
@pytest.mark.parametrize("kind", fr.LOSS_NAMES)
def test_recon_loss_is_the_oracles(kind, with_bw):
    pred, target, mask = frames(10)
    bw = rnd(13, N).abs() + 0.5 if with_bw else None
    cfg = types.SimpleNamespace(reconstruction_loss=kind, robot_pixel_weight=0.5)
    want = orc.recon_loss(cfg, pred, target, mask, bw)
    got = fr.recon_out(kind, pred, target, mask, 0.5, bw)
    assert torch.equal(got[0], want)
    assert torch.equal(got[1], orc.robot_mse(pred, target, mask))
    assert torch.equal(got[2], orc.world_mse(pred, target, mask))
    got64 = fr.recon_out(kind, pred.double(), target.double(), mask.double(), 0.5, None if bw is None else bw.double())
    assert got64.dtype == torch.float64
    torch.testing.assert_close(got64.float(), got, rtol=1e-5, atol=0)
    if kind in ("mse", "l1"):
        plain = fr.recon_out(kind, pred, target, None, 0.0, bw)
        assert torch.equal(plain[0], want) and float(plain[1]) == 0.0 and float(plain[2]) == 0.0


def test_kl_psnr_ssim_are_the_oracles():
    mu1, lv1, mu2, lv2 = rnd(20, 4, 10, 8, 8), rnd(21, 4, 10, 8, 8) * 1.5, rnd(22, 4, 10, 8, 8), rnd(23, 4, 10, 8, 8) * 1.5
    assert torch.equal(fr.kl_loss(mu1, lv1, mu2, lv2, 4), orc.kl_loss(mu1, lv1, mu2, lv2, 4))
    a, b, mask = frames(30)
    assert torch.equal(fr.psnr(a, b), orc.psnr(a, b))
    assert torch.equal(fr.ssim_map(a, b), orc.ssim_map(a, b))
    # the per-sample sum rac_psnr_ssim keeps is orc.psnr's mean times the element count (another order of the sum)
    mse = fr.sq_err(a, b) / (3 * H * W)
    torch.testing.assert_close(10 * torch.log(1.0 / mse) / np.log(10), orc.psnr(a, b), rtol=1e-6, atol=0)
    smap, se, ss = fr.psnr_ssim(a, b, mask)
    za, zb = orc.zero_robot_region(mask, a), orc.zero_robot_region(mask, b)
    assert torch.equal(smap, orc.ssim_map(za, zb)) and torch.equal(se, fr.sq_err(za, zb))
    assert torch.equal(ss, smap.sum((1, 2, 3)))
    assert bool((smap[1] == 1.0).all()) and float(se[1]) == 0.0  # the fully masked sample
    p, s = fr.masked_psnr_ssim(b, a, mask)
    assert torch.equal(p, orc.psnr(za, zb)) and torch.equal(s, orc.ssim_map(za, zb).mean())
    w64 = fr.ssim_window(torch.float64)
    assert w64.dtype == torch.float64 and torch.equal(w64.float(), fr.ssim_window(torch.float32))


def test_cem_costs_are_the_oracles():
    curr, goal = torch.sigmoid(rnd(40, 5, 3, H, W)), torch.sigmoid(rnd(41, 1, 3, H, W))
    cm, gm = rnd(42, 5, 1, H, W) > 0.5, rnd(43, 1, 1, H, W) > 0.5
    assert np.array_equal(fr.img_l2_cost(curr, goal).numpy(), orc.img_l2_cost(curr, goal))
    assert np.array_equal(fr.img_dontcare_cost(curr, goal, cm, gm).numpy(), orc.img_dontcare_cost(curr, goal, cm, gm))
    none = torch.zeros_like(gm)
    assert np.array_equal(fr.img_dontcare_cost(curr, goal, cm, None).numpy(), orc.img_dontcare_cost(curr, goal, cm, none))
    assert np.array_equal(fr.img_dontcare_cost(curr, goal, None, gm).numpy(),
                          orc.img_dontcare_cost(curr, goal, torch.zeros_like(cm), gm))


def test_frame_refs_reproduce_the_stored_losses(golden_dir):
    """The values and gradients of losses.npz (written by the reference project's own loss and cost classes), at the
    tolerances of test_frame_ops_and_losses and test_cem_step_tail."""
    g = np.load(os.path.join(golden_dir, "losses.npz"))
    target, mask, bw = (torch.from_numpy(g[k]) for k in ("target", "mask", "bw"))
    for name, kind, rw, use_bw in (("l1", "l1", 0, False), ("l1_bw", "l1", 0, True), ("mse", "mse", 0, False),
                                   ("dc_l1_w0", "dontcare_l1", 0.0, False), ("dc_l1_w05", "dontcare_l1", 0.5, False),
                                   ("dc_l1_w0_bw", "dontcare_l1", 0.0, True), ("dc_mse_w05", "dontcare_mse", 0.5, False)):
        pred = torch.from_numpy(g["pred"]).requires_grad_(True)
        out = fr.recon_out(kind, pred, target, mask, rw, bw if use_bw else None)
        np.testing.assert_allclose(out[0].item(), g[name], rtol=2e-6)
        np.testing.assert_allclose(out[1].item(), g["robot_mse"], rtol=2e-6)
        np.testing.assert_allclose(out[2].item(), g["world_mse"], rtol=2e-6)
        out[0].backward()
        np.testing.assert_allclose(pred.grad.numpy(), g[name + "_grad"], rtol=1e-5, atol=1e-9)
    ts = [torch.from_numpy(g[k]).requires_grad_(True) for k in ("mu1", "lv1", "mu2", "lv2")]
    kl = fr.kl_loss(*ts, 3)
    np.testing.assert_allclose(kl.item(), g["kl"], rtol=3e-6)
    kl.backward()
    for t, k in zip(ts, ("kl_gmu1", "kl_glv1", "kl_gmu2", "kl_glv2")):
        np.testing.assert_allclose(t.grad.numpy(), g[k], rtol=2e-5, atol=1e-7)
    curr, goal = torch.from_numpy(g["c_curr"]), torch.from_numpy(g["c_goal"])
    cm, gm = torch.from_numpy(g["c_cmask"]), torch.from_numpy(g["c_gmask"])
    np.testing.assert_allclose(fr.img_l2_cost(curr, goal).numpy(), g["cost_l2"], rtol=2e-6)
    np.testing.assert_allclose(fr.img_dontcare_cost(curr, goal, cm, gm.view(1, 1, *gm.shape[-2:])).numpy(),
                               g["cost_dontcare"], rtol=2e-6)


def test_pool_upsample_tilecat_reparam_layouts():
    """The map-layout helpers: maxpool2 / upsample2 are torch's on planes; tilecat is the oracle's tiling followed by cat."""
    x = rnd(50, 2, 4, 6, 5)
    assert torch.equal(fr.from_map(fr.maxpool2(x)), torch.nn.functional.max_pool2d(fr.from_map(x), 2, 2))
    assert fr.upsample2(x).shape == (2, 8, 12, 5) and torch.equal(fr.upsample2(x)[:, 1::2, ::2], x)
    a, r, hm = rnd(51, 3, 5), rnd(52, 3, 4), rnd(53, 3, 8, 8, 8)
    want = torch.cat([orc._tile(a, 8, 8), orc._tile(r, 8, 8), fr.from_map(hm)], 1)
    got = fr.tilecat([a, r, None], [hm.view(3, 64, 8), None], 3, 3, 64)
    assert torch.equal(fr.from_map(got.view(3, 8, 8, 20))[:, :17], want) and float(got[..., 17:].abs().max()) == 0.0
    mu, lv, eps = rnd(54, 37).requires_grad_(True), rnd(55, 37).requires_grad_(True), rnd(56, 37)
    dz = rnd(57, 37)
    fr.reparam(mu, lv, eps).backward(dz)
    assert torch.equal(mu.grad, dz)
    torch.testing.assert_close(lv.grad, fr.reparam_dlogvar(dz, lv.detach(), eps), rtol=1e-6, atol=1e-12)
