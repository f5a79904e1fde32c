"""Plain torch references of the frame, loss, metric, CEM-tail and pool / upsample / tilecat / reparam operations, written
once and dtype-generic: called on .double() inputs they are the fp64 reference of tests/test_gpu_frame.py, on fp32 inputs
the "same formula in fp32" of the rule in tests/fp64_tools.py.  Where oracle/svg_oracle.py's expression works in any
dtype it is used as it stands; tests/test_frame_refs_host.py shows that the rest are the oracle's operations in fp32.

Layouts: frames and masks are planes (N, C, H, W) as in the oracle; `to_map` / `from_map` go to and from the kernels'
(N, H, W, C) maps."""
import math
import types

import torch
import torch.nn.functional as F

from oracle import svg_oracle as orc

LOSS_NAMES = ("mse", "l1", "dontcare_mse", "dontcare_l1")

composite = orc.composite                  # (x4 planes (N, 4, H, W), prev) -> (N, 3, H, W)
zero_region = orc.zero_robot_region        # (mask (N, 1, H, W), image): image * 0 where the mask is set
kl_loss = orc.kl_loss
psnr = orc.psnr


def to_map(planes):
    return planes.permute(0, 2, 3, 1).contiguous()


def from_map(m):
    return m.permute(0, 3, 1, 2).contiguous()


def pack_input(img, zmask, mask, pad):
    """rac_pack_input as planes: [zero_region(zmask, img) | mask | `pad` zero channels]."""
    N, _, H, W = img.shape
    parts = [img if zmask is None else zero_region(zmask, img)]
    if mask is not None:
        parts.append(mask.to(img.dtype))
    parts.append(torch.zeros(N, pad, H, W, dtype=img.dtype))
    return torch.cat(parts, 1)


def unpack_grad(dpacked, zmask):
    """Gradient of pack_input with respect to img: the first 3 channels of the packed gradient, 0 where zmask is set."""
    d = dpacked[:, :3]
    return d if zmask is None else torch.where(zmask.bool().expand(-1, 3, -1, -1), torch.zeros_like(d), d)


def recon_loss(kind, pred, target, mask=None, robot_weight=0.0, batch_weight=None):
    """PredictionTrainer._recon_loss of the oracle for the loss named `kind`."""
    cfg = types.SimpleNamespace(reconstruction_loss=kind, robot_pixel_weight=robot_weight)
    return orc.recon_loss(cfg, pred, target, mask, batch_weight)


def robot_mse(pred, target, mask):
    """orc.robot_mse with the zero in the inputs' dtype."""
    m3 = mask.bool().expand(-1, 3, -1, -1)
    d = target - pred
    d = torch.where(m3, d, torch.zeros_like(d))
    return torch.mean((d ** 2).sum((1, 2, 3)) / (m3.sum((1, 2, 3)) + 1))


def world_mse(pred, target, mask):
    """orc.world_mse with the zero in the inputs' dtype."""
    m3 = mask.bool().expand(-1, 3, -1, -1)
    d = target - pred
    d = torch.where(m3, torch.zeros_like(d), d)
    return torch.mean((d ** 2).sum((1, 2, 3)) / ((~m3).sum((1, 2, 3)) + 1))


def recon_out(kind, pred, target, mask=None, robot_weight=0.0, batch_weight=None):
    """The (3,) result of rac_recon_loss_fwd: [loss, robot_mse, world_mse]; the two metrics are 0 without a mask."""
    loss = recon_loss(kind, pred, target, mask, robot_weight, batch_weight)
    zero = torch.zeros((), dtype=pred.dtype)
    return torch.stack([loss, robot_mse(pred, target, mask) if mask is not None else zero,
                        world_mse(pred, target, mask) if mask is not None else zero])


def ssim_window(dtype):
    """(3, 1, 11, 11) depthwise window: g32 = the fp32 gaussian(11, 1.5) over its fp32 sum, outer(g32, g32) in fp32, cast."""
    g = torch.tensor([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return (g @ g.t()).float().to(dtype).expand(3, 1, 11, 11).contiguous()


def ssim_map(img1, img2):
    """orc.ssim_map in the inputs' dtype."""
    w = ssim_window(img1.dtype)
    blur = lambda t: F.conv2d(t, w, padding=5, groups=3)  # noqa: E731
    m1, m2 = blur(img1), blur(img2)
    v1, v2, v12 = blur(img1 * img1) - m1 * m1, blur(img2 * img2) - m2 * m2, blur(img1 * img2) - m1 * m2
    return ((2 * m1 * m2 + 1e-4) * (2 * v12 + 9e-4)) / ((m1 * m1 + m2 * m2 + 1e-4) * (v1 + v2 + 9e-4))


def sq_err(a, b):
    """Per-sample sum over (C, H, W) of the squared difference of (x + 1) / 2: orc.psnr's mse times 3 H W."""
    return (((a + 1) / 2) - ((b + 1) / 2)).pow(2).sum((1, 2, 3))


def psnr_ssim(a, b, mask=None):
    """(ssim_map, sq_err [N], ssim_sum [N]) of rac_psnr_ssim: both frames through zero_region(mask, .) first."""
    if mask is not None:
        a, b = zero_region(mask, a), zero_region(mask, b)
    smap = ssim_map(a, b)
    return smap, sq_err(a, b), smap.sum((1, 2, 3))


def masked_psnr_ssim(pred, target, mask):
    """(per-sample PSNR, mean SSIM) of the zeroed frames, as metrics.masked_psnr_ssim returns them."""
    a, b = zero_region(mask, target), zero_region(mask, pred)
    return psnr(a, b), ssim_map(a, b).mean()


def cem_next(x4, curr, next_mask=None):
    """The frame a CEM step feeds back: composite, then the robot region zeroed."""
    nxt = composite(x4, curr)
    return nxt if next_mask is None else zero_region(next_mask, nxt)


def img_l2_cost(curr, goal):
    """orc.img_l2_cost as a tensor."""
    return -(((255 * (curr - goal)) ** 2).sum((1, 2, 3)).sqrt())


def img_dontcare_cost(curr, goal, curr_mask, goal_mask):
    """orc.img_dontcare_cost as a tensor with the zero in the inputs' dtype; either mask may be None."""
    N, _, H, W = curr.shape
    tot = torch.zeros(N, 1, H, W, dtype=torch.bool)
    if curr_mask is not None:
        tot = tot | curr_mask.bool()
    if goal_mask is not None:
        tot = tot | goal_mask.bool()
    d = (255 * (curr - goal)) ** 2
    d = torch.where(tot.expand(-1, 3, -1, -1), torch.zeros_like(d), d)
    return -(d.sum((1, 2, 3)).sqrt() / (~tot).sum((1, 2, 3)))


def maxpool2(x_map):
    return to_map(F.max_pool2d(from_map(x_map), 2, 2))


def upsample2(x_map):
    return to_map(F.interpolate(from_map(x_map), scale_factor=2, mode="nearest"))


def tilecat(vs, ms, pad, B, HW):
    """[B][HW][sum of widths + pad]: the vectors vs[k] [B][n_k] tiled over the pixels, the maps ms[k] [B][HW][c_k], zeros."""
    parts = [v.view(B, 1, -1).expand(B, HW, -1) for v in vs if v is not None]
    parts += [m for m in ms if m is not None]
    parts.append(torch.zeros(B, HW, pad, dtype=parts[0].dtype))
    return torch.cat(parts, 2).contiguous()


def reparam(mu, logvar, eps):
    return eps * torch.exp(0.5 * logvar) + mu


def reparam_dlogvar(dz, logvar, eps):
    return dz * eps * (0.5 * torch.exp(0.5 * logvar))
