"""PSNR / SSIM of the evaluation path (reference src/utils/metrics.py:45-78), one fused HIP launch."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def _run(img1, img2, mask=None, want_map=False):
    if not img1.is_cuda:
        raise _lib.RacError("metrics run on the GPU only (no CPU fallback)")
    a, b = img1.to(torch.float32).contiguous(), img2.to(torch.float32).contiguous()
    N, C, H, W = a.shape
    assert C == 3 and b.shape == a.shape
    acc = torch.zeros((2, N), device=a.device, dtype=torch.float32)
    ssim_map = torch.empty_like(a) if want_map else None
    m = None if mask is None else mask.to(torch.float32).contiguous()
    _lib.call("rac_psnr_ssim", a.data_ptr(), b.data_ptr(), _lib.ptr(m), acc[0].data_ptr(), acc[1].data_ptr(),
              _lib.ptr(ssim_map), N, H, W, _lib.stream_ptr())
    return acc, ssim_map, 3 * H * W


DONTCARE_KINDS = (2, 3)  # RAC_LOSS_DONTCARE_MSE, RAC_LOSS_DONTCARE_L1


def _sum_in_order(x):
    """Sum over the last dimension, element 0 first: one add per element whatever the tensor's other dimensions are, so
    a video group's mean has the same bits whether its rows stand alone or among other groups."""
    t = x[..., 0]
    for k in range(1, x.shape[-1]):
        t = t + x[..., k]
    return t


@torch.no_grad()
def table_scalars(rows, kind, n_values, index=None):
    """The scalars `_eval_step` logs for a frame from the per-video table of `ops.eval_frames`: `rows` (..., B, 8), one
    video group per leading index; `kind` the loss kind the table was made for, `n_values` = 3 H W; `index`: the videos
    of the group to average over (a sequence or a tensor of positions in [0, B), default all) -- selecting rows
    replaces gathering frames and scoring them again (the per-robot losses).  Returns a dict of tensors of the leading
    shape: recon_loss, robot_loss, world_loss (losses.py:11-78 with their `+ 1` denominators), psnr (the mean of the
    per-video 10 log10(1 / mse), src/utils/metrics.py:61-78) and ssim (the mean of the map).  Plain elementwise torch
    on the table's device; no host sync."""
    if index is not None:
        index = torch.as_tensor(index, dtype=torch.long, device=rows.device)
        rows = rows.index_select(-2, index)
    nb = rows.shape[-2]
    main, rob2, world2, rob_n, se = (rows[..., k] for k in range(5))
    world_n = n_values - rob_n
    recon = main / (world_n + 1.0) if kind in DONTCARE_KINDS else main / n_values
    psnr_video = 10.0 * torch.log(1.0 / (se / n_values)) / np.log(10)
    ssim_video = (rows[..., 5] + rows[..., 6]) + rows[..., 7]
    return {"recon_loss": _sum_in_order(recon) / nb,
            "robot_loss": _sum_in_order(rob2 / (rob_n + 1.0)) / nb,
            "world_loss": _sum_in_order(world2 / (world_n + 1.0)) / nb,
            "psnr": _sum_in_order(psnr_video) / nb,
            "ssim": _sum_in_order(ssim_video) / (nb * n_values)}


@torch.no_grad()
def psnr(estimates, targets, data_dims=3):
    """Per-sample PSNR of two [0,1] batches; like the reference both are first mapped to (x+1)/2
    (src/utils/metrics.py:61-78).  Inputs are clamped to [0,1] as the eval loop does (trainer.py:685)."""
    acc, _, n = _run(estimates, targets)
    return 10.0 * torch.log(1.0 / (acc[0] / n)) / np.log(10)


@torch.no_grad()
def ssim(img1, img2, window_size=11):
    """SSIM map as a numpy array (N,3,H,W) (src/utils/metrics.py:45-58)."""
    assert window_size == 11
    return _run(img1, img2, want_map=True)[1].cpu().numpy()


@torch.no_grad()
def masked_psnr_ssim(pred, target, mask):
    """(per-sample PSNR tensor, mean SSIM tensor) of zero_robot_region(mask, .) versions of both frames --
    the fused form of trainer.py:681-693; no host sync."""
    acc, _, n = _run(target, pred, mask)
    return 10.0 * torch.log(1.0 / (acc[0] / n)) / np.log(10), acc[1].sum() / (acc.shape[1] * n)
