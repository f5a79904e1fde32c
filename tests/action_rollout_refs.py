"""numpy / fp64 restatements of what `rac_action_rollout_sheet` (include/rac_hip.h) computes, for
tests/test_action_rollout_host.py and tests/test_gpu_action_rollout.py.

`sheet_ref`: the reference's `save_gif(name, gifs)` with `gifs[t][i] = [truth[t][i], gen[0][t][i], ...]`
(src/prediction/test_action_rollout.py:152-174, src/utils/plot.py:32-81,109-115), derived from its text (the module
imports packages this project does not depend on, so no fixture was recorded from it): the inner `image_tensor(row)` is
a canvas of ones (c, h, w n + (n - 1)) with image k copied to columns [k (w + 1), k (w + 1) + w); the outer call, with
padding 0, stacks those rows along the height; then channels last, clamp to [0, 1], `np.uint8(img * 255)`.

`response_ref` / `response_bound`: the header's formula in fp64 and the error bound of its documented reduction order."""
import math

import numpy as np


def u8_ref(v):
    """np.uint8(clamp(v, 0, 1) * 255) in fp32; a NaN, which numpy's cast leaves undefined, gives 0."""
    v = np.asarray(v, dtype=np.float32)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1))).astype(np.float32)
    return (v * np.float32(255)).astype(np.uint8)


def row_ref(images):
    """image_tensor(images) for a flat list of (3, h, w) images: side by side on a canvas of ones, one column between."""
    c, h, w = images[0].shape
    canvas = np.ones((c, h, w * len(images) + (len(images) - 1)), np.float32)
    for k, img in enumerate(images):
        canvas[:, :, k * (w + 1):k * (w + 1) + w] = img
    return canvas


def sheet_ref(truth, gen):
    """uint8 (S, L, b h, (1 + G) w + G, 3) from `truth` (T >= L, B >= b, 3, h, w) and `gen` (S, G, L, b, 3, h, w)."""
    S, G, L, b = gen.shape[:4]
    sheets = []
    for s in range(S):
        for t in range(L):
            rows = [row_ref([truth[t, i]] + [gen[s, g, t, i] for g in range(G)]) for i in range(b)]
            sheets.append(u8_ref(np.concatenate(rows, axis=1).transpose(1, 2, 0)))  # padding 0: stacked along the height
    return np.stack(sheets).reshape((S, L) + sheets[0].shape)


def response_ref(gen, base):
    """fp64 (S, G, L, b): the mean |gen[s] - gen[base]| of every frame; sweep `base` itself is 0 by definition."""
    g = np.asarray(gen, dtype=np.float64)
    with np.errstate(invalid="ignore"):  # (an infinity minus itself, in sweep `base`, which is overwritten)
        out = np.abs(g - g[base:base + 1]).mean(axis=(4, 5, 6))
    out[base] = 0.0
    return out


def response_bound(H, W):
    """Relative error bound of one response entry against `response_ref`, from the header's reduction order.

    Every addend |d| is one fp32 subtraction of two fp32 inputs (relative error <= u = 2^-24; |.| is exact) and the
    addends are non-negative, so a value that passes through k roundings on its way into the result carries a factor in
    [(1 - u)^k, (1 + u)^k] and so does the whole sum.  The longest path: 1 subtraction, 12 ceil(H W / 1024) adds of the
    thread's running sum, 6 butterfly adds, 3 serial adds of the wave sums, 1 conversion of 3 H W to fp32 and 1 division:
    k = 12 ceil(H W / 1024) + 12, bound gamma_k = k u / (1 - k u)."""
    k = 12 * math.ceil(H * W / 1024) + 12
    u = 2.0 ** -24
    return k * u / (1 - k * u)
