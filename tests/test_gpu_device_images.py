"""GPU: `rac_image_pipeline` (csrc/rac_augment.hip), the image half of the data path in one launch, against the host
`ImagePipeline` arithmetic: masks bit for bit, images against an fp64 replay of the pipeline written here, within 4x the
error the fp32 host pipeline itself has against that replay (fused multiply-adds and another summation order of the
contrast mean each add at most one rounding of the kind already inside that error; a wrong tap, factor or order of
operations shows at 1e-3 or more).

Shapes (raw -> model): 20x28 -> 12x16, 64x85 -> 48x64, 48x64 -> 48x64, 64x64 -> 64x64.  At these every interpolation
coordinate is at least 1/128 away from an integer unless it is clamped or exact, so fp32 and fp64 pick the same taps and
the fp32 masks equal the fp64 replay's; likewise at 32x43 -> 48x64 and 40x100 -> 48x64, where the stored frame is smaller
than the model's on one or both axes.  The replay has its own jitter arithmetic (`jitter64`), written from the
definitions and not shared with data.py.  Measured on an MI355X: see DESIGN.md 7."""
import argparse
import itertools
import os
import random
import sys

import numpy as np
import pytest
import torch

from robot_aware_control_amd import RacError
from robot_aware_control_amd import data as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((20, 28), (12, 16)), ((64, 85), (48, 64)), ((48, 64), (48, 64)), ((64, 64), (64, 64))]
# stored frames SMALLER than the model size on both axes / on one axis only (rows up, columns down); the coordinates are
# odd multiples of 1/96, 1/128, 1/12 and 1/32 minus a half: never an integer, at least 1/128 away from one
UPSAMPLING = [((32, 43), (48, 64)), ((40, 100), (48, 64))]
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def clip(seed, T, Hs, Ws):
    """uint8 frames with distinct content per frame: 0 noise, 1 low contrast, 2 exactly gray (r == g == b), 3.. smooth
    colour ramps plus noise; a moving rectangular robot mask."""
    g = np.random.Generator(np.random.Philox(key=[5, seed]))
    frames = g.integers(0, 256, (T, Hs, Ws, 3), dtype=np.uint8)
    if T > 1:
        frames[1] = g.integers(118, 126, (Hs, Ws, 3), dtype=np.uint8)
    if T > 2:
        frames[2] = g.integers(0, 256, (Hs, Ws, 1), dtype=np.uint8)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    for t in range(3, T):
        ramp = np.stack([255 * yy / Hs, 255 * xx / Ws, 255 * (yy + xx) / (Hs + Ws)], -1)
        frames[t] = np.clip(ramp + g.integers(-20, 20, (Hs, Ws, 3)) + 7 * t, 0, 255).astype(np.uint8)
    mask = np.zeros((T, Hs, Ws), np.uint8)
    for t in range(T):
        cy, cx = int(g.integers(2, Hs - 2)), int(g.integers(2, Ws - 2))
        mask[t, max(0, cy - Hs // 6):cy + Hs // 6, max(0, cx - Ws // 7):cx + Ws // 7] = 1
    return frames, mask


def params(seed, h, w, shrink, order=None, jitter=True):
    g = random.Random(1000 + seed)
    top, left = g.randint(0, shrink), g.randint(0, shrink)
    factors = (g.uniform(0.8, 1.2), g.uniform(0.8, 1.2), g.uniform(0.8, 1.2), g.uniform(-0.1, 0.1))
    if order is None:
        order = [0, 1, 2, 3]
        g.shuffle(order)
    return D.ImageParams(h, w, top, left, h - shrink, w - shrink, jitter, tuple(order), factors)


def resize64(x, h, w):
    """torch's bilinear rule (align_corners=False) as an explicit gather in float64."""
    H, W = x.shape[-2:]
    if (H, W) == (h, w):
        return x

    def axis(n_in, n_out):
        o = torch.arange(n_out, dtype=torch.float64)
        src = ((n_in / n_out) * (o + 0.5) - 0.5).clamp(min=0)
        i0 = src.floor().long().clamp(max=n_in - 1)
        i1 = i0 + (i0 < n_in - 1).long()
        l1 = src - i0
        return i0, i1, 1 - l1, l1

    y0, y1, ly0, ly1 = axis(H, h)
    x0, x1, lx0, lx1 = axis(W, w)

    def rows(r):
        return lx0 * r[..., x0] + lx1 * r[..., x1]
    return ly0[:, None] * rows(x[..., y0, :]) + ly1[:, None] * rows(x[..., y1, :])


def replay64(frames, mask, p):
    """The whole pipeline in float64: u8 / 255, resize, crop + resize back, the jitter closures on a float64 clip."""
    video = resize64(torch.from_numpy(frames).permute(0, 3, 1, 2).double() / 255, p.h, p.w)
    m = resize64(torch.from_numpy(mask)[:, None].double(), p.h, p.w)
    if (p.th, p.tw) != (p.h, p.w):
        video = resize64(video[:, :, p.top:p.top + p.th, p.left:p.left + p.tw], p.h, p.w)
        m = resize64(m[:, :, p.top:p.top + p.th, p.left:p.left + p.tw], p.h, p.w)
    if p.jitter:
        video = jitter64(video, p.factors, p.order)
    return video, (m != 0).double()


def jitter64(x, factors, order):
    """The colour jitter on a float64 (T,3,H,W) clip, from the definitions (torchvision's tensor adjust_* functions as the
    reference applies them, robonet_dataset.py:545-572): operation order[k] runs k-th, 0 brightness, 1 contrast, 2
    saturation, 3 hue."""
    bf, cf, sf, hf = factors

    def gray(v):
        return 0.2989 * v[:, 0] + 0.587 * v[:, 1] + 0.114 * v[:, 2]

    for op in order:
        if op == 0:
            x = (x * bf).clamp(0, 1)
        elif op == 1:
            mean = gray(x).mean((1, 2))[:, None, None, None]
            x = (cf * x + (1 - cf) * mean).clamp(0, 1)
        elif op == 2:
            x = (sf * x + (1 - sf) * gray(x)[:, None]).clamp(0, 1)
        else:
            r, g, b = x[:, 0], x[:, 1], x[:, 2]
            mx, mn = torch.maximum(torch.maximum(r, g), b), torch.minimum(torch.minimum(r, g), b)
            flat = mx == mn
            span = mx - mn
            sat = span / torch.where(flat, torch.ones_like(mx), mx)
            d = torch.where(flat, torch.ones_like(mx), span)
            rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
            hue = torch.where(mx == r, bc - gc, torch.where(mx == g, 2.0 + rc - bc, 4.0 + gc - rc))
            hue = torch.remainder(torch.fmod(hue / 6.0 + 1.0, 1.0) + hf, 1.0)
            sext = torch.floor(hue * 6.0)
            f = hue * 6.0 - sext
            sext = sext.long() % 6
            p = (mx * (1.0 - sat)).clamp(0, 1)
            q = (mx * (1.0 - sat * f)).clamp(0, 1)
            t = (mx * (1.0 - sat * (1.0 - f))).clamp(0, 1)
            table = {0: (mx, t, p), 1: (q, mx, p), 2: (p, mx, t), 3: (p, q, mx), 4: (t, p, mx), 5: (mx, p, q)}
            out = torch.zeros_like(x)
            for k, rgb in table.items():
                for c in range(3):
                    out[:, c] = torch.where(sext == k, rgb[c], out[:, c])
            x = out
    return x


def items_of(videos, plist):
    return [{"frames": torch.from_numpy(f), "raw_masks": torch.from_numpy(m), "image_params": p}
            for (f, m), p in zip(videos, plist)]


def launch(videos, plist, dev):
    batch = D.collate(items_of(videos, plist))
    images, masks, _ = D.device_images(batch, dev)
    torch.cuda.synchronize()
    return images, masks


class Case:
    """One launch and its references (computed once, never modified): GPU, fp32 host pipeline, fp64 replay, per video."""

    def __init__(self, videos, plist, dev):
        self.plist = plist
        images, masks = launch(videos, plist, dev)
        self.contiguous = images.is_contiguous() and masks.is_contiguous()
        self.shape = (tuple(images.shape), tuple(masks.shape))
        self.gpu, self.gpu_masks = images.cpu().transpose(0, 1), masks.cpu().transpose(0, 1)  # (B, T, ...)
        host = [D.apply_image_params(f, m, p) for (f, m), p in zip(videos, plist)]
        ref = [replay64(f, m, p) for (f, m), p in zip(videos, plist)]
        self.host, self.host_masks = torch.stack([a for a, _ in host]), torch.stack([b for _, b in host])
        self.ref, self.ref_masks = torch.stack([a for a, _ in ref]), torch.stack([b for _, b in ref])

    def errors(self, b=None):
        """(e_ref, e_gpu): max |fp32 host - fp64 replay| and max |GPU - fp64 replay|, of video b or of the launch."""
        s = slice(None) if b is None else b
        return (float((self.host[s].double() - self.ref[s]).abs().max()),
                float((self.gpu[s].double() - self.ref[s]).abs().max()))

    def check_images(self, what, b=None):
        e_ref, e_gpu = self.errors(b)
        print(f"{what}: e_ref {e_ref:.3e}  gpu {e_gpu:.3e}  bound {4 * max(e_ref, ULP):.3e}")
        assert e_gpu <= 4 * max(e_ref, ULP), (what, e_ref, e_gpu)


_CASES = {}


def shape_case(shape, dev):
    """Six videos of 4 frames, shrink 0..5, their own corners, factors and orders."""
    if shape not in _CASES:
        (Hs, Ws), (h, w) = shape
        first = 10 * (SHAPES + UPSAMPLING).index(shape)
        videos = [clip(first + s, 4, Hs, Ws) for s in range(6)]
        plist = [params(first + s, h, w, s) for s in range(6)]
        _CASES[shape] = Case(videos, plist, dev)
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES + UPSAMPLING, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_masks_equal_the_host_pipeline(shape, dev):
    case = shape_case(shape, dev)
    assert [p.h - p.th for p in case.plist] == [0, 1, 2, 3, 4, 5]
    assert torch.equal(case.gpu_masks, case.host_masks)
    assert torch.equal(case.host_masks.double(), case.ref_masks)  # (what makes the comparison above meaningful)
    assert 0 < float(case.gpu_masks.mean()) < 1


@pytest.mark.parametrize("shape", SHAPES + UPSAMPLING, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_images_within_the_host_pipelines_own_error(shape, dev):
    case = shape_case(shape, dev)
    (h, w) = shape[1]
    assert case.shape == ((4, 6, 3, h, w), (4, 6, 1, h, w)) and case.contiguous
    assert case.gpu.dtype == torch.float32 and float(case.gpu.min()) >= 0 and float(case.gpu.max()) <= 1
    case.check_images(f"{shape}")


def test_all_24_operation_orders_in_one_launch(dev):
    orders = list(itertools.permutations(range(4)))
    videos = [clip(200 + i, 2, 20, 28) for i in range(24)]
    plist = [params(200 + i, 12, 16, i % 6, order=orders[i]) for i in range(24)]
    case = Case(videos, plist, dev)
    assert torch.equal(case.gpu_masks, case.host_masks)
    for b in range(24):  # per video: parameters are taken per video
        case.check_images(f"order {orders[b]}", b)
    # the orders matter at these inputs: another video's order on the same pixels is off by far more than the bound
    swapped = replay64(*videos[0], plist[0]._replace(order=orders[23]))[0]
    assert float((swapped - case.ref[0]).abs().max()) > 1e-3


@pytest.mark.parametrize("size", [(48, 64), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity(size, dev):
    h, w = size
    videos = [clip(300 + b, 3, h, w) for b in range(2)]
    plist = [D.draw_image_params(h, w, False)] * 2
    images, masks = launch(videos, plist, dev)
    for b, (f, m) in enumerate(videos):
        assert torch.equal(images[:, b].cpu(), torch.from_numpy(f).permute(0, 3, 1, 2).float().div(255))
        assert torch.equal(masks[:, b, 0].cpu(), torch.from_numpy(m).float())


def test_time_first_layout_and_mixed_raw_sizes(dev):
    videos = [clip(400, 3, 64, 85), clip(401, 3, 48, 64), clip(402, 3, 64, 85)]
    plist = [params(400, 48, 64, 2), params(401, 48, 64, 0), D.draw_image_params(48, 64, False)]
    case = Case(videos, plist, dev)
    assert case.shape == ((3, 3, 3, 48, 64), (3, 3, 1, 48, 64)) and case.contiguous
    assert torch.equal(case.gpu_masks, case.host_masks)
    for b in range(3):
        case.check_images(f"video {b}", b)
        for t in range(3):  # frame (t, b) is video b's frame t and nobody else's
            near = float((case.gpu[b, t] - case.host[b, t]).abs().max())
            for b2, t2 in ((b, (t + 1) % 3), ((b + 1) % 3, t)):
                assert float((case.gpu[b, t] - case.host[b2, t2]).abs().max()) > 1000 * max(near, ULP)


def test_two_launches_give_the_same_bits(dev):
    videos = [clip(500 + b, 4, 64, 85) for b in range(4)]
    plist = [params(500 + b, 48, 64, b + 1) for b in range(4)]
    a, am = launch(videos, plist, dev)
    b, bm = launch(videos, plist, dev)
    assert all(p.jitter for p in plist) and torch.equal(a, b) and torch.equal(am, bm)


def cfg(root, **kw):
    d = dict(data_root=root, load_movement_info=False, video_length=8, n_past=1, n_future=2, action_dim=4, robot_dim=5,
             robot_joint_dim=7, impute_autograsp_action=False, image_width=64, image_height=48, seed=3,
             preload_ram=False, preprocess_action="raw", experiment="train_robonet", model_use_heatmap=False,
             train_val_split=0.75, img_augmentation=True, data_threads=0, batch_size=3, test_batch_size=2)
    d.update(kw)
    return argparse.Namespace(**d)


def seed_all(seed):
    random.seed(seed)
    torch.manual_seed(seed)


def test_end_to_end_through_the_loaders(tmp_path, dev):
    """Train and test loaders over a synthetic tree, img_augmentation on, with and without device_images under the same
    seeds: through the device prefetcher and through process_batch on the GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_robonet as mk
    assert mk.write(str(tmp_path), per_view=2, length=10, seed=4) == 8

    def batches(on, prefetch, n=3):
        seed_all(31)
        train, test = D.create_loaders(cfg(str(tmp_path), device_images=on))
        if prefetch:
            pf = D.DevicePrefetcher(train, dev)
            out = [next(pf) for _ in range(n)]
            pf.close()
            pf.thread.join(30)
            assert not pf.thread.is_alive()
        else:
            gen = D.get_batch(train, dev, prefetch=False)
            out = [next(gen) for _ in range(n)]
        out.append(D.process_batch(next(iter(test)), dev))  # the test loader: no augmentation, jitter flag off
        torch.cuda.synchronize()
        return out

    seed_all(31)
    raw_train, raw_test = D.create_loaders(cfg(str(tmp_path), device_images=True))
    raw = list(itertools.islice((b for _ in range(2) for b in raw_train), 3))  # collated, not yet processed
    raw.append(next(iter(raw_test)))
    assert raw[0]["image_jobs"].numpy().reshape(-1).view(D.IMAGE_JOB)["jitter"].all()
    assert not raw[3]["image_jobs"].numpy().reshape(-1).view(D.IMAGE_JOB)["jitter"].any()
    host = batches(False, True)
    for prefetch in (True, False):
        got = batches(True, prefetch)
        for k, (a, b, r) in enumerate(zip(host, got, raw)):
            assert set(a) == set(b)
            for key in a:
                if isinstance(a[key], torch.Tensor):
                    assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].device == b[key].device
                    if key != "images":
                        assert torch.equal(a[key], b[key]), key
                else:
                    assert a[key] == b[key], key
            # images: the bound of the kernel tests, against the fp64 replay of this batch's raw bytes and jobs
            jobs, T, h, w = D._image_jobs(r)
            frames, masks = r["frames"].numpy(), r["raw_masks"].numpy()
            ref = [replay64(*D.job_video(j, frames, masks, T), D.job_params(j, h, w))[0] for j in jobs]
            ref = torch.stack(ref).transpose(0, 1)
            e_ref = float((a["images"].cpu().double() - ref).abs().max())
            e_gpu = float((b["images"].cpu().double() - ref).abs().max())
            print(f"batch {k} prefetch {prefetch}: e_ref {e_ref:.3e} gpu {e_gpu:.3e}")
            assert e_gpu <= 4 * max(e_ref, ULP), (k, e_ref, e_gpu)
    # and through get_batch's default route (the prefetcher it builds itself)
    seed_all(31)
    train, _ = D.create_loaders(cfg(str(tmp_path), device_images=True))
    first = next(D.get_batch(train, dev))
    assert set(first) == set(host[0]) and first["images"].shape == host[0]["images"].shape
    assert torch.equal(first["masks"], host[0]["masks"]) and torch.equal(first["states"], host[0]["states"])


def test_unsupported_width_is_an_error(dev):
    videos = [clip(600, 2, 20, 28)]
    with pytest.raises(RacError, match="multiple of 4"):
        launch(videos, [D.draw_image_params(12, 18, False)], dev)
    torch.cuda.synchronize()
    images, _ = launch(videos, [D.draw_image_params(12, 16, False)], dev)  # the device is fine afterwards
    assert torch.isfinite(images).all()
