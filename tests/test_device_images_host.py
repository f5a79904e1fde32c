"""CPU: the host side of `--device_images` (robot_aware_control_amd/data.py): the augmentation parameters drawn apart from
their application replay `ImagePipeline` bit for bit, a device-mode item carries the raw bytes and the parameters, a CPU
device gets today's batches, videos of different raw sizes collate into one flat buffer, and the ctypes mirror of
`struct rac_image_job` has the library's size."""
import argparse
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

from robot_aware_control_amd import _lib
from robot_aware_control_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def legacy_pipeline(frames, masks, h, w, augment):
    """`ImagePipeline.__call__` as it was before it was split into draw + apply (draws and arithmetic interleaved, the
    jitter as shuffled closures): what the split must reproduce, images, masks and both generators' states."""
    video = D._resize(D._to_tensor(frames), h, w)
    mask = D._resize(D._to_tensor(masks), h, w)
    if augment:
        shrink = random.randint(0, 5)
        th, tw = h - shrink, w - shrink
        top = left = 0
        if shrink:
            top = int(torch.randint(0, h - th + 1, size=(1,)).item())
            left = int(torch.randint(0, w - tw + 1, size=(1,)).item())
        ops = []
        bf = random.uniform(0.8, 1.2)
        ops.append(lambda im: (im * bf).clamp(0, 1))
        cf = random.uniform(0.8, 1.2)
        ops.append(lambda im: (cf * im + (1 - cf) * D._gray(im).mean((1, 2, 3), keepdim=True)).clamp(0, 1))
        sf = random.uniform(0.8, 1.2)
        ops.append(lambda im: (sf * im + (1 - sf) * D._gray(im)).clamp(0, 1))
        hf = random.uniform(-0.1, 0.1)
        ops.append(lambda im: D._adjust_hue(im, hf))
        random.shuffle(ops)
        window = (slice(None), slice(None), slice(top, top + th), slice(left, left + tw))
        video = D._resize(video[window], h, w)
        for op in ops:
            video = op(video)
        mask = D._resize(mask[window], h, w)
    return video, mask.type(torch.bool).type(torch.float32)


def clip(seed, T=4, Hs=64, Ws=85):
    g = np.random.Generator(np.random.Philox(key=[77, seed]))
    frames = g.integers(0, 256, (T, Hs, Ws, 3), dtype=np.uint8)
    mask = np.zeros((T, Hs, Ws), np.uint8)
    for t in range(T):
        cy, cx = int(g.integers(4, Hs - 4)), int(g.integers(4, Ws - 4))
        mask[t, max(0, cy - 7):cy + 7, max(0, cx - 9):cx + 9] = 1
    return frames, mask


def seed_all(seed):
    random.seed(seed)
    torch.manual_seed(seed)


def test_draw_then_apply_replays_image_pipeline():
    shrinks = set()
    for seed in range(20):
        frames, mask = clip(seed)
        seed_all(seed)
        ref_img, ref_mask = legacy_pipeline(frames, mask.astype(np.float32), 48, 64, True)
        ref_state = (random.getstate(), torch.get_rng_state())
        seed_all(seed)
        cls_img, cls_mask = D.ImagePipeline(48, 64, True)(frames, mask.astype(np.float32))
        assert random.getstate() == ref_state[0] and torch.equal(torch.get_rng_state(), ref_state[1])
        seed_all(seed)
        p = D.draw_image_params(48, 64, True)
        assert random.getstate() == ref_state[0] and torch.equal(torch.get_rng_state(), ref_state[1])
        img, msk = D.apply_image_params(frames, mask.astype(np.float32), p)
        for got_i, got_m in ((cls_img, cls_mask), (img, msk)):
            assert got_i.dtype == torch.float32 and torch.equal(got_i, ref_img) and torch.equal(got_m, ref_mask)
        # the device mode's uint8 `mask != 0` gives the same binary mask
        assert torch.equal(D.apply_image_params(frames, (mask != 0).astype(np.uint8), p)[1], ref_mask)
        assert p.jitter and sorted(p.order) == [0, 1, 2, 3] and (p.h - p.th) == (p.w - p.tw)
        assert 0 <= p.top <= p.h - p.th and 0 <= p.left <= p.w - p.tw
        shrinks.add(p.h - p.th)
    assert 0 in shrinks and len(shrinks) >= 3, shrinks
    # without augmentation nothing is drawn and nothing but the resize is applied
    seed_all(5)
    before = (random.getstate(), torch.get_rng_state())
    p = D.draw_image_params(48, 64, False)
    assert random.getstate() == before[0] and torch.equal(torch.get_rng_state(), before[1])
    assert (p.top, p.left, p.th, p.tw, p.jitter) == (0, 0, 48, 64, False)
    frames, mask = clip(99)
    ref = legacy_pipeline(frames, mask.astype(np.float32), 48, 64, False)
    got = D.apply_image_params(frames, mask, p)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def cfg(root, **kw):
    d = dict(data_root=root, load_movement_info=False, video_length=8, n_past=1, n_future=2, action_dim=4, robot_dim=5,
             robot_joint_dim=7, impute_autograsp_action=False, image_width=64, image_height=48, seed=3,
             preload_ram=False, preprocess_action="raw", experiment="train_robonet", model_use_heatmap=False,
             train_val_split=0.75, img_augmentation=True, data_threads=0, batch_size=3, test_batch_size=2)
    d.update(kw)
    return argparse.Namespace(**d)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_robonet as mk
    root = str(tmp_path_factory.mktemp("robonet_dev"))
    assert mk.write(root, per_view=4, length=10, seed=1) == 16
    return root


def same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def test_device_mode_item(tree):
    c = cfg(tree)
    Xtr, _, ytr, _ = D.split_files(c)
    for augment in (True, False):
        seed_all(11)
        host = [D.RoboNetDataset(Xtr, ytr, c, augment_img=augment)[i] for i in (0, 5)]
        seed_all(11)
        dev = [D.RoboNetDataset(Xtr, ytr, c, augment_img=augment, device_images=True)[i] for i in (0, 5)]
        for h, d in zip(host, dev):
            assert set(d) == (set(h) - {"images", "masks"}) | {"frames", "raw_masks", "image_params"}
            assert d["frames"].dtype == torch.uint8 and tuple(d["frames"].shape) == (8, 64, 85, 3)
            assert d["raw_masks"].dtype == torch.uint8 and tuple(d["raw_masks"].shape) == (8, 64, 85)
            assert set(d["raw_masks"].unique().tolist()) <= {0, 1}
            for k in set(h) - {"images", "masks"}:
                assert same(h[k], d[k]), k
            p = d["image_params"]
            assert isinstance(p, D.ImageParams) and (p.h, p.w, p.jitter) == (48, 64, augment)
            img, msk = D.apply_image_params(d["frames"], d["raw_masks"], p)
            assert torch.equal(img, h["images"]) and torch.equal(msk, h["masks"])
    # the preload_ram cache keeps an item's parameters, as it keeps a host item's augmented frames
    ds = D.RoboNetDataset(Xtr[:2], ytr[:2], cfg(tree, preload_ram=True), augment_img=True, device_images=True)
    assert ds[1]["image_params"] == ds[1]["image_params"] and ds[1] is ds[1]


def test_cpu_batches_equal_host_mode(tree):
    batches = {}
    for on in (False, True):
        seed_all(21)
        train, test = D.create_loaders(cfg(tree, device_images=on))
        assert train.dataset._device_images is on and test.dataset._device_images is on
        gen, tgen = (D.get_batch(l, torch.device("cpu"), prefetch=False) for l in (train, test))
        batches[on] = [next(gen) for _ in range(5)] + [next(tgen)]  # 4 batches per epoch: into the second epoch
    for a, b in zip(batches[False], batches[True]):
        assert list(a) and set(a) == set(b)
        for k in a:
            assert same(a[k], b[k]), k
            if isinstance(a[k], torch.Tensor):
                assert a[k].shape == b[k].shape
        assert a["images"].shape[:1] == (8,) and a["images"].shape[2:] == (3, 48, 64)
    # the config flag reaches the parser, off by default
    from robot_aware_control_amd import config
    assert config.argparser([])[0].device_images is False
    assert config.argparser(["--device_images", "True"])[0].device_images is True


def test_transfer_and_finetune_loaders_pass_the_flag(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_robonet as mk
    mk.write(str(tmp_path), per_view=1, length=10, seed=2, locobot=3)
    c = cfg(str(tmp_path), robot_joint_dim=5, finetune_num_test=2, finetune_num_train=3, device_images=True)
    loaders = (D.create_transfer_loader(c),) + D.create_finetune_loaders(c)
    assert all(l.dataset._device_images for l in loaders)
    b = next(iter(loaders[0]))
    assert b["frames"].dim() == 1 and "images" not in b
    out = D.process_batch(b, torch.device("cpu"))
    assert out["images"].shape[0] == 8 and out["images"].shape[2:] == (3, 48, 64) and "frames" not in out


def test_collation_of_mixed_raw_sizes():
    items, refs = [], []
    for i, (Hs, Ws) in enumerate(((64, 85), (48, 64), (64, 85))):
        frames, mask = clip(100 + i, T=3, Hs=Hs, Ws=Ws)
        seed_all(40 + i)
        p = D.draw_image_params(48, 64, True)
        seed_all(40 + i)
        refs.append(D.ImagePipeline(48, 64, True)(frames, mask.astype(np.float32)))
        items.append({"frames": torch.from_numpy(frames), "raw_masks": torch.from_numpy(mask), "image_params": p,
                      "states": np.full((3, 5), i, np.float32), "robot": f"r{i}"})
    batch = D.collate(items)
    assert batch["frames"].dtype == torch.uint8 and batch["frames"].dim() == 1
    assert batch["frames"].numel() == 3 * 3 * (2 * 64 * 85 + 48 * 64) and batch["raw_masks"].numel() == 3 * (2 * 64 * 85 + 48 * 64)
    assert batch["image_shape"].tolist() == [3, 48, 64] and batch["robot"] == ["r0", "r1", "r2"]
    assert tuple(batch["states"].shape) == (3, 3, 5)
    jobs = batch["image_jobs"].numpy().reshape(-1).view(D.IMAGE_JOB)
    assert batch["image_jobs"].shape == (3, ctypes.sizeof(_lib.ImageJob))
    assert jobs["frame_offset"].tolist() == [0, 3 * 64 * 85 * 3, 3 * 64 * 85 * 3 + 3 * 48 * 64 * 3]
    assert jobs["mask_offset"].tolist() == [0, 3 * 64 * 85, 3 * 64 * 85 + 3 * 48 * 64]
    assert jobs["Hs"].tolist() == [64, 48, 64] and jobs["Ws"].tolist() == [85, 64, 85]
    for j, it in zip(jobs, items):
        p = it["image_params"]
        assert (j["top"], j["left"], j["th"], j["tw"], j["jitter"]) == (p.top, p.left, p.th, p.tw, 1)
        assert tuple(j["order"]) == p.order and tuple(j["factor"]) == p.factors  # the factors stay doubles
    images, masks = D.host_images(batch)
    for i, (img, msk) in enumerate(refs):
        assert torch.equal(images[i], img) and torch.equal(masks[i], msk)
    # a job that points outside its buffer is refused before anything is launched
    bad = dict(batch)
    bad["frames"] = batch["frames"][:-1]
    with pytest.raises(ValueError):
        D.host_images(bad)


def test_abi_of_the_image_job():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.ImageJob) == lib.rac_image_job_bytes() == D.IMAGE_JOB.itemsize == 96
    for name, _ in _lib.ImageJob._fields_:
        assert D.IMAGE_JOB.fields[name][1] == getattr(_lib.ImageJob, name).offset, name
    assert "rac_image_pipeline" in _lib.EXPORTS and "rac_image_job_bytes" in _lib.EXPORTS
    assert lib.rac_version() == 12
