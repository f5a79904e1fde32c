"""GPU: `--device_resident True` -- `rac_window_gather` (csrc/rac_joint.hip) against numpy indexing, the resident feed
(`ResidentVideos` -> `collate` -> `process_batch` / `DevicePrefetcher`) against the loader-fed `--device_images True`
path batch by batch with torch.equal, and `_compute_epoch_metrics` over a resident test loader.  Both feeds end in the
same `rac_image_pipeline` arithmetic on the same bytes and in copies of the same host-computed numerics, so equality is
exact."""
import ctypes as C
import os
import random
import shutil
import sys

import numpy as np
import pytest
import torch

import experiment_split_refs as refs
from robot_aware_control_amd import _lib
from robot_aware_control_amd import data as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_synthetic_robonet as synth  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------ rac_window_gather
LENGTHS, L, PAD = np.array([5, 3, 4]), 3, -777.0
# a repeated video; start 0, the last admissible start of videos 0 (2) and 2 (1), and video 1, exactly one window long
INDEX, START = np.array([0, 2, 1, 0]), np.array([2, 1, 0, 0])
# name -> (width, per video, rows of a window, rows stored): per frame 5 and 7 wide, per step, per video 5 and 17 wide
TABLES = {"states": (5, False, L, 5), "qpos": (7, False, L, 5), "actions": (5, False, L - 1, 4),
          "low": (5, True, 1, 1), "view": (17, True, 1, 1)}


@pytest.fixture(scope="module")
def tables():
    """Host tables padded to the longest video with a value no window may show."""
    g = np.random.Generator(np.random.Philox(key=[9, 1]))
    out = {}
    for name, (width, per_video, rows, stored) in TABLES.items():
        if per_video:
            out[name] = g.normal(size=(len(LENGTHS), width)).astype(np.float32)
            continue
        t = np.full((len(LENGTHS), stored, width), PAD, np.float32)
        for v, n in enumerate(LENGTHS):
            n = n - (rows == L - 1)
            t[v, :n] = g.normal(size=(n, width)).astype(np.float32)
        out[name] = t
    return out


def expected(tables):
    out = {}
    for name, (width, per_video, rows, _) in TABLES.items():
        t = tables[name]
        out[name] = t[INDEX] if per_video else np.stack([t[i, s:s + rows] for i, s in zip(INDEX, START)], 1)
    return out


def gather(tables, dev):
    up = lambda a: torch.from_numpy(a).to(dev)
    index, start = D.check_windows(INDEX, START, LENGTHS, L)
    return D.window_gather([(k, up(tables[k]), TABLES[k][1], TABLES[k][2]) for k in TABLES], up(index), up(start),
                           up(LENGTHS.astype(np.int32)), L)


def test_window_gather_is_numpy_indexing(dev, tables):
    want = expected(tables)
    assert not any((w == PAD).any() for w in want.values())  # (the cases stay inside the videos)
    got = gather(tables, dev)
    again = gather(tables, dev)
    for name, (width, per_video, rows, _) in TABLES.items():
        assert tuple(got[name].shape) == ((len(INDEX), width) if per_video else (rows, len(INDEX), width))
        assert torch.equal(got[name].cpu(), torch.from_numpy(want[name])), name
        assert torch.equal(got[name], again[name]), name


def test_window_gather_more_than_one_block_and_nine_tables(dev):
    """More elements than one workgroup covers (and than the grid cap times 256 covers in one stride), an odd width, and
    9 tables: two launches."""
    g = np.random.Generator(np.random.Philox(key=[9, 2]))
    V, Lmax, Lw, B = 37, 11, 4, 300
    lengths = g.integers(Lw, Lmax + 1, V)
    index = g.integers(0, V, B)
    start = np.array([g.integers(0, lengths[i] - Lw + 1) for i in index])
    host = {f"t{k}": g.normal(size=(V, Lmax, 7 + 30 * k)).astype(np.float32) for k in range(9)}
    up = lambda a: torch.from_numpy(a).to(dev)
    i32, s32 = D.check_windows(index, start, lengths, Lw)
    got = D.window_gather([(k, up(t), False, Lw) for k, t in host.items()], up(i32), up(s32),
                          up(lengths.astype(np.int32)), Lw)
    assert sum(v.numel() for v in got.values()) > 1024 * 256
    for k, t in host.items():
        assert torch.equal(got[k].cpu(), torch.from_numpy(np.stack([t[i, s:s + Lw] for i, s in zip(index, start)], 1))), k


def test_range_check_refuses_before_any_launch(dev, monkeypatch):
    launched = []
    monkeypatch.setattr(_lib, "call", lambda *a: launched.append(a))
    for index, start in ((np.array([len(LENGTHS)]), np.array([0])), (np.array([0]), np.array([LENGTHS[0] - L + 1])),
                         (np.array([1]), np.array([1])), (np.array([-1]), np.array([0])), (np.array([0]), np.array([-1]))):
        with pytest.raises(ValueError, match="resident batch"):
            D.check_windows(index, start, LENGTHS, L)
    assert not launched


def test_window_gather_refuses_bad_arguments(dev):
    lib = _lib.load()
    src, dst = torch.zeros(3, 5, 5, device=dev), torch.zeros(3, 4, 5, device=dev)
    ints = torch.zeros(4, dtype=torch.int32, device=dev)
    ok = (src.data_ptr(), dst.data_ptr(), 5, 5, 3, 0)
    stream = _lib.stream_ptr()

    def status(records, n, V=3, B=4, Lw=3, tables=True):
        array = (_lib.GatherTable * len(records))(*records)
        rc = lib.rac_window_gather(C.cast(array, C.c_void_p) if tables else None, n, ints.data_ptr(), ints.data_ptr(),
                                   ints.data_ptr(), V, B, Lw, stream)
        assert rc == 0 or lib.rac_last_error()
        return rc

    assert status([ok], 1) == 0
    assert status([ok], 1, tables=False) != 0 and b"NULL" in lib.rac_last_error()
    assert status([(None, dst.data_ptr(), 5, 5, 3, 0)], 1) != 0
    assert status([(src.data_ptr(), None, 5, 5, 3, 0)], 1) != 0
    assert status([ok] * 9, 9) != 0 and b"9 tables" in lib.rac_last_error()
    assert status([ok], 0) != 0
    for kw in ({"V": 0}, {"B": 0}, {"Lw": 0}):
        assert status([ok], 1, **kw) != 0
    assert status([(src.data_ptr(), dst.data_ptr(), 5, 0, 3, 0)], 1) != 0   # width 0
    assert status([(src.data_ptr(), dst.data_ptr(), 2, 5, 3, 0)], 1) != 0   # fewer rows stored than a window
    assert status([(src.data_ptr(), dst.data_ptr(), 5, 5, 1, 0)], 1) != 0   # rows neither L nor L - 1
    assert status([(src.data_ptr(), dst.data_ptr(), 1, 5, 3, 1)], 1) != 0   # a per-video table of 3 rows
    torch.cuda.synchronize(dev)


# ------------------------------------------------------------------ the resident feed against the loader feed
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """4 files per view of 8..10 frames; widowx1_c0 and locobot c1 are stored 40x52, the rest 64x85."""
    root = str(tmp_path_factory.mktemp("resident"))
    other = str(tmp_path_factory.mktemp("other_size"))
    synth.write(root, per_view=4, length=8, seed=2, locobot=4)
    synth.write(other, per_view=4, length=8, seed=5, h=40, w=52, locobot=4)
    for folder in ("widowx_views/widowx1_c0", "locobot_views/c1"):
        shutil.rmtree(os.path.join(root, folder))
        shutil.copytree(os.path.join(other, folder), os.path.join(root, folder))
    return root


def reseed(seed=17):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def config(tree, dev, experiment, resident, **kw):
    base = dict(device=dev, device_images=True, device_resident=resident, video_length=5, batch_size=3,
                test_batch_size=2, finetune_num_test=3, finetune_num_train=5, train_val_split=0.75,
                device_resident_max_gb=1.0)
    base.update(kw)
    return refs.config(tree, experiment, 3, **base)


def same(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, v in want.items():
        if torch.is_tensor(v):
            assert torch.is_tensor(got[k]) and got[k].dtype == v.dtype and torch.equal(got[k].cpu(), v.cpu()), k
        else:
            assert list(got[k]) == list(v), k
    for k in D.TRANSPOSE_KEYS:
        assert k not in got or got[k].is_cuda, k


def passes(loader, dev, epochs, prefetch):
    """`epochs` passes of `get_batch`'s batches; the prefetcher's thread is stopped and joined before the next reseed."""
    n = epochs * len(loader)
    if not prefetch:
        gen = D.get_batch(loader, dev, prefetch=False)
        return [next(gen) for _ in range(n)]
    feed = D.DevicePrefetcher(loader, dev)
    out = [next(feed) for _ in range(n)]
    torch.cuda.synchronize(dev)
    feed.close()
    feed.thread.join(30)
    assert not feed.thread.is_alive()
    return out


CASES = [(exp, size, aug, False) for exp in ("finetune_locobot", "train_robonet") for size in ((8, 8), (48, 64))
         for aug in (False, True)] + [("train_robonet", (48, 64), True, True)]


@pytest.mark.parametrize("experiment,size,augment,heatmap", CASES)
def test_resident_batches_equal_loader_batches(dev, tree, tmp_path, monkeypatch, experiment, size, augment, heatmap):
    """Two epochs of the train loader and one of the test loader, through `process_batch` and through the prefetcher: every
    tensor key torch.equal, every string key equal.  Once its stores are built the resident pass opens no trajectory
    file, and a batch uploads its job array and its (index, start) pairs -- and, under --model_use_heatmap, the camera
    records the loader path uploads too."""
    kw = dict(image_height=size[0], image_width=size[1], img_augmentation=augment)
    if heatmap:
        import heatmap_refs as hr
        cameras = str(tmp_path / "cameras.npz")
        hr.synthetic_root_table().save(cameras)
        kw.update(model_use_heatmap=True, camera_calibration=cameras)
    want = {}
    for prefetch in (False, True):
        reseed()
        train, test, _ = D.experiment_loaders(config(tree, dev, experiment, False, **kw))
        want[prefetch] = passes(train, dev, 2, prefetch) + passes(test, dev, 1, prefetch)
    assert len({b["images"].shape[1] for b in want[False]}) > 1 or experiment == "finetune_locobot"
    opened, uploaded = [], []
    orig_open, orig_to = D.open_trajectory, torch.Tensor.to

    def counting_to(self, *a, **k):
        out = orig_to(self, *a, **k)
        if not self.is_cuda and out.is_cuda:
            uploaded.append(self.numel() * self.element_size())
        return out

    for prefetch in (False, True):
        reseed()
        train, test, _ = D.experiment_loaders(config(tree, dev, experiment, True, **kw))
        assert isinstance(train.dataset, D.ResidentDataset) and train.num_workers == 0
        monkeypatch.setattr(D, "open_trajectory", lambda p: opened.append(p) or orig_open(p))
        if not prefetch:
            monkeypatch.setattr(torch.Tensor, "to", counting_to)
        got = passes(train, dev, 2, prefetch) + passes(test, dev, 1, prefetch)
        monkeypatch.setattr(torch.Tensor, "to", orig_to)
        monkeypatch.setattr(D, "open_trajectory", orig_open)
        assert len(got) == len(want[prefetch])
        for g, w in zip(got, want[prefetch]):
            same(g, w)
        assert not opened
    from robot_aware_control_amd.heatmaps import VIEW
    per_sample = D.IMAGE_JOB.itemsize + 2 * 4 + (VIEW.itemsize if heatmap else 0)
    assert sum(uploaded) == per_sample * sum(b["images"].shape[1] for b in want[False])
    assert len(uploaded) == (3 if heatmap else 2) * len(want[False])


def test_resident_store_layout(dev, tree):
    """What the store holds: whole videos of both raw sizes back to back, tables padded to the longest video."""
    reseed()
    train, _, _ = D.experiment_loaders(config(tree, dev, "train_robonet", True))
    store = train.dataset.store
    assert {tuple(s[1:]) for s in store.shapes} == {(64, 85), (40, 52)} and len(set(store.shapes[:, 0])) > 1
    V, Lmax = len(store), int(store.shapes[:, 0].max())
    assert store.frames.numel() == 3 * store.raw_masks.numel() == 3 * int(store.shapes.prod(1).sum())
    assert tuple(store.tables["states"].shape) == (V, Lmax, 5) and tuple(store.tables["actions"].shape) == (V, Lmax - 1, 4)
    assert tuple(store.tables["qpos"].shape) == (V, Lmax, 7) and set(store.tables) == {"states", "actions", "qpos"}
    i = int(np.argmin(store.shapes[:, 0]))
    with D.open_trajectory(store.paths[i]) as traj:
        frames = traj[D.picture_keys(traj, store.paths[i])[0]][:]
    f0 = int(store.frame_offsets[i])
    assert torch.equal(store.frames[f0:f0 + frames.size].cpu(), torch.from_numpy(frames.reshape(-1)))
    assert store.nbytes() < 2 ** 30


# ------------------------------------------------------------------ evaluation over a resident loader
def test_epoch_metrics_over_a_resident_test_loader(dev, tree, tmp_path):
    """One test batch of 4 videos through `_compute_epoch_metrics`, loader-fed and resident: the same scalars.  The batch
    itself is bit-equal (the tests above), and every loss key is computed in a fixed order: those are compared with ==.
    The PSNR / SSIM keys are not reproducible bit for bit on ANY feed: `rac_psnr_ssim` adds the partial sums of a video's
    16 tiles x 3 channels (64x64 frames) with one float atomicAdd each, in the order the workgroups happen to finish.
    Two orders of m = 48 fp32 partials differ by at most 2 (m - 1) 2^-24 times the sum of their magnitudes; an SSIM
    value is at most 1 and the squared error is a sum of non-negative terms, so the mean SSIM differs by at most
    2 * 47 * 2^-24 = 5.7e-6 and the squared error by that relative amount, which moves a PSNR by at most
    10 / ln(10) * 5.7e-6 = 2.5e-5 dB.  (Measured on an MI355X: three SSIM keys differed, by 1.5e-8 at most.)"""
    from robot_aware_control_amd.config import argparser
    from robot_aware_control_amd.trainer import PredictionTrainer
    argv = ("--jobname t --wandb False --batch_size 2 --test_batch_size 4 --n_future 2 --n_past 1 --n_eval 4 --g_dim 32 "
            "--z_dim 8 --model svg --reconstruction_loss dontcare_l1 --last_frame_skip True --action_dim 4 --robot_dim 5 "
            "--robot_joint_dim 7 --data_threads 0 --experiment train_robonet --model_use_robot_state True "
            "--model_use_mask True --model_use_future_mask True --video_length 8 --image_height 64 --image_width 64 "
            f"--train_val_split 0.75 --device_images True --seed 3 --data_root {tree} --log_dir {tmp_path / 'log'}").split()
    cfg, _ = argparser(argv)
    cfg.device = dev
    torch.manual_seed(5)
    tr = PredictionTrainer(cfg)
    tr.model.eval()
    scalars = []
    for resident in (False, True):
        cfg.device_resident = resident
        reseed()
        _, test, _ = D.experiment_loaders(cfg, transfer=False)
        assert len(test) == 1 and isinstance(test.dataset, D.ResidentDataset) == resident
        scalars.append(tr._compute_epoch_metrics(test, "test"))
    assert scalars[0] and all(np.isfinite(v) for v in scalars[0].values())
    assert set(scalars[0]) == set(scalars[1])
    reorder = 2 * 47 * 2.0 ** -24
    for k, v in scalars[0].items():
        print(k, v, scalars[1][k], v - scalars[1][k])
        if "ssim" in k:
            assert abs(v - scalars[1][k]) <= reorder, k
        elif "psnr" in k:
            assert abs(v - scalars[1][k]) <= 10 / np.log(10) * reorder, k
        else:
            assert v == scalars[1][k], k
