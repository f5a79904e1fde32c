"""CPU: `data.experiment_loaders` -- every `--experiment` of the reference's trainer gets the reference's own split
(tests/golden/experiment_splits.json, recorded from the reference's loader functions by tools/gen_golden_splits.py over
the tree of tests/experiment_split_refs.py) -- and the host half of `--device_resident True`: the resident dataset draws
what the file-reading dataset draws, and the numerics of a whole video, sliced at a window, are the window's numerics
bit for bit (what lets `ResidentVideos` preprocess every video once)."""
import argparse
import json
import os
import pickle
import random
import sys
import types

import numpy as np
import pytest
import torch

import experiment_split_refs as refs
from robot_aware_control_amd import RacError
from robot_aware_control_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_synthetic_robonet as synth  # noqa: E402


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("splits"))
    refs.write_tree(root)
    return root


@pytest.fixture(scope="module")
def golden():
    with open(refs.GOLDEN) as f:
        return json.load(f)


def described(loader, root):
    ds = loader.dataset
    return {"files": [os.path.relpath(p, root) for p in ds._traj_names], "labels": list(ds._traj_robots),
            "augment": ds._images.augment, "batch_size": loader.batch_size,
            "shuffle": isinstance(loader.sampler, torch.utils.data.RandomSampler)}


# ------------------------------------------------------------------ splits
@pytest.mark.parametrize("seed", refs.SEEDS)
@pytest.mark.parametrize("experiment", refs.EXPERIMENTS)
def test_split_is_the_references(tree, golden, experiment, seed):
    """Files in order, labels, augmentation, batch size and shuffling of the train, test and transfer loaders."""
    want = golden[refs.case_key(experiment, seed)]
    train, test, transfer = D.experiment_loaders(refs.config(tree, experiment, seed, img_augmentation=True))
    assert described(train, tree) == want["train"]
    assert described(test, tree) == want["test"]
    assert (transfer is None) == (want["transfer"] is None)
    if transfer is not None:
        assert described(transfer, tree) == want["transfer"]


def test_sawyer_multiview_never_trains_on_the_transfer_view(tree):
    train, test, transfer = D.experiment_loaders(refs.config(tree, "train_sawyer_multiview", 0))
    seen = {os.path.basename(os.path.dirname(p)) for ds in (train.dataset, test.dataset) for p in ds._traj_names}
    assert seen == set(refs.SAWYER_VIEWS) - {"sudri2_c1"}
    assert {os.path.basename(os.path.dirname(p)) for p in transfer.dataset._traj_names} == {"sudri2_c1"}


def test_reference_module_paths_resolve_here():
    from src.dataset.locobot import locobot_singleview_dataloader as loco
    from src.dataset.locobot import locobot_table_dataloaders as table
    from src.dataset.sawyer import sawyer_dataloaders as sawyer
    from src.dataset.widowx import widowx_dataloaders as widowx
    assert sawyer.create_loaders is D.create_sawyer_loaders and sawyer.create_transfer_loader is D.create_sawyer_transfer_loader
    assert sawyer.create_finetune_loaders is D.create_sawyer_finetune_loaders
    assert widowx.create_finetune_loaders is D.create_widowx_finetune_loaders
    assert loco.create_loaders is D.create_locobot_loaders and loco.create_finetune_loaders is D.create_finetune_loaders
    assert loco.create_transfer_loader is D.create_transfer_loader
    assert table.create_loaders is D.create_locobot_table_loaders


def test_movement_table_replaces_a_missing_world_error_dict(tmp_path):
    """Without --world_error_dict the folder's obj_movement.pkl selects the files: the same split as with the pickle
    that carries the same flags; a folder nobody scored names the command that scores it."""
    root = str(tmp_path)
    refs.write_tree(root, movement_tables=True)
    for experiment in ("finetune_widowx", "finetune_sawyer_view"):
        with_dict = D.experiment_loaders(refs.config(root, experiment, 3))
        without = D.experiment_loaders(refs.config(root, experiment, 3, world_error_dict=None))
        for a, b in zip(with_dict[:2], without[:2]):
            assert described(a, root) == described(b, root)
        kept = {int(os.path.basename(p)[5:8]) for ld in without[:2] for p in ld.dataset._traj_names}
        assert kept and all(refs.moves(i) for i in kept)
    os.remove(os.path.join(root, "widowx_views", "widowx1_c0", D.MOVEMENT_FILE))
    with pytest.raises(FileNotFoundError, match="measure_obj_movement"):
        D.experiment_loaders(refs.config(root, "finetune_widowx", 3, world_error_dict=None))


def test_unknown_experiment_raises_its_name(tree):
    for experiment in ("train_locobot_pick", "eval_franka", "control_franka"):
        with pytest.raises(NotImplementedError, match=experiment):
            D.experiment_loaders(refs.config(tree, experiment, 0))


def test_stale_singlerobot_value_keeps_the_robonet_split(tree):
    """`--experiment singlerobot` (published command lines; not in the reference's parser) ran on the RoboNet split
    before `experiment_loaders` and still does, without a transfer set."""
    train, test, transfer = D.experiment_loaders(refs.config(tree, "singlerobot", 0))
    want = D.experiment_loaders(refs.config(tree, "train_robonet", 0), transfer=False)
    assert described(train, tree) == described(want[0], tree) and described(test, tree) == described(want[1], tree)
    assert transfer is None


def test_flags_parse():
    from robot_aware_control_amd import config
    d, _ = config.argparser([])
    assert d.device_resident is False and d.device_resident_max_gb == 16.0
    cf, _ = config.argparser(["--device_resident", "True", "--device_resident_max_gb", "2.5",
                              "--experiment", "finetune_widowx"])
    assert cf.device_resident is True and cf.device_resident_max_gb == 2.5


# ------------------------------------------------------------------ the trainer's front door
@pytest.fixture(scope="module")
def videos(tmp_path_factory):
    """A synthetic RoboNet tree with real videos (12..14 frames of 64x85) and locobot views, every widowx / sudri2_c1 file
    marked as high-movement."""
    root = str(tmp_path_factory.mktemp("videos"))
    synth.write(root, per_view=5, length=12, locobot=5)
    info = {}
    for folder in ("widowx_views/widowx1_c0", "sawyer_views/sudri2_c1"):
        for d in os.scandir(os.path.join(root, folder)):
            info[d.path] = [{"high_error": True}]
    with open(os.path.join(root, refs.WORLD_ERROR), "wb") as f:
        pickle.dump(info, f)
    return root


def video_config(root, experiment="finetune_widowx", **kw):
    base = dict(finetune_num_test=2, finetune_num_train=3, batch_size=2, test_batch_size=2, video_length=8)
    base.update(kw)
    return refs.config(root, experiment, 3, **base)


def trainer(cf):
    from robot_aware_control_amd.trainer import PredictionTrainer
    tr = object.__new__(PredictionTrainer)
    tr._config, tr._device = cf, torch.device("cpu")
    return tr


def test_setup_data_trains_finetune_widowx_on_widowx_only(videos):
    """(Before `experiment_loaders` the run trained on baxter + widowx + sawyer under every --experiment.)"""
    tr = trainer(video_config(videos))
    batches, test_loader = tr._setup_data()
    folders = set()
    for _ in range(4):
        batch = next(batches)
        assert batch["images"].shape[:2] == (8, len(batch["folder"]))  # time-first, from process_batch
        folders |= set(batch["folder"])
    assert folders == {"widowx1_c0"}
    assert {os.path.basename(os.path.dirname(p)) for p in test_loader.dataset._traj_names} == {"widowx1_c0"}
    assert len(test_loader.dataset) == 2 and not hasattr(tr, "transfer_loader")


def test_setup_data_synthetic_root_is_unchanged():
    """`--data_root synthetic` feeds the generator under every experiment, files or not."""
    from robot_aware_control_amd.synthetic import synth_video
    cf = video_config("synthetic", n_eval=3, channels=3)
    gen, test = trainer(cf)._setup_data()
    first = next(gen)
    want = synth_video(cf.seed + 1, cf.video_length, cf.batch_size, cf.image_height, cf.image_width, cf.robot_dim,
                       cf.action_dim)
    assert all(torch.equal(first[k], want[k]) for k in ("images", "masks", "states", "actions"))
    assert isinstance(test.dataset, D.SyntheticVideoDataset) and len(test.dataset) == 2 * cf.test_batch_size


# ------------------------------------------------------------------ the resident dataset's choices
def reseed(seed=11):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def lengths_of(ds):
    out = []
    for name in ds._traj_names:
        with D.open_trajectory(os.path.join(ds._data_root, name)) as traj:
            out.append(traj[D.picture_keys(traj, name)[0]].shape[0])
    return np.array(out)


@pytest.mark.parametrize("augment", [False, True])
def test_resident_dataset_draws_what_the_file_reader_draws(videos, augment):
    """Two epochs of a shuffled loader with data_threads=0 and the same seed: the same (idx, start, ImageParams) in the
    same order from the file-reading device_images dataset and from the resident dataset, which opens no file.  The
    videos have 12..14 frames for windows of 8, so every start is drawn; `video_length=12` adds videos that are exactly
    one window long, for which nothing is drawn."""
    for length in (8, 12):
        cf = video_config(videos, "train_robonet", device_images=True, img_augmentation=augment, video_length=length,
                          train_val_split=0.75, batch_size=3)
        X_train, _, y_train, _ = D.split_files(cf)
        reseed()
        ds = D.RoboNetDataset(X_train, y_train, cf, augment_img=augment, device_images=True)
        loader = D._plain_loader(ds, cf, cf.batch_size)
        stored = {i: np.load(p)["qpos"].astype(np.float32) for i, p in enumerate(X_train)}
        want = []
        for _ in range(2):
            for i in iter(loader.sampler):
                item = ds[i]
                (hits,) = np.nonzero((stored[i] == item["qpos"][0]).all(1))
                want.append((i, int(hits[0]), item["image_params"]))
        reseed()
        base = D.RoboNetDataset(X_train, y_train, cf, augment_img=augment, device_images=True)
        store = types.SimpleNamespace(lengths_host=lengths_of(base), paths=list(X_train))  # (all the dataset reads of it)
        resident = D.ResidentDataset(base, store)
        order = D._plain_loader(resident, cf, cf.batch_size)
        assert order.num_workers == 0
        calls = []
        orig = D.open_trajectory
        D.open_trajectory = lambda p: calls.append(p) or orig(p)
        try:
            got = [tuple(resident[i])[:3] for _ in range(2) for i in iter(order.sampler)]
        finally:
            D.open_trajectory = orig
        assert got == want and not calls
        assert len({s for _, s, _ in got}) > 1 or length == 12
        if augment:
            assert any(p.jitter and (p.th, p.tw) != (p.h, p.w) for _, _, p in got)


# ------------------------------------------------------------------ whole-video numerics, sliced
def rigid(seed):
    g = np.random.RandomState(seed)
    q, _ = np.linalg.qr(g.randn(3, 3))
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, g.randn(3)
    return m


@pytest.mark.parametrize("strategy", ["raw", "camera_raw"])
def test_whole_video_numerics_sliced_are_the_windows_numerics(videos, monkeypatch, strategy):
    """Per file of a RoboNet viewpoint and of a locobot one: `numerics` over the WHOLE stored video, sliced at the window
    the item drew, equals the item's states / actions / qpos (+ raw_* and the bounds under finetune_* with a camera
    strategy) with np.array_equal.  The camera strategies go through a 4x4 float64 matmul over all rows: this is the
    test that it gives a row the same bits whatever the row count."""
    views = ("sawyer_sudri0_c0", "locobot_c0")
    w2c = {v: rigid(k) for k, v in enumerate(views)}
    monkeypatch.setattr(D, "_camera_dicts", lambda: (w2c, {v: np.linalg.inv(m) for v, m in w2c.items()}))
    cf = video_config(videos, "finetune_locobot", preprocess_action=strategy, video_length=5)
    files, labels = [], []
    for folder, label in (("sawyer_views/sudri0_c0", views[0]), ("locobot_views/c0", views[1])):
        paths = sorted(d.path for d in os.scandir(os.path.join(videos, folder)) if d.path.endswith(".npz"))
        files += paths
        labels += [label] * len(paths)
    ds = D.RoboNetDataset(files, labels, cf)
    starts = set()
    for i, (path, label) in enumerate(zip(files, labels)):
        item = ds[i]
        pipe = ds.pipeline(label)
        with D.open_trajectory(path) as traj:
            n = traj[D.picture_keys(traj, path)[0]].shape[0]
            whole = ds.numerics(pipe, ds.stored_numerics(traj, pipe, 0, n), item["folder"], path)
        (hits,) = np.nonzero((np.asarray(whole["qpos"]) == np.asarray(item["qpos"])[0]).all(1))
        s = int(hits[0])
        starts.add(s)
        keys = ["states", "actions", "qpos"] + (["raw_states", "raw_actions"] if strategy != "raw" else [])
        assert set(keys) <= set(item)
        for k in keys:
            rows = 5 - (k in D.STEP_TABLES)
            got, want = np.asarray(whole[k])[s:s + rows], np.asarray(item[k])
            assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want), (path, k)
        for k in [k for k in D.VIDEO_TABLES if k in item]:
            assert np.array_equal(whole[k], item[k]), (path, k)
        assert ("raw_low" in item) == (strategy != "raw") and "low" in item
    assert len(starts) > 2 and max(starts) > 0  # (windows inside the videos, not only their heads)


# ------------------------------------------------------------------ guards
def test_resident_guards(videos):
    cf = video_config(videos, device_resident=True, device=torch.device("cuda:0"), device_resident_max_gb=1e-4)
    # the cap: named with the size and the flag, before anything is allocated (this machine may not even have a GPU)
    with pytest.raises(ValueError, match=r"0\.00 GB.*--device_resident_max_gb"):
        D.experiment_loaders(cf)
    with pytest.raises(ValueError, match="--preload_ram.*--device_resident"):
        D.experiment_loaders(video_config(videos, device_resident=True, preload_ram=True, device=torch.device("cuda:0")))
    with pytest.raises(RacError, match="no CPU fallback"):
        D.experiment_loaders(video_config(videos, device_resident=True, device=torch.device("cpu")))
