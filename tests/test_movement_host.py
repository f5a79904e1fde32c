"""CPU: the host side of the object-movement pass -- the `rac_video_movement` symbol in the header, the ctypes table and
the export list, the threshold table, `create_movement_loader`'s file selection over hand-written tables, the command
line of `src.prediction.measure_obj_movement`, the `src.*` import paths, and the test reference on a case done by hand."""
import argparse
import os
import pickle
import re
from collections import defaultdict

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cfg(root, **kw):
    d = dict(data_root=str(root), load_movement_info=False, video_length=8, n_past=1, n_future=7, action_dim=4, robot_dim=5,
             robot_joint_dim=7, impute_autograsp_action=False, image_width=16, image_height=16, seed=3,
             preload_ram=False, preprocess_action="raw", experiment="train_robonet", model_use_heatmap=False,
             img_augmentation=False, data_threads=0, batch_size=2, test_batch_size=2)
    d.update(kw)
    return argparse.Namespace(**d)


def test_header_sigs_and_exports_carry_rac_video_movement():
    import ctypes as C
    from robot_aware_control_amd import EXPORTS, _lib
    hdr = open(os.path.join(ROOT, "include", "rac_hip.h")).read()
    assert re.search(r"^int\s+rac_video_movement\s*\(", hdr, flags=re.M)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert _lib._SIGS["rac_video_movement"] == [vp, i64, i64, vp, i64, i64, vp, vp, i32, i32, i32, i32, vp]
    assert "rac_video_movement" in EXPORTS
    assert _lib.ABI_VERSION == 12
    assert "#define RAC_ABI_VERSION 12" in hdr


def test_thresholds_are_the_twelve_of_the_reference():
    from robot_aware_control_amd.movement import MOVEMENT_THRESHOLDS, ROBOT_VIEWPOINTS
    assert set(MOVEMENT_THRESHOLDS) == {
        "sawyer_sudri0_c0", "sawyer_sudri0_c1", "sawyer_sudri0_c2", "sawyer_vestri_table2_c0", "sawyer_vestri_table2_c1",
        "sawyer_vestri_table2_c2", "sawyer_sudri2_c0", "sawyer_sudri2_c1", "sawyer_sudri2_c2", "baxter_left_c0",
        "widowx_widowx1_c0", "locobot_c0"}
    assert MOVEMENT_THRESHOLDS["baxter_left_c0"] == 0.017 and MOVEMENT_THRESHOLDS["widowx_widowx1_c0"] == 0.11
    # every folder the command line walks has a threshold
    assert {f"{r}_{v}" for r, vs in ROBOT_VIEWPOINTS.items() for v in vs} == set(MOVEMENT_THRESHOLDS)


def test_unknown_viewpoint_without_threshold_is_a_key_error(tmp_path):
    from robot_aware_control_amd.movement import measure_obj_movement
    with pytest.raises(KeyError, match="franka_c9"):
        measure_obj_movement("franka", "c9", cfg(tmp_path))


def test_existing_table_is_kept(tmp_path):
    """The refusal comes before anything is read or scored (no GPU needed to see it)."""
    from robot_aware_control_amd.movement import measure_obj_movement
    folder = tmp_path / "baxter_views" / "left_c0"
    folder.mkdir(parents=True)
    (folder / "obj_movement.pkl").write_bytes(pickle.dumps({"kept": True}))
    with pytest.raises(FileExistsError, match="overwrite"):
        measure_obj_movement("baxter", "left_c0", cfg(tmp_path))
    assert pickle.loads((folder / "obj_movement.pkl").read_bytes()) == {"kept": True}


def placeholder_tree(root, tables):
    """{(robot, view): {file name: flag or None}} -> empty trajectory files; a pkl over the non-None entries per view
    (a view whose dict is all None gets no pkl).  Returns {robot: [flagged paths]}."""
    flagged = defaultdict(list)
    for (robot, view), entries in tables.items():
        d = os.path.join(str(root), f"{robot}_views", view)
        os.makedirs(d)
        table = defaultdict(bool)
        for name, flag in entries.items():
            path = os.path.join(d, name)
            open(path, "wb").close()
            if flag is not None:
                table[path] = flag
                if flag:
                    flagged[robot].append(path)
        if any(f is not None for f in entries.values()):
            with open(os.path.join(d, "obj_movement.pkl"), "wb") as f:
                pickle.dump(table, f)
    return flagged


def test_movement_loader_selects_the_flagged_files(tmp_path):
    from robot_aware_control_amd import data
    from tests.movement_refs import expected_order
    names = {f"traj_{i:03d}.npz": i % 3 != 0 for i in range(9)}
    tables = {("baxter", "left_c0"): dict(names, **{"traj_100.hdf5": True, "notes.txt": True}),
              ("sawyer", "sudri0_c0"): {f"s_{i}.npz": i < 2 for i in range(5)},
              ("sawyer", "sudri2_c1"): {"t_0.npz": False, "t_1.npz": True, "unlisted.npz": None, "x.npz": False},
              ("sawyer", "not_a_train_dir"): {"u_0.npz": True}}  # (no widowx_views folder at all: skipped)
    flagged = placeholder_tree(tmp_path, tables)
    flagged["baxter"] = [p for p in flagged["baxter"] if not p.endswith(".txt")]
    flagged["sawyer"] = [p for p in flagged["sawyer"] if "not_a_train_dir" not in p]
    assert len(flagged["baxter"]) == 7 and len(flagged["sawyer"]) == 3
    c = cfg(tmp_path)
    want = expected_order(flagged["baxter"] + flagged["sawyer"], c.seed)
    files, labels = data.movement_files(c)
    assert files == want and len(files) == 10
    assert labels == [f"{p.split(os.sep)[-3][:-len('_views')]}_{p.split(os.sep)[-2]}" for p in files]
    loader = data.create_movement_loader(c)
    assert loader.dataset._traj_names == want and loader.batch_size == c.batch_size
    assert loader.dataset._images.augment is False
    # the cap (4000 in the reference) through the small parameter
    assert data.movement_files(c, n_files=4)[0] == want[:4]
    assert data.create_movement_loader(c, n_files=4).dataset._traj_names == want[:4]
    # `_robot_files` without the predicate finds what it found before
    every = data._robot_files(c, "baxter_views", data.BAXTER_TRAIN_DIRS, "baxter")
    assert len(every) == 10 and all(lb == "baxter_left_c0" for _, lb in every)


def test_movement_loader_names_the_command_when_a_table_is_missing(tmp_path):
    from robot_aware_control_amd import data
    placeholder_tree(tmp_path, {("baxter", "left_c0"): {"a.npz": True}, ("widowx", "widowx1_c0"): {"b.npz": None}})
    with pytest.raises(FileNotFoundError) as e:
        data.create_movement_loader(cfg(tmp_path))
    msg = str(e.value)
    assert os.path.join("widowx_views", "widowx1_c0", "obj_movement.pkl") in msg
    assert "python -m src.prediction.measure_obj_movement" in msg


def test_command_line_defaults_and_views():
    from robot_aware_control_amd import config as rc
    from src.prediction import measure_obj_movement as cli
    table_before = [list(t) for t in (rc._GENERAL, rc._PREDICTION, rc._DATASET, rc._COST, rc._CEM, rc._COMPAT, rc._NATIVE)]
    config, tool = cli.parse_args(["--data_root", "/data/robonet"])
    assert (config.video_length, config.n_past, config.n_future, config.image_width, config.action_dim) == (31, 1, 30, 64, 5)
    assert config.image_height == 48 and config.data_root == "/data/robonet"
    assert tool.views is None and tool.threshold is None and tool.overwrite is False
    pairs = cli.parse_views(tool.views)
    assert pairs[0] == ("baxter", "left_c0") and pairs[1] == ("widowx", "widowx1_c0") and len(pairs) == 12
    config, tool = cli.parse_args(["--views", "baxter/left_c0,sawyer/vestri_table2_c1", "--n_future", "9", "--threshold",
                                   "0.25", "--overwrite", "True", "--batch_size", "16", "--image_width", "32"])
    assert cli.parse_views(tool.views) == [("baxter", "left_c0"), ("sawyer", "vestri_table2_c1")]
    assert tool.threshold == 0.25 and tool.overwrite is True
    assert (config.n_future, config.batch_size, config.image_width, config.video_length) == (9, 16, 32, 31)
    with pytest.raises(ValueError, match="robot/viewpoint_folder"):
        cli.parse_views(["left_c0"])
    with pytest.raises(AssertionError):
        cli.parse_args(["--no_such_flag", "1"])
    # the trainer's own parser knows nothing of the tool's flags and keeps its defaults
    assert [list(t) for t in (rc._GENERAL, rc._PREDICTION, rc._DATASET, rc._COST, rc._CEM, rc._COMPAT, rc._NATIVE)] == table_before
    plain = rc.create_parser("FetchPush")
    assert plain.get_default("n_future") == 9 and plain.get_default("action_dim") == 2
    assert not any(a.dest in ("views", "threshold", "overwrite") for a in plain._actions)


def test_reference_import_paths():
    from robot_aware_control_amd import data, movement
    from src.dataset.robonet import robonet_dataloaders as rd
    from src.prediction import measure_obj_movement as cli
    from src.prediction.evaluation import evaluate_obj_movement as ev
    assert cli.measure_obj_movement is movement.measure_obj_movement
    assert cli.MOVEMENT_THRESHOLDS is movement.MOVEMENT_THRESHOLDS
    assert rd.create_movement_loader is data.create_movement_loader and rd.create_loaders is data.create_loaders
    assert ev.create_movement_loader is data.create_movement_loader and callable(ev.compute_metrics)


def test_ops_video_movement_refuses_cpu_tensors():
    from robot_aware_control_amd import _lib, ops
    with pytest.raises(_lib.RacError, match="GPU only"):
        ops.video_movement(torch.zeros(3, 1, 3, 4, 4), torch.zeros(3, 1, 1, 4, 4))


def test_reference_formula_by_hand():
    """T = 3, one video of 1 x 2 pixels: step 0 has both pixels in the world, step 1 one robot pixel."""
    from tests.movement_refs import movement_ref
    x = torch.zeros(3, 1, 3, 1, 2)
    x[1, 0, :, 0, 0] = 0.5                      # step 0: 3 values differ by 0.5          -> 0.75 / (6 + 1)
    x[2, 0, :, 0, 0] = 0.5
    x[2, 0, :, 0, 1] = torch.tensor([1.0, 2.0, 3.0])   # step 1: that pixel is robot; pixel 0 unchanged -> 0 / (3 + 1)
    m = torch.zeros(3, 1, 1, 1, 2)
    m[2, 0, 0, 0, 1] = 0.5
    score, step = movement_ref(x, m, torch.float64)
    assert step.shape == (2, 1) and score.shape == (1,)
    assert float(step[0, 0]) == 0.75 / 7 and float(step[1, 0]) == 0.0 and float(score[0]) == 0.75 / 7
    m[2] = 0
    assert float(movement_ref(x, m, torch.float64)[1][1, 0]) == 14.0 / 7


def test_fixture_separates_moving_from_static(tmp_path):
    """What test_gpu_movement.py relies on, seen without a GPU: through the dataset's own image path the fp64 scores of
    the two halves of the fixture lie more than 10 x apart."""
    from robot_aware_control_amd.data import RoboNetDataset
    from tests.movement_refs import movement_ref, write_movement_fixture
    truth = write_movement_fixture(str(tmp_path))
    assert len(truth) == 12 and sum(truth.values()) == 6
    files = sorted(truth)
    ds = RoboNetDataset(files, ["x_y"] * len(files), cfg(tmp_path))
    items = [ds[i] for i in range(len(files))]
    assert tuple(items[0]["images"].shape) == (8, 3, 16, 16) and [it["file_path"] for it in items] == files
    images = torch.stack([it["images"] for it in items], 1)
    masks = torch.stack([it["masks"] for it in items], 1)
    score = movement_ref(images, masks, torch.float64)[0]
    moving = torch.tensor([truth[f] for f in files])
    assert float(score[moving].min()) >= 10 * float(score[~moving].max()) > 0
