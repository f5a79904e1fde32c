"""CPU tests of the end-effector heatmap producer (`--model_use_heatmap`): the fp64 restatement of the contract
(tests/heatmap_refs.py) against the golden vectors of the reference's own `create_heatmaps`
(tools/gen_golden_heatmaps.py), the ABI entry's declarations, the camera table, the flag, and the dataset item."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import heatmap_refs as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64


def cfg(root, **kw):
    return hr.data_config(root, **kw)


@pytest.fixture(scope="module")
def golden():
    return hr.load_golden()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_robonet as mk
    root = str(tmp_path_factory.mktemp("robonet_heat"))
    assert mk.write(root, per_view=2, length=10, seed=5) == 8
    return root


@pytest.mark.parametrize("robot", list(hr.ROBOTS))
def test_restatement_reproduces_the_reference(golden, robot):
    g = golden
    states, ref = g[f"{robot}_states"], g[f"{robot}_centres"]
    heat, cen = hr.heatmaps(states, g[f"{robot}_low"], g[f"{robot}_high"], robot, g[f"{robot}_K"], g[f"{robot}_wTc"], H, W)
    assert len(states) == 64 and 8 <= ref[:, 2].sum() <= 56
    assert np.array_equal(cen[:, 2], ref[:, 2])
    # the reference holds its integers as uint8: equal to ours for every drawn frame, and ours modulo 256 for the others
    # (all recorded coordinates lie inside (-100, 200), where that cast wraps and nothing else)
    assert np.array_equal(cen[:, :2] & 0xFF, ref[:, :2])
    drawn = ref[:, 2] == 1
    assert np.array_equal(cen[drawn, :2], ref[drawn, :2])
    assert np.array_equal(cen[:, :2], np.trunc(g[f"{robot}_precast"]).astype(np.int64))
    full = g[f"{robot}_full_idx"]
    assert len(full) == 4 and g[f"{robot}_heatmaps"].dtype == np.float32
    assert np.abs(heat[full] - g[f"{robot}_heatmaps"]).max() <= 1e-7
    assert abs(float(g[f"{robot}_heatmaps"].max()) - 0.63662) < 1e-5  # the peak: the reference's clip(0, 1) never acts


def test_golden_set_holds_the_edge_cases(golden):
    cen = np.concatenate([golden[f"{r}_centres"] for r in hr.ROBOTS])
    pre = np.concatenate([golden[f"{r}_precast"] for r in hr.ROBOTS])
    drawn = cen[:, 2] == 1
    for corner in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        assert (drawn & (cen[:, 0] == corner[0]) & (cen[:, 1] == corner[1])).any(), corner
    assert (drawn & (pre[:, 0] > -1) & (pre[:, 0] < 0)).any() and (drawn & (pre[:, 1] > -1) & (pre[:, 1] < 0)).any()
    assert (~drawn & (cen[:, 0] == W) & (pre[:, 1] > 0) & (pre[:, 1] < H)).any()
    assert (~drawn & (cen[:, 1] == H) & (pre[:, 0] > 0) & (pre[:, 0] < W)).any()
    frac = np.abs(pre - np.trunc(pre))
    assert (pre > -100).all() and (pre < 200).all() and (frac >= 0.001).all() and (frac <= 0.999).all()


def test_abi_declares_the_entry():
    from robot_aware_control_amd import EXPORTS, _lib
    from robot_aware_control_amd import heatmaps as hm
    hdr = open(os.path.join(ROOT, "include", "rac_hip.h")).read()
    assert "int rac_eef_heatmaps(" in hdr and "int rac_heatmap_view_bytes(void);" in hdr and "#define RAC_ABI_VERSION 12" in hdr
    assert "rac_eef_heatmaps" in EXPORTS and "rac_heatmap_view_bytes" in EXPORTS
    assert len(_lib._SIGS["rac_eef_heatmaps"]) == 16
    lib = _lib.load()
    assert ctypes.sizeof(_lib.HeatmapView) == lib.rac_heatmap_view_bytes() == hm.VIEW.itemsize == 120
    for name in ("proj", "scale_x", "scale_y", "z_offset"):
        assert getattr(_lib.HeatmapView, name).offset == hm.VIEW.fields[name][1], name
    # refused calls come back as a status and a message, without a launch
    assert lib.rac_eef_heatmaps(None, 0, 0, None, None, 0, None, None, 0, 0, None, 1, 1, 48, 64, None) != 0
    assert b"rac_eef_heatmaps" in lib.rac_last_error()


def test_flag_parses():
    from robot_aware_control_amd import config
    cf, _ = config.argparser(["--model_use_heatmap", "True", "--camera_calibration", "/some/cameras.npz"])
    assert cf.model_use_heatmap is True and cf.camera_calibration == "/some/cameras.npz"
    assert config.argparser([])[0].camera_calibration is None


def test_camera_table_round_trip_and_views(golden, tmp_path, monkeypatch):
    from robot_aware_control_amd import heatmaps as hm
    table = hr.golden_table(golden)
    path = str(tmp_path / "cameras.npz")
    table.save(path)
    back = hm.CameraTable.load(path)
    assert set(back.world_to_camera) == set(table.world_to_camera) == {"sawyer_sudri0_c0", "baxter_left_c0",
                                                                       "widowx_widowx1_c0", "locobot_c0"}
    assert set(back.intrinsics) == {"logitech_c420", "intel_realsense_d435"}
    for k, v in table.world_to_camera.items():
        assert back.world_to_camera[k].dtype == np.float64 and np.array_equal(back.world_to_camera[k], v)
    for k, v in table.intrinsics.items():
        assert np.array_equal(back.intrinsics[k], v)
    assert np.array_equal(hm.CameraTable.from_config(argparse.Namespace(camera_calibration=path)).intrinsics["logitech_c420"],
                          table.intrinsics["logitech_c420"])
    # the view record: the reference's fp64 product, the scale factors, the fp32 offset
    row = back.view_row("sawyer", "sudri0_c0", 48, 64)
    assert row.shape == (hm.VIEW_ROW,) and row.dtype == np.float64
    assert np.array_equal(row[:12].reshape(3, 4), golden["sawyer_K"] @ golden["sawyer_wTc"][:3])
    assert row[12] == 64 / 320 and row[13] == 48 / 240 and row[14] == float(np.float32(-0.15)) and tuple(row[15:]) == (48, 64)
    loco = back.view_row("locobot", "c1", 64, 64)  # always locobot_c0, the 640 x 480 camera
    assert np.array_equal(loco[:12].reshape(3, 4), golden["locobot_K"] @ golden["locobot_wTc"][:3])
    assert loco[12] == 64 / 640 and loco[13] == 64 / 480 and loco[14] == 0.0
    assert back.view_row("widowx", "widowx1_c0", 48, 64)[14] == float(np.float32(0.05))
    views = hm.pack_views(np.stack([row, loco]))
    assert views.dtype.itemsize == 120 and views["z_offset"].dtype == np.float32 and views["z_offset"][0] == np.float32(-0.15)
    assert np.array_equal(views["proj"][1], loco[:12]) and views["scale_y"][1] == 64 / 480
    # unknown robots and viewpoints
    with pytest.raises(ValueError, match="franka"):
        back.view_row("franka", "c0", 48, 64)
    with pytest.raises(ValueError):
        hm.create_heatmaps(torch.zeros(2, 5), np.zeros(5, np.float32), np.ones(5, np.float32), "franka", "c0")
    with pytest.raises(KeyError, match="sawyer_nowhere"):
        back.view_row("sawyer", "nowhere", 48, 64)
    # neither source: the message names both
    def no_reference():
        raise ImportError("No module named 'src.utils.camera_calibration'")
    monkeypatch.setattr(hm.CameraTable, "from_reference", staticmethod(no_reference))
    with pytest.raises(ImportError, match=r"--camera_calibration FILE.*src/utils/camera_calibration\.py"):
        hm.CameraTable.from_config(argparse.Namespace(camera_calibration=None))


def test_create_heatmaps_is_reexported_and_has_no_cpu_fallback(golden):
    from robot_aware_control_amd import RacError
    from robot_aware_control_amd import heatmaps as hm
    from src.dataset.robonet.robonet_dataset import create_heatmaps
    assert create_heatmaps is hm.create_heatmaps
    with pytest.raises(RacError):
        hm.heatmaps_from_views(torch.zeros(2, 1, 5), np.zeros((1, 5)), np.ones((1, 5)), np.zeros((1, hm.VIEW_ROW)), 48, 64)
    if not torch.cuda.is_available():
        with pytest.raises(RacError):
            create_heatmaps(torch.zeros(2, 5), np.zeros(5, np.float32), np.ones(5, np.float32), "sawyer", "sudri0_c0")


def test_dataset_item_under_the_flag(tree, golden, tmp_path, monkeypatch):
    from robot_aware_control_amd import RacError
    from robot_aware_control_amd import data as D
    from robot_aware_control_amd import heatmaps as hm
    path = str(tmp_path / "cameras.npz")
    hr.synthetic_root_table(golden).save(path)
    off = cfg(tree)
    Xtr, Xte, ytr, yte = D.split_files(off)
    plain = D.RoboNetDataset(Xtr, ytr, off)[0]
    assert set(plain) == {"images", "states", "actions", "masks", "robot", "folder", "file_path", "idx", "qpos"}
    on = cfg(tree, model_use_heatmap=True, camera_calibration=path)
    ds = D.RoboNetDataset(Xtr, ytr, on)
    table = hm.CameraTable.load(path)
    for i in range(len(ds)):
        it = ds[i]
        assert set(it) == set(plain) | {"low", "high", "heatmap_view"}
        z = np.load(it["file_path"])
        assert np.array_equal(it["low"], z["low_bound"]) and np.array_equal(it["high"], z["high_bound"])
        assert np.array_equal(it["heatmap_view"], table.view_row(it["robot"], it["folder"], 48, 64))
    it = D.RoboNetDataset(Xtr, ytr, cfg(tree))[0]  # the same window with the flag off: the same numbers
    on_it = D.RoboNetDataset(Xtr, ytr, on)[0]
    for k in plain:
        same = torch.equal(torch.as_tensor(it[k]), torch.as_tensor(on_it[k])) if k not in ("robot", "folder", "file_path", "idx") \
            else it[k] == on_it[k]
        assert same, k
    # the camera strategies normalise the states in the camera frame: refused, with the reason
    eyes = {v: np.eye(4) for v in set(ytr)}
    monkeypatch.setattr(D, "_camera_dicts", lambda: (eyes, eyes))
    cam = D.RoboNetDataset(Xtr, ytr, cfg(tree, model_use_heatmap=True, camera_calibration=path, preprocess_action="camera_raw"))
    with pytest.raises(NotImplementedError, match="world frame"):
        cam[0]
    assert "heatmap_view" not in D.RoboNetDataset(Xtr, ytr, cfg(tree, preprocess_action="camera_raw"))[0]
    # a batch: collated as numbers; making the heatmaps needs the GPU (no CPU fallback)
    batch = D.collate([ds[0], ds[1]])
    assert batch["heatmap_view"].shape == (2, hm.VIEW_ROW) and batch["heatmap_view"].dtype == torch.float64
    assert batch["low"].shape == (2, 5)
    with pytest.raises(RacError):
        D.process_batch(batch, torch.device("cpu"))
    out = D.process_batch(D.collate([D.RoboNetDataset(Xtr, ytr, off)[0]]), torch.device("cpu"))
    assert "heatmaps" not in out and "heatmap_view" not in out and "low" not in out


def test_learned_robot_model_without_heatmaps_in_the_batch_still_raises():
    from robot_aware_control_amd.robot_model import GripperStatePredictor, JointPosPredictor, LearnedRobotModel
    cf = argparse.Namespace(robot_joint_dim=7, robot_dim=5, action_dim=5, image_height=48, image_width=64,
                            experiment="finetune_widowx", preprocess_action="raw", model_use_heatmap=True)
    model = LearnedRobotModel(cf, JointPosPredictor(cf), GripperStatePredictor(cf), renderers={})
    batch = {"states": torch.zeros(3, 2, 5), "qpos": torch.zeros(3, 2, 7), "actions": torch.zeros(2, 2, 5),
             "masks": torch.zeros(3, 2, 1, 48, 64), "folder": ["a", "b"], "robot": ["widowx"] * 2}
    with pytest.raises(NotImplementedError, match="heatmap"):
        model.predict_batch(batch)
