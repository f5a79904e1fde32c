"""GPU tests of `rac_eef_heatmaps` and of everything that makes heatmaps with it (`--model_use_heatmap`): the kernel
against the golden vectors of the reference's own `create_heatmaps` and against the fp64 restatement of the contract
(tests/heatmap_refs.py), the data path, one train step fed by it, and the two robot models.

Bound on a heatmap value: 2e-7 absolute.  The squared distance is an exact integer in fp32; after the division by 50 and
`expf` the error is at most about 0.6366 e^-a (a + 2) ulp, <= 8e-8 at the peak, so 2e-7 is three fp32 ulp of the largest
value; a centre off by one pixel costs 1.3e-2.  Integers and validity must be equal."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import svg_oracle as orc  # noqa: E402
from tests import heatmap_refs as hr  # noqa: E402
from tests import robot_model_oracle as rmo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return hr.load_golden()


@pytest.fixture(scope="module")
def table(golden):
    return hr.synthetic_root_table(golden)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_robonet as mk
    root = str(tmp_path_factory.mktemp("robonet_heat_gpu"))
    assert mk.write(root, per_view=2, length=10, seed=5) == 8
    return root


def launch(dev, table, states, low, high, robots, H, W, time_first=True, **kw):
    """(heatmaps, centres) of one launch; `states` a host array, (T, B, S) or (B, T, S)."""
    from robot_aware_control_amd import heatmaps as hm
    rows = table.view_rows(robots, [hr.ROBOTS[r][3] for r in robots], H, W)
    return hm.heatmaps_from_views(torch.as_tensor(states).to(dev), np.stack(low), np.stack(high), rows, H, W,
                                  time_first=time_first, centres=True, **kw)


def restated(golden, states, low, high, robots, H, W):
    return hr.batch(np.asarray(states), low, high, robots, [golden[f"{r}_K"] for r in robots],
                    [golden[f"{r}_wTc"] for r in robots], H, W)


def mixed_batch(golden, T, B, seed, S=5):
    """Seeded states (T, B, S) of B videos of different robots with the golden bounds: golden states (two thirds of them
    inside the image) moved by up to 0.01 of the box, so that a batch mixes valid and invalid frames."""
    robots = [list(hr.ROBOTS)[(b + seed) % 4] for b in range(B)]
    g = np.random.Generator(np.random.Philox(key=[seed, 51]))
    states = np.stack([golden[f"{r}_states"][g.integers(0, 64, T)] for r in robots], 1)[..., :S]
    states = (states + g.uniform(-0.01, 0.01, states.shape)).astype(np.float32)
    return states, [golden[f"{r}_low"] for r in robots], [golden[f"{r}_high"] for r in robots], robots


def check(got, cen, want, want_cen, what=""):
    assert got.dtype == torch.float32 and cen.dtype == torch.int32
    assert np.array_equal(cen.cpu().numpy(), want_cen), what
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max() if want.size else 0.0
    print(f"{what}: max |kernel - fp64| = {err:.3g}, {int(want_cen[..., 2].sum())} of {want_cen[..., 2].size} frames valid")
    assert err <= TOL, (what, err)


@pytest.mark.parametrize("robot", list(hr.ROBOTS))
def test_kernel_vs_reference_golden(dev, golden, table, robot):
    g = golden
    states, ref = g[f"{robot}_states"], g[f"{robot}_centres"]
    full = {int(i): k for k, i in enumerate(g[f"{robot}_full_idx"])}
    worst, compared = 0.0, 0
    for lo in range(0, len(states), 24):  # 64 states as launches of up to 6 x 4 frames
        part = states[lo:lo + 24]
        B = 4
        T = len(part) // B
        st = part.reshape(T, B, -1)
        heat, cen = launch(dev, table, st, [g[f"{robot}_low"]] * B, [g[f"{robot}_high"]] * B, [robot] * B, 48, 64)
        cen, heat = cen.cpu().numpy().reshape(T * B, 3), heat.cpu().numpy().reshape(T * B, 48, 64)
        want = ref[lo:lo + T * B]
        assert np.array_equal(cen[:, 2], want[:, 2])
        assert np.array_equal(cen[:, :2] & 0xFF, want[:, :2])  # (the reference keeps uint8; drawn frames: equal as they are)
        assert np.array_equal(cen[want[:, 2] == 1, :2], want[want[:, 2] == 1, :2])
        for j in range(T * B):
            if want[j, 2] == 0:
                assert not heat[j].any()
            if lo + j in full:
                worst = max(worst, np.abs(heat[j].astype(np.float64) - g[f"{robot}_heatmaps"][full[lo + j], 0]).max())
                compared += 1
    print(f"{robot}: max |kernel - reference| = {worst:.3g} over {compared} heatmaps")
    assert compared == 4 and worst <= TOL


@pytest.mark.parametrize("time_first", [True, False])
@pytest.mark.parametrize("H,W", [(48, 64), (64, 64), (10, 12), (7, 9)])
def test_kernel_vs_restatement(dev, golden, table, H, W, time_first):
    """(10, 12) and (7, 9): no multiple of anything; (7, 9) takes the scalar stores (W % 4 != 0)."""
    states, low, high, robots = mixed_batch(golden, 5, 3, seed=H + W)
    want, want_cen = restated(golden, states, low, high, robots, H, W)
    given = states if time_first else np.ascontiguousarray(states.transpose(1, 0, 2))
    heat, cen = launch(dev, table, given, low, high, robots, H, W, time_first=time_first)
    assert heat.shape == (5, 3, 1, H, W)
    check(heat, cen, want, want_cen, f"{H}x{W} time_first={time_first}")


def test_rows_of_a_larger_tensor_and_single_frames(dev, golden, table):
    states, low, high, robots = mixed_batch(golden, 4, 3, seed=7)
    want, want_cen = restated(golden, states, low, high, robots, 48, 64)
    out = torch.full((5, 3, 1, 48, 64), 7.0, device=dev)
    heat, cen = launch(dev, table, states, low, high, robots, 48, 64, out=out, first_row=1)
    assert heat is out and bool((out[0] == 7.0).all())
    check(out[1:], cen, want, want_cen, "rows 1..T")
    fresh, _ = launch(dev, table, states, low, high, robots, 48, 64)
    assert torch.equal(fresh, out[1:])
    # an unaligned view of a larger buffer: the scalar stores give the same values
    buf = torch.zeros(4 * 3 * 48 * 64 + 1, device=dev)
    odd, _ = launch(dev, table, states, low, high, robots, 48, 64, out=buf[1:].view(4, 3, 1, 48, 64))
    assert torch.equal(odd, fresh)
    # T = 1 and B = 1; a frame's bits alone and inside the batch
    picks = [tuple(np.argwhere(want_cen[..., 2] == v)[0]) for v in (1, 0)] + [(3, 2)]
    for t, b in picks:
        one, one_cen = launch(dev, table, states[t:t + 1, b:b + 1], low[b:b + 1], high[b:b + 1], robots[b:b + 1], 48, 64)
        assert one.shape == (1, 1, 1, 48, 64) and torch.equal(one[0, 0], fresh[t, b]) and torch.equal(one_cen[0, 0], cen[t, b])
    # two runs
    again, again_cen = launch(dev, table, states, low, high, robots, 48, 64)
    assert torch.equal(again, fresh) and torch.equal(again_cen, cen)
    # S = 3 states
    three, _ = launch(dev, table, np.ascontiguousarray(states[..., :3]), low, high, robots, 48, 64)
    assert torch.equal(three, fresh)


def test_invalid_and_non_finite_frames_are_zero(dev, golden, table):
    states, low, high, robots = mixed_batch(golden, 3, 4, seed=11)
    far = states + 40.0  # every frame far outside its image
    want, want_cen = restated(golden, far, low, high, robots, 48, 64)
    assert want_cen[..., 2].sum() == 0
    heat, cen = launch(dev, table, far, low, high, robots, 48, 64)
    check(heat, cen, want, want_cen, "all invalid")
    assert not bool(heat.any())
    bad = states.copy()
    bad[0, 0, 0], bad[1, 1, 2], bad[2, 2, 1], bad[2, 3, :3] = np.nan, np.inf, -np.inf, np.nan
    want, want_cen = restated(golden, bad, low, high, robots, 48, 64)
    heat, cen = launch(dev, table, bad, low, high, robots, 48, 64)
    torch.cuda.synchronize()
    check(heat, cen, want, want_cen, "non-finite")
    for t, b in ((0, 0), (1, 1), (2, 2), (2, 3)):
        assert not bool(heat[t, b].any()) and int(cen[t, b, 2]) == 0, (t, b)
    assert cen[0, 0].tolist() == [0, 0, 0] and cen[2, 3].tolist() == [0, 0, 0]
    assert want_cen[..., 2].sum() > 0  # (the other frames of that batch are untouched by their neighbours)


@pytest.mark.parametrize("robot", list(hr.ROBOTS))
def test_create_heatmaps_vs_reference_golden(dev, golden, robot):
    from robot_aware_control_amd import heatmaps as hm
    g = golden
    hm.use_camera_table(hr.golden_table(g))
    try:
        idx = g[f"{robot}_full_idx"]
        got = hm.create_heatmaps(torch.from_numpy(g[f"{robot}_states"][idx]), g[f"{robot}_low"], g[f"{robot}_high"], robot,
                                 hr.ROBOTS[robot][3])
    finally:
        hm.use_camera_table(None)
    assert isinstance(got, np.ndarray) and got.shape == (4, 1, 48, 64) and got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - g[f"{robot}_heatmaps"]).max() <= TOL


def loader_batches(tree, golden, tmp_path, **kw):
    from robot_aware_control_amd import data as D
    path = str(tmp_path / "cameras.npz")
    hr.synthetic_root_table(golden).save(path)
    cf = hr.data_config(tree, model_use_heatmap=True, camera_calibration=path, batch_size=2, **kw)
    Xtr, _, ytr, _ = D.split_files(cf)
    ds = D.RoboNetDataset(Xtr, ytr, cf)
    return cf, [D.collate([ds[i], ds[i + 1]]) for i in (0, 2)]


def test_process_batch_and_prefetcher_add_heatmaps(dev, tree, golden, table, tmp_path):
    from robot_aware_control_amd import data as D
    from robot_aware_control_amd import heatmaps as hm
    cf, raws = loader_batches(tree, golden, tmp_path)
    pf = D.DevicePrefetcher([{k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()} for raw in raws], dev)
    try:
        for raw in raws:
            got = next(pf)
            out = D.process_batch(raw, dev)
            assert "heatmap_view" not in out and out["heatmaps"].shape == (8, 2, 1, 48, 64)
            want = hm.batch_heatmaps(out["states"], out["low"], out["high"], out["robot"], out["folder"], table, 48, 64)
            assert torch.equal(out["heatmaps"], want) and torch.equal(got["heatmaps"], want)
            assert torch.equal(got["states"], out["states"]) and "heatmap_view" not in got
            ref, _ = hr.batch(out["states"].cpu().numpy(), out["low"].numpy(), out["high"].numpy(), out["robot"],
                              [table.intrinsics[hm.ROBOTS[r][1]] for r in out["robot"]],
                              [table.world_to_camera[hm.view_key(r, f)] for r, f in zip(out["robot"], out["folder"])])
            assert np.abs(want.cpu().numpy() - ref).max() <= TOL
    finally:
        pf.close()


def test_train_step_from_the_loader_equals_hand_fed_heatmaps(dev, tree, golden, table, tmp_path):
    from robot_aware_control_amd import data as D
    from robot_aware_control_amd import heatmaps as hm
    from robot_aware_control_amd.trainer import PredictionTrainer
    _, raws = loader_batches(tree, golden, tmp_path)
    batch = D.process_batch(raws[0], dev)
    cfg = orc.Cfg(g_dim=64, z_dim=16, batch_size=2, n_past=1, n_future=2, lr=1e-4, image_height=48, image_width=64,
                  action_dim=4, robot_dim=5, model_use_robot_state=True, model_use_heatmap=True)
    d = dict(cfg.__dict__)
    d.update(device=dev, experiment="train_robonet", load_movement_info=False, movement_weight=1.0,
             scheduled_sampling=False, scheduled_sampling_k=4000, model="svg", optimizer="adam", seed=0, wandb=False,
             log_dir=str(tmp_path / "log"), dynamics_model_ckpt=None, ddp_bucket_mb=64)
    sd = orc.make_weights(cfg, seed=1, randomize_bn_stats=False)

    def step(heatmaps):
        tr = PredictionTrainer(argparse.Namespace(**d))
        tr.model.load_state_dict({k: v.clone() for k, v in sd.items()})
        tr.model.train()
        gen = torch.Generator().manual_seed(5)
        tr.model.eps_source = lambda shape: torch.randn(shape, generator=gen)
        window = {k: (v[:3] if torch.is_tensor(v) and k not in ("low", "high") else v) for k, v in batch.items()}
        window["actions"], window["heatmaps"] = batch["actions"][:2], heatmaps[:3]
        return tr._train_step(window)
    by_hand = hm.batch_heatmaps(batch["states"], batch["low"], batch["high"], batch["robot"], batch["folder"], table, 48, 64)
    a, b = step(batch["heatmaps"]), step(by_hand.clone())
    assert a.keys() == b.keys() and all(np.isfinite(v) for v in a.values())
    assert all(a[k] == b[k] for k in a), (a, b)
    c = step(torch.zeros_like(by_hand))  # (the heatmaps do reach the loss)
    assert any(a[k] != c[k] for k in a)


def robot_batch(golden, T, robots, seed):
    """A window whose start states are golden states the reference drew, so that the rollouts stay near the image."""
    B = len(robots)
    data = rmo.synth_window(seed, T + 1, B, 7, 5, 5)
    for b, r in enumerate(robots):
        data["states"][:, b] = torch.from_numpy(golden[f"{r}_states"][int(golden[f"{r}_full_idx"][b % 4])])
    g = np.random.Generator(np.random.Philox(key=[seed, 52]))
    data.update(robot=list(robots), folder=[hr.ROBOTS[r][3] for r in robots],
                low=torch.from_numpy(np.stack([golden[f"{r}_low"] for r in robots])),
                high=torch.from_numpy(np.stack([golden[f"{r}_high"] for r in robots])),
                masks=torch.zeros(T + 1, B, 1, 48, 64), heatmaps=torch.from_numpy(g.random((T + 1, B, 1, 48, 64), dtype=np.float32)))
    return data


def check_triple(golden, data, out, T, what):
    states, masks, heat = out
    robots = data["robot"]
    assert heat.shape == data["heatmaps"].shape and heat.dtype == torch.float32 and heat.is_cuda
    assert torch.equal(heat[0].cpu(), data["heatmaps"][0])
    want, cen = restated(golden, states[1:T + 1].cpu().numpy(), data["low"].numpy(), data["high"].numpy(), robots, 48, 64)
    err = np.abs(heat[1:].cpu().numpy() - want).max()
    print(f"{what}: max |heatmaps - fp64| = {err:.3g}, {int(cen[..., 2].sum())} of {cen[..., 2].size} rebuilt frames valid")
    assert err <= TOL
    return states, masks


def test_learned_robot_model_returns_the_triple(dev, golden, table):
    from robot_aware_control_amd.robot_model import GripperStatePredictor, JointPosPredictor, LearnedRobotModel
    T, robots = 3, ["sawyer", "widowx", "baxter"]
    cf = argparse.Namespace(robot_joint_dim=7, robot_dim=5, action_dim=5, image_height=48, image_width=64,
                            experiment="finetune_widowx", preprocess_action="raw", model_use_heatmap=True)
    joint, gripper = JointPosPredictor(cf).to(dev), GripperStatePredictor(cf).to(dev)
    joint.load_state_dict(rmo.make_weights("joint", 7, 5, 31))
    gripper.load_state_dict({k: v * 0.25 for k, v in rmo.make_weights("gripper", 5, 5, 31).items()})
    renderers = {hr.ROBOTS[r][3]: rmo.RectRenderer(i) for i, r in enumerate(robots)}
    model = LearnedRobotModel(cf, joint, gripper, renderers=renderers, camera_table=table)
    data = robot_batch(golden, T, robots, seed=17)
    states, masks = check_triple(golden, data, model.predict_batch(data), T, "learned robot model")
    cf.model_use_heatmap = False
    plain = model.predict_batch(data)
    assert len(plain) == 2 and torch.equal(plain[0], states) and torch.equal(plain[1], masks)


def test_atlas_robot_model_returns_the_triple(dev, golden, table):
    from robot_aware_control_amd.robot_atlas import AtlasRobotModel
    T, robots = 3, ["locobot", "locobot"]
    data = robot_batch(golden, T, robots, seed=19)
    lo, hi = golden["locobot_low"], golden["locobot_high"]
    height = float(data["states"][0, 0, 2] * (hi[2] - lo[2]) + lo[2])  # the start state's own world height
    data["actions"] = data["actions"] * 0.1
    cf = argparse.Namespace(model_use_heatmap=True, camera_calibration=None)
    atlas = torch.zeros((1, 1, 48, 64), dtype=torch.uint8)
    model = AtlasRobotModel(atlas, 0.0, 0.0, 1.0, 1.0, height, device=dev, config=cf, camera_table=table)
    states, masks = check_triple(golden, data, model.predict_batch(data), T, "atlas robot model")
    pair = AtlasRobotModel(atlas, 0.0, 0.0, 1.0, 1.0, height, device=dev).predict_batch(data)  # no config: the pair
    assert len(pair) == 2 and torch.equal(pair[0], states) and torch.equal(pair[1], masks)
    no_heat = {k: v for k, v in data.items() if k != "heatmaps"}
    assert len(model.predict_batch(no_heat)) == 2


def test_command_line_trains_from_a_data_root_with_heatmaps(dev, tree, golden, tmp_path, monkeypatch):
    """`python -m src.prediction.multirobot_trainer --data_root <root> --model_use_heatmap True --camera_calibration
    <npz>`: one epoch of two steps through loader, prefetcher, `rac_eef_heatmaps` and the train step; a checkpoint whose
    encoder takes the heatmap plane is written."""
    from src.prediction import multirobot_trainer as cli
    cameras = str(tmp_path / "cameras.npz")
    hr.synthetic_root_table(golden).save(cameras)
    argv = (f"prog --jobname h --wandb False --data_root {tree} --camera_calibration {cameras} --model_use_heatmap True "
            "--batch_size 2 --test_batch_size 2 --n_future 2 --n_past 1 --n_eval 3 --g_dim 32 --z_dim 8 --model svg "
            "--niter 1 --epoch_size 2 --checkpoint_interval 1 --eval_interval 10 --reconstruction_loss l1 "
            "--last_frame_skip True --action_dim 4 --robot_dim 5 --impute_autograsp_action False --data_threads 0 "
            "--lr 0.0001 --experiment train_robonet --model_use_robot_state True --random_snippet True --video_length 8 "
            f"--log_dir {tmp_path}").split()
    monkeypatch.setattr(sys, "argv", argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main()
    ckpts = [f for f in os.listdir(os.path.join(tmp_path, "h")) if f.startswith("ckpt_") and f.endswith(".pt")]
    assert ckpts, os.listdir(os.path.join(tmp_path, "h"))
    ck = torch.load(os.path.join(tmp_path, "h", ckpts[0]), map_location="cpu")
    assert ck["step"] > 0
    first = [v for k, v in ck["model"].items() if v.dim() == 4 and k.startswith("encoder")][0]
    assert first.shape[1] == 3 + 1  # rgb + the heatmap plane
