"""CPU: the learned robot model's host side -- the oracle restatement against the reference's own numbers, the modules'
state_dict / flat-buffer layout, checkpoints in both directions against plain torch, initialisation, error messages."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import robot_model_oracle as rmo
from tests.fp64_tools import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = rmo.GOLDEN
J, R, A, B = C["J"], C["R"], C["A"], C["B"]
N_PAST, N_FUTURE, N_EVAL = C["n_past"], C["n_future"], C["n_eval"]
SEED, LR, BETA1 = C["seed"], C["lr"], C["beta1"]


def _cf(**kw):
    d = dict(image_height=64, robot_joint_dim=J, robot_dim=R, action_dim=A, n_past=N_PAST, n_future=N_FUTURE, n_eval=N_EVAL,
             experiment="finetune_widowx", preprocess_action="raw", model_use_heatmap=False, image_width=64,
             optimizer="adam", lr=LR, beta1=BETA1, log_dir="/nonexistent")
    d.update(kw)
    return argparse.Namespace(**d)


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "robot_model.npz"))


def test_oracle_reproduces_the_reference():
    """The restatement IS the reference: every recorded number of the reference's own classes and trainer methods comes
    back from the fp32 oracle.  Both are fp32 evaluations of one formula and may differ by the order of their sums only:
    each is within e32 = |oracle32 - oracle64| of the exact value, so they are within 2 e32 of each other (floor 1e-7)."""
    g = _golden()
    assert str(g["source"]) in ("reference", "oracle")
    o32, o64 = rmo.golden_recipe(g, torch.float32), rmo.golden_recipe(g, torch.float64)
    checked = 0
    for key in g.files:
        if key.startswith("in_") or key == "source":
            continue
        gold = torch.from_numpy(np.asarray(g[key], dtype=np.float64))
        e32 = relerr(o32[key], o64[key])
        err = relerr(o32[key], gold)
        print(f"{key}: |oracle32 - golden| {err:.2e}  e32 {e32:.2e}")
        assert err <= max(1e-7, 2 * e32), (key, err, e32)
        checked += 1
    assert checked >= 20


def test_state_dict_and_flat_layout():
    from robot_aware_control_amd.robot_model import GripperStatePredictor, JointPosPredictor, RobotModels, param_count
    for D_j, D_r, A_ in ((7, 5, 5), (5, 6, 2), (6, 7, 4)):
        cf = _cf(robot_joint_dim=D_j, robot_dim=D_r, action_dim=A_)
        joint, gripper = JointPosPredictor(cf), GripperStatePredictor(cf)
        for m, D in ((joint, D_j), (gripper, D_r)):
            sd = m.state_dict()
            assert tuple(sd) == rmo.KEYS
            for k, shape in rmo.shapes(D, A_).items():
                assert tuple(sd[k].shape) == shape, k
            # one contiguous block in state_dict order, torch's [out][in] layout; all but b4 start at multiples of 512
            flat, grad = m.flat_parameters()
            assert flat.numel() == param_count(D, A_) == sum(v.numel() for v in sd.values())
            off = 0
            for k, p in m.named_parameters():
                assert p.is_contiguous() and p.data_ptr() == flat.data_ptr() + 4 * off, k
                assert p.grad.data_ptr() == grad.data_ptr() + 4 * off, k
                assert off % 512 == 0 or k == "predictor.6.bias"
                assert torch.equal(flat[off:off + p.numel()].view(p.shape), p.detach())
                off += p.numel()
        models = RobotModels(joint, gripper)
        flat, grad = models.flat_parameters()
        assert [id(p) for p in models.parameters()] == [id(p) for p in list(joint.parameters()) + list(gripper.parameters())]
        assert joint.flat_parameters()[0].data_ptr() == flat.data_ptr()
        goff = (param_count(D_j, A_) + 3) // 4 * 4
        assert gripper.flat_parameters()[0].data_ptr() == flat.data_ptr() + 4 * goff
        assert all(p._rac_off == (p.data_ptr() - flat.data_ptr()) // 4 for p in models.parameters())
        # load_state_dict writes through the views
        ws = rmo.make_weights("gripper", D_r, A_, 3)
        gripper.load_state_dict(ws)
        assert torch.equal(flat[goff:goff + 512 * (D_r + A_)].view(512, D_r + A_), ws["predictor.0.weight"])
    with pytest.raises(ValueError):
        JointPosPredictor(_cf(robot_joint_dim=8))
    with pytest.raises(ValueError):
        GripperStatePredictor(_cf(action_dim=6))


def test_same_seed_same_initial_weights_as_torch():
    """The reference applies no init_weights to these models: torch's default nn.Linear initialisation, in its order."""
    from robot_aware_control_amd.robot_model import GripperStatePredictor, JointPosPredictor
    torch.manual_seed(123)
    ours = [JointPosPredictor(_cf()), GripperStatePredictor(_cf())]
    torch.manual_seed(123)
    theirs = [rmo.Predictor(J, A), rmo.Predictor(R, A)]
    for a, b in zip(ours, theirs):
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka


def test_checkpoint_round_trips_against_plain_torch(tmp_path):
    """RobotPredictionTrainer's checkpoint (joint_model, gripper_model, optimizer, step) loads into plain nn.Sequential
    models and a torch.optim.Adam, and what those write loads back."""
    from robot_aware_control_amd.optim import FusedAdam
    from robot_aware_control_amd.robot_model import GripperStatePredictor, JointPosPredictor, RobotModels
    from robot_aware_control_amd.robot_trainer import RobotPredictionTrainer
    cf = _cf(log_dir=str(tmp_path))
    joint, gripper = JointPosPredictor(cf), GripperStatePredictor(cf)
    joint.load_state_dict(rmo.make_weights("joint", J, A, 1))
    gripper.load_state_dict(rmo.make_weights("gripper", R, A, 1))
    models = RobotModels(joint, gripper)
    opt = FusedAdam(models, lr=LR, betas=(BETA1, 0.999))
    m, v = opt._moments()
    m.copy_(torch.arange(m.numel(), dtype=torch.float32) * 1e-6)
    v.fill_(0.25)
    opt._steps = 5
    ns = argparse.Namespace(_config=cf, _step=17, joint_model=joint, gripper_model=gripper, optimizer=opt,
                            _device=torch.device("cpu"))
    path = RobotPredictionTrainer._save_checkpoint(ns)
    ckpt = torch.load(path)
    assert set(ckpt) == {"joint_model", "gripper_model", "optimizer", "step"} and ckpt["step"] == 17
    # ... into the plain models and torch's Adam (the reference's side)
    pj, pg = rmo.Predictor(J, A), rmo.Predictor(R, A)
    pj.load_state_dict(ckpt["joint_model"])
    pg.load_state_dict(ckpt["gripper_model"])
    ref_opt = torch.optim.Adam(list(pj.parameters()) + list(pg.parameters()), lr=LR, betas=(BETA1, 0.999))
    ref_opt.load_state_dict(ckpt["optimizer"])
    st = ref_opt.state[pg.predictor[6].bias]
    assert float(st["step"]) == 5.0 and torch.equal(st["exp_avg_sq"], torch.full((R,), 0.25))
    off = pj.predictor[2].weight
    assert torch.equal(ref_opt.state[off]["exp_avg"].flatten()[:3], m[6656:6659])
    # ... and back: one real torch step, saved in the reference's format, loaded by this trainer's method
    for p in ref_opt.param_groups[0]["params"]:
        p.grad = torch.full_like(p, 0.5)
    ref_opt.step()
    back = os.path.join(str(tmp_path), "ref.pt")
    torch.save({"joint_model": pj.state_dict(), "gripper_model": pg.state_dict(), "optimizer": ref_opt.state_dict(),
                "step": 99}, back)
    ns2 = argparse.Namespace(_config=_cf(experiment="train_robot_model"), joint_model=joint, gripper_model=gripper,
                             optimizer=opt, _device=torch.device("cpu"))
    assert RobotPredictionTrainer._load_checkpoint(ns2, back) == 99
    assert opt._steps == 6
    assert torch.equal(joint.state_dict()["predictor.4.weight"], pj.state_dict()["predictor.4.weight"])
    assert torch.equal(opt.state_dict()["state"][15]["exp_avg_sq"],
                       ref_opt.state[pg.predictor[6].bias]["exp_avg_sq"])
    # a given path under the three finetune experiments restarts at step 0 and keeps the optimiser
    opt._steps = 0
    ns3 = argparse.Namespace(_config=_cf(experiment="finetune_widowx"), joint_model=joint, gripper_model=gripper,
                             optimizer=opt, _device=torch.device("cpu"))
    assert RobotPredictionTrainer._load_checkpoint(ns3, back) == 0 and opt._steps == 0
    # no path: the newest ckpt_*.pt of log_dir
    ns4 = argparse.Namespace(_config=cf, joint_model=joint, gripper_model=gripper, optimizer=opt,
                             _device=torch.device("cpu"))
    assert RobotPredictionTrainer._load_checkpoint(ns4, None) == 17 and opt._steps == 5


def test_reference_import_paths():
    from src.prediction.joint_pos_trainer import RobotPredictionTrainer
    from src.prediction.models.dynamics import GripperStatePredictor, JointPosPredictor
    from robot_aware_control_amd import robot_model, robot_trainer
    assert RobotPredictionTrainer is robot_trainer.RobotPredictionTrainer
    assert JointPosPredictor is robot_model.JointPosPredictor and GripperStatePredictor is robot_model.GripperStatePredictor
    for name in ("_train_video", "_train_step", "_eval_video", "_eval_step", "_compute_epoch_metrics", "train",
                 "_save_checkpoint", "_load_checkpoint"):
        assert callable(getattr(RobotPredictionTrainer, name))


def test_error_messages():
    from robot_aware_control_amd import RacError
    from robot_aware_control_amd.robot_model import GripperStatePredictor, JointPosPredictor, LearnedRobotModel
    from robot_aware_control_amd.trainer import PredictionTrainer
    # no checkpoint: the path the flags name is the one that is read
    from robot_aware_control_amd import config
    cf, _ = config.argparser(["--learned_robot_model", "True", "--robot_model_ckpt", "/nonexistent/robot.pt",
                              "--experiment", "finetune_widowx"])
    assert cf.learned_robot_model is True
    with pytest.raises(ValueError, match="/nonexistent/robot.pt"):
        PredictionTrainer._load_robot_model_checkpoint(argparse.Namespace(), cf.robot_model_ckpt)
    for path in (None, "/nonexistent/ckpt.pt"):
        with pytest.raises(ValueError, match="robot_model_ckpt"):
            PredictionTrainer._load_robot_model_checkpoint(argparse.Namespace(), path)
    joint, gripper = JointPosPredictor(_cf()), GripperStatePredictor(_cf())
    data = rmo.synth_window(1, 3, 2, J, R, A)
    data.update(masks=torch.zeros(3, 2, 1, 64, 64), folder=["cam0", "cam1"])
    # no renderer: the reference's MuJoCo envs are tried and are not here
    model = LearnedRobotModel(_cf(), joint, gripper, renderers={"cam0": rmo.RectRenderer(0)})
    with pytest.raises(NotImplementedError, match="cam1.*generate_masks.*full reference checkout"):
        model.predict_batch(data)
    # heatmaps
    with pytest.raises(NotImplementedError, match="heatmap"):
        LearnedRobotModel(_cf(model_use_heatmap=True), joint, gripper, renderers={}).predict_batch(data)
    # no CPU fallback
    with pytest.raises(RacError):
        joint(data["qpos"][0], data["actions"][0])
    both = {"cam0": rmo.RectRenderer(0), "cam1": rmo.RectRenderer(1)}
    with pytest.raises(RacError):
        LearnedRobotModel(_cf(), joint, gripper, renderers=both).predict_batch(data)


def test_resize_masks_is_the_video_trainers_transform():
    """trainer.py:87-88, 222-226: ToTensor, Resize((image_height, image_width)), bool -- bilinear without antialiasing."""
    from robot_aware_control_amd.robot_model import resize_masks
    same = np.zeros((48, 64), np.uint8)
    same[3:5, 7] = 255
    assert np.array_equal(resize_masks([same], 48, 64)[0], same != 0)  # already the frames' size: unchanged
    # worked by hand: 2 x 2 -> 4 x 4 reads source coordinates -0.25, 0.25, 0.75, 1.25, so the pixel (0, 0) reaches target
    # rows / columns 0..2 and not 3
    up = resize_masks([np.array([[255, 0], [0, 0]], np.uint8)], 4, 4)[0]
    want = np.zeros((4, 4), bool)
    want[:3, :3] = True
    assert np.array_equal(up, want)
    # 4 x 4 -> 2 x 2 reads 0.5 and 2.5: the pixel (1, 1) reaches target (0, 0) only
    src = np.zeros((4, 4), np.uint8)
    src[1, 1] = 1
    assert resize_masks([src], 2, 2)[0].tolist() == [[True, False], [False, False]]
    # the real envs' 64 x 85 renders at the default 48 x 64 frames, against the test oracle's restatement
    renders = rmo.RectRenderer(3, H=64, W=85).generate_masks([np.full(7, 0.1 * k) for k in range(4)])
    got = resize_masks(renders, 48, 64)
    assert got.shape == (4, 48, 64) and got.dtype == np.bool_
    for g, m in zip(got, renders):
        assert g.any() and np.array_equal(g, (rmo.img_transform(48, 64)(m)[0] != 0).numpy())
    assert resize_masks([r.astype(np.float32) for r in renders], 48, 64).tolist() == got.tolist()  # float renders too
