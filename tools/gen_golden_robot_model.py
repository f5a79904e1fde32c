"""TEST INFRASTRUCTURE ONLY -- golden vectors of the learned robot model (`--learned_robot_model`).

Runs only where the reference checkout is present: it loads oracle/gen_golden.py for its recipe (absent third-party
modules stubbed, the reference first on sys.path so that the name `src` is the reference's), builds the REFERENCE's
JointPosPredictor / GripperStatePredictor on the CPU (fp32) with the name-keyed weights of tests/robot_model_oracle.py
and records inputs and results only -- the weights are regenerated from the seed -- to tests/golden/robot_model.npz:

  * the two deltas of one step and a 3-step residual rollout (the reference's modules called directly);
  * the loss dicts of two consecutive `RobotPredictionTrainer._train_step`s with torch.optim.Adam and a few weight slices
    afterwards, and the 1-step and autoregressive `_eval_step` dicts.  These are the reference's OWN methods
    (src/prediction/joint_pos_trainer.py imports under the stubs), called unbound on a stand-in namespace because the
    constructor wants the MuJoCo mask envs; `_get_gripper_pos` (MuJoCo forward kinematics) is the stand-in
    `robot_model_oracle.fake_fk`.  Should that import fail, the restatements of tests/robot_model_oracle.py are recorded
    instead and the file's `source` entry says so.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_robot_model.py
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


gg = _load("gen_golden", os.path.join(REPO, "oracle", "gen_golden.py"))  # stubs + sys.path: the reference imports now
rmo = _load("robot_model_oracle", os.path.join(REPO, "tests", "robot_model_oracle.py"))

from src.prediction.models.dynamics import GripperStatePredictor, JointPosPredictor  # noqa: E402

EXTRA_STUBS = ("pybullet", "pybullet_data", "pyquaternion")
C = rmo.GOLDEN
J, R, A, B = C["J"], C["R"], C["A"], C["B"]
N_PAST, N_FUTURE, N_EVAL = C["n_past"], C["n_future"], C["n_eval"]
SEED, LR, BETA1 = C["seed"], C["lr"], C["beta1"]
SLICES = (("joint", "predictor.0.weight", (slice(0, 4), slice(None))),
          ("joint", "predictor.2.weight", (slice(0, 4), slice(0, 8))),
          ("joint", "predictor.6.weight", (slice(None), slice(0, 8))),
          ("joint", "predictor.6.bias", (slice(None),)),
          ("gripper", "predictor.4.weight", (slice(0, 4), slice(0, 8))),
          ("gripper", "predictor.6.bias", (slice(None),)))


def models():
    cf = argparse.Namespace(robot_joint_dim=J, robot_dim=R, action_dim=A, n_past=N_PAST, n_future=N_FUTURE, n_eval=N_EVAL)
    joint, gripper = JointPosPredictor(cf), GripperStatePredictor(cf)
    joint.load_state_dict(rmo.make_weights("joint", J, A, SEED))
    gripper.load_state_dict(rmo.make_weights("gripper", R, A, SEED))
    return cf, joint, gripper


def main():
    out = {}
    data = rmo.synth_window(C["data_seed"], N_PAST + N_FUTURE, B, J, R, A)
    for k in ("qpos", "states", "actions"):
        out["in_" + k] = data[k]
    cf, joint, gripper = models()
    with torch.no_grad():
        out["delta_joint"] = joint(data["qpos"][0], data["actions"][0])
        out["delta_gripper"] = gripper(data["states"][0], data["actions"][0])
        q, s = [data["qpos"][0]], [data["states"][0]]
        for a in data["actions"]:
            q.append(joint(q[-1], a) + q[-1])
            s.append(gripper(s[-1], a) + s[-1])
        out["rollout_qpos"], out["rollout_states"] = torch.stack(q), torch.stack(s)
    try:
        gg.MISSING.update(EXTRA_STUBS)  # what the mask envs import on top of the svg trainer's modules
        from src.prediction.joint_pos_trainer import RobotPredictionTrainer as Ref
        source = "reference"
    except Exception as e:  # noqa: BLE001
        print("reference joint_pos_trainer did not import (%s: %s): recording the oracle restatement" % (type(e).__name__, e))
        Ref, source = None, "oracle"
    out["source"] = np.array(source)
    opt = torch.optim.Adam(list(joint.parameters()) + list(gripper.parameters()), lr=LR, betas=(BETA1, 0.999))
    if Ref is not None:
        import src.prediction.joint_pos_trainer as ref_mod
        ref_mod.mse_criterion = torch.nn.MSELoss()  # (src.prediction.losses builds it the same way; robust to the stubs)
        ns = argparse.Namespace(_config=cf, joint_model=joint, gripper_model=gripper, optimizer=opt,
                                _get_gripper_pos=rmo.fake_fk)
        ns._joint_loss = lambda p, t: Ref._joint_loss(ns, p, t)
        ns._gripper_loss = lambda p, t: Ref._gripper_loss(ns, p, t)
        train = lambda: Ref._train_step(ns, data)
        evaluate = lambda ar: Ref._eval_step(ns, data, ar)
    else:
        train = lambda: rmo.train_step(joint, gripper, opt, data, N_PAST, N_FUTURE)
        evaluate = lambda ar: rmo.eval_step(joint, gripper, data, N_EVAL, ar, fk=rmo.fake_fk)
    for step in (1, 2):
        for k, v in train().items():
            out[f"train{step}_{k}"] = v
    sds = {"joint": joint.state_dict(), "gripper": gripper.state_dict()}
    for which, key, sl in SLICES:
        out[f"after_{which}_{key}"] = sds[which][key][sl].clone()
    for ar in (False, True):
        for k, v in evaluate(ar).items():
            out[f"eval_{k}"] = v
    gg.save("robot_model", **out)
    print("source:", source)


if __name__ == "__main__":
    main()
