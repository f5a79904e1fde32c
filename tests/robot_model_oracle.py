"""TEST INFRASTRUCTURE ONLY -- the learned robot model restated in plain torch on the CPU, in fp32 or fp64.

The two predictors as `nn.Sequential` stacks (reference dynamics.py:269-338), name-keyed seeded weights in the manner of
tests/det_oracle.make_weights, and the reference's loops restated step by step: `RobotPredictionTrainer._train_step` /
`_eval_step` (joint_pos_trainer.py:160-216, :269-325) and `PredictionTrainer._generate_learned_robot_states`
(trainer.py:164-257).  tests/test_robot_model_host.py checks these restatements against the reference's own numbers
(tests/golden/robot_model.npz, tools/gen_golden_robot_model.py)."""
import math
import zlib
from collections import defaultdict

import numpy as np
import torch
import torch.nn as nn

HIDDEN = 512
# the configuration of tests/golden/robot_model.npz (tools/gen_golden_robot_model.py)
GOLDEN = dict(J=7, R=5, A=5, B=3, n_past=2, n_future=2, n_eval=4, seed=11, lr=1e-3, beta1=0.9, data_seed=5)
KEYS = tuple(f"predictor.{i}.{n}" for i in (0, 2, 4, 6) for n in ("weight", "bias"))


def shapes(D, A):
    dims = [(HIDDEN, D + A), (HIDDEN, HIDDEN), (HIDDEN, HIDDEN), (D, HIDDEN)]
    return {f"predictor.{2 * i}.{n}": (s if n == "weight" else s[:1]) for i, s in enumerate(dims) for n in ("weight", "bias")}


def make_weights(tag, D, A, seed=0):
    """State dict of one predictor: Philox keyed by crc32(tag.key) and the seed; 1/sqrt(fan_in) weights, 0.05 biases."""
    out = {}
    for key, shape in shapes(D, A).items():
        rng = np.random.Generator(np.random.Philox(key=[zlib.crc32(f"{tag}.{key}".encode()), seed]))
        std = 1.0 / math.sqrt(shape[1]) if key.endswith("weight") else 0.05
        out[key] = torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * np.float32(std))
    return out


class Predictor(nn.Module):
    """in -> 512 -> 512 -> 512 -> D; forward(x, action) returns the delta."""

    def __init__(self, D, A):
        super().__init__()
        self.predictor = nn.Sequential(nn.Linear(D + A, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, HIDDEN), nn.ReLU(),
                                       nn.Linear(HIDDEN, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, D))

    def forward(self, x, action):
        return self.predictor(torch.cat([x, action], 1))


def build(sd, dtype=torch.float32):
    D, A = sd["predictor.6.bias"].shape[0], sd["predictor.0.weight"].shape[1] - sd["predictor.6.bias"].shape[0]
    m = Predictor(D, A)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    return m.to(dtype)


def synth_window(seed, T, B, J, R, A, dtype=torch.float32):
    """qpos (T, B, J), states (T, B, R), actions (T - 1, B, A) of one window."""
    g = np.random.Generator(np.random.Philox(key=[seed, 4242]))
    n = lambda *s, scale: torch.from_numpy(g.standard_normal(s, dtype=np.float32) * np.float32(scale)).to(dtype)
    return {"qpos": n(T, B, J, scale=0.5), "states": n(T, B, R, scale=0.5), "actions": n(T - 1, B, A, scale=0.1),
            "robot": ["widowx"] * B}


def cast(data, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in data.items()}


def mse(pred, target):
    return ((pred - target) ** 2).mean()


def fake_fk(q):
    """A stand-in for the MuJoCo forward kinematics of `_get_gripper_pos`: any fixed smooth map qpos -> xyz."""
    q = np.asarray(q, dtype=np.float64)
    return np.array([q.sum(), q[0] - q[1], 0.5 * q[2] * q[2]])


def train_step(joint, gripper, optimizer, data, n_past, n_future):
    """joint_pos_trainer.py:160-216."""
    losses = defaultdict(float)
    joint_loss = gripper_loss = 0
    states, ac, qpos = data["states"], data["actions"], data["qpos"]
    joint.zero_grad()
    gripper.zero_grad()
    for i in range(1, n_past + n_future):
        r_j, a_j, q_j, q_i = states[i - 1], ac[i - 1], qpos[i - 1], qpos[i]
        q_pred = joint(q_j, a_j) + q_j
        q_loss = mse(q_pred, q_i)
        joint_loss = joint_loss + q_loss
        losses["joint_loss"] += q_loss.item()
        losses["joint_mse"] += mse(q_pred, q_i).item()
        r_pred = gripper(r_j, a_j) + r_j
        r_loss = mse(r_pred, states[i])
        gripper_loss = gripper_loss + r_loss
        losses["gripper_loss"] += r_loss.item()
    (joint_loss + gripper_loss).backward()
    optimizer.step()
    return {k: v / (n_past + n_future) for k, v in losses.items()}


@torch.no_grad()
def eval_step(joint, gripper, data, n_eval, autoregressive=False, fk=None):
    """joint_pos_trainer.py:269-325; the end-effector term only with a forward-kinematics callable."""
    states, ac, qpos = data["states"], data["actions"], data["qpos"]
    losses = defaultdict(float)
    prefix = "autoreg" if autoregressive else "1step"
    for i in range(1, n_eval):
        if autoregressive and i > 1:
            q_j, r_j = q_pred.clone(), r_pred.clone()  # noqa: F821
        else:
            q_j, r_j = qpos[i - 1], states[i - 1]
        a_j = ac[i - 1]
        q_pred = joint(q_j, a_j) + q_j
        losses[f"{prefix}_joint_loss"] += mse(q_pred, qpos[i]).item()
        losses[f"{prefix}_joint_mse"] += mse(q_pred, qpos[i]).item()
        if fk is not None:
            pred = torch.from_numpy(np.asarray([fk(q.numpy()) for q in q_pred]))
            true = torch.from_numpy(np.asarray([fk(q.numpy()) for q in q_j]))
            losses[f"{prefix}_joint_eef_pos_loss"] += mse(pred, true).item()
        r_pred = gripper(r_j, a_j) + r_j
        losses[f"{prefix}_gripper_loss"] += mse(r_pred, states[i]).item()
    return {k: v / n_eval for k, v in losses.items()}


@torch.no_grad()
def rollout(joint, gripper, qpos0, state0, actions):
    q, s = [qpos0], [state0]
    for a in actions:
        q.append(joint(q[-1], a) + q[-1])
        s.append(gripper(s[-1], a) + s[-1])
    return torch.stack(q), torch.stack(s)


@torch.no_grad()
def generate_learned_robot_states(joint, gripper, data, renderers, transform, preprocess_action="raw"):
    """trainer.py:164-257 (no heatmaps): (states, masks), one render per predicted qpos and sample, in the reference's
    order; `transform(mask)` is its `_img_transform` (`img_transform` below)."""
    states, mask, qpos = data["states"], data["masks"], data["qpos"]
    ac = data["actions"] if preprocess_action == "raw" else data["raw_actions"]
    pred_states, pred_masks = torch.zeros_like(states), torch.zeros_like(mask)
    pred_states[0], pred_masks[0] = states[0], mask[0]
    q_j, r_j = qpos[0], states[0]
    for i in range(1, len(ac) + 1):
        a_j = ac[i - 1]
        r_pred = gripper(r_j, a_j) + r_j
        q_pred = joint(q_j, a_j) + q_j
        pred_states[i] = r_pred
        for b in range(q_pred.shape[0]):
            m = renderers[data["folder"][b]].generate_masks([q_pred[b].cpu().numpy()])[0]
            pred_masks[i][b] = transform(m).to(torch.bool)
        q_j, r_j = q_pred, r_pred
    return pred_states, pred_masks


def img_transform(height, width):
    """trainer.py:87-88 restated without torchvision: ToTensor (uint8 (H, W) -> float (1, H, W) / 255), then
    Resize((height, width)) -- bilinear, no antialiasing, as the reference's torchvision resizes tensors."""
    def apply(m):
        t = torch.from_numpy(np.ascontiguousarray(m)).unsqueeze(0)
        t = t.float().div(255) if t.dtype == torch.uint8 else t.float()
        return torch.nn.functional.interpolate(t.unsqueeze(0), size=(height, width), mode="bilinear",
                                               align_corners=False)[0]
    return apply


class RectRenderer:
    """A deterministic stand-in for a MuJoCo mask env: a rectangle whose corner is a fixed function of the qpos rounded to
    3 decimals and of the viewpoint's offset, so that a wrong qpos row or viewpoint gives a different mask."""

    def __init__(self, offset, H=48, W=64):
        self.offset, self.H, self.W = offset, H, W
        self.calls = []

    def generate_masks(self, qpos_list):
        out = []
        for q in qpos_list:
            q = np.round(np.asarray(q, dtype=np.float64), 3)
            self.calls.append(q.copy())
            key = int(abs(q * 1000).sum()) + self.offset
            top, left = key % (self.H - 8), (key // 7) % (self.W - 8)
            m = np.zeros((self.H, self.W), dtype=np.uint8)
            m[top:top + 6, left:left + 5] = 255
            out.append(m)
        return out


def golden_inputs(g, dtype=torch.float32):
    return cast({k: torch.from_numpy(g["in_" + k]) for k in ("qpos", "states", "actions")}, dtype)


def golden_recipe(g, dtype):
    """Everything tests/golden/robot_model.npz records, on the oracle in `dtype`: the deltas of one step, the rollout, two
    Adam train steps, the weight slices afterwards and the two eval dicts (of the trained weights), keyed as the file."""
    c = GOLDEN
    data = golden_inputs(g, dtype)
    joint = build(make_weights("joint", c["J"], c["A"], c["seed"]), dtype)
    gripper = build(make_weights("gripper", c["R"], c["A"], c["seed"]), dtype)
    out = {}
    with torch.no_grad():
        out["delta_joint"] = joint(data["qpos"][0], data["actions"][0])
        out["delta_gripper"] = gripper(data["states"][0], data["actions"][0])
    out["rollout_qpos"], out["rollout_states"] = rollout(joint, gripper, data["qpos"][0], data["states"][0], data["actions"])
    opt = torch.optim.Adam(list(joint.parameters()) + list(gripper.parameters()), lr=c["lr"], betas=(c["beta1"], 0.999))
    for step in (1, 2):
        for k, v in train_step(joint, gripper, opt, data, c["n_past"], c["n_future"]).items():
            out[f"train{step}_{k}"] = torch.tensor(v, dtype=torch.float64)
    sds = {"joint": joint.state_dict(), "gripper": gripper.state_dict()}
    for key in g.files:
        if key.startswith("after_"):
            which, name = key[len("after_"):].split("_", 1)
            out[key] = sds[which][name][tuple(slice(0, n) for n in g[key].shape)].clone()
    for ar in (False, True):
        for k, v in eval_step(joint, gripper, data, c["n_eval"], ar, fk=fake_fk).items():
            out[f"eval_{k}"] = torch.tensor(v, dtype=torch.float64)
    return out
