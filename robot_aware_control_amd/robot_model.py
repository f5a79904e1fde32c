"""The learned robot model (`--learned_robot_model True --robot_model_ckpt <ckpt>`): robot states and masks of the
finetune_* experiments from two small MLPs instead of an analytical model.

`JointPosPredictor` and `GripperStatePredictor` are the reference's modules (src/prediction/models/dynamics.py:269-338):
`in -> 512 -> 512 -> 512 -> D` with ReLU after the first three layers, `forward(x, action)` returns the DELTA and the
caller adds the residual, `state_dict` keys `predictor.{0,2,4,6}.{weight,bias}`.  Here a model's parameters are views of
ONE contiguous block in state_dict order with torch's [out][in] layout

    W1[512][D+A], b1[512], W2[512][512], b2[512], W3[512][512], b3[512], W4[D][512], b4[D]

(and their gradients views of a second block), which is what the kernels of csrc/rac_mlp.hip read: forward, backward and
the T-step residual rollout of both models in one launch.  `RobotModels` puts both models into one buffer so that the
fused optimisers (optim.make_optimizer) step them in one launch, with a state dict interchangeable with a torch.optim one
over `list(joint.parameters()) + list(gripper.parameters())` (joint_pos_trainer.py:98-101).

`LearnedRobotModel` has `PredictionTrainer.robot_model`'s contract: `predict_batch(batch) -> (states, masks)` is the
reference's `_generate_learned_robot_states` (trainer.py:164-257) -- the whole window is rolled out in one launch; with
renderers that render on the device (render.MjcfMaskRenderer, `--robot_mjcf`) the masks are made from the joint positions
where they are, one launch per viewpoint, at the frames' size; with host renderers (MuJoCo on the CPU: any object with
the reference mask envs' `generate_masks(list_of_qpos)`) the predicted joint positions come to the host in one copy, the
masks are rendered, resized to the frames' size as the reference resizes them, and go back in one upload.  The planner's
batch (no `folder`, no `masks`) is answered with every row rendered, row 0 too.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops

HIDDEN = ops.MLP_HIDDEN
MAX_STATE_DIM, MAX_ACTION_DIM = 7, 5  # rac_mlp4_* (include/rac_hip.h)


def param_count(D: int, A: int) -> int:
    return HIDDEN * (D + A) + HIDDEN + 2 * (HIDDEN * HIDDEN + HIDDEN) + D * HIDDEN + D


class _Mlp4Predictor(nn.Module):
    _dim_field = None

    def __init__(self, config):
        super().__init__()
        D, A = int(getattr(config, self._dim_field)), int(config.action_dim)
        if not (1 <= D <= MAX_STATE_DIM and 1 <= A <= MAX_ACTION_DIM):
            raise ValueError(f"{type(self).__name__}: {self._dim_field} in 1..{MAX_STATE_DIM} and action_dim in "
                             f"1..{MAX_ACTION_DIM} are built on the HIP path (got {D}, {A})")
        self.state_dim, self.action_dim = D, A
        # torch's default nn.Linear initialisation on the CPU, in the reference's order (it applies no init_weights to
        # these models): the same seed gives the same initial weights
        self.predictor = nn.Sequential(
            nn.Linear(D + A, HIDDEN), nn.ReLU(inplace=True), nn.Linear(HIDDEN, HIDDEN), nn.ReLU(inplace=True),
            nn.Linear(HIDDEN, HIDDEN), nn.ReLU(inplace=True), nn.Linear(HIDDEN, D))
        self._flatten()

    def numel(self) -> int:
        return param_count(self.state_dim, self.action_dim)

    def _flatten(self, flat=None, grad=None, base=0):
        """Re-home every parameter as a view of one block (and its .grad of another): the blocks are this model's own, or
        the slice [base, base + numel) of a container's buffers."""
        params = list(self.parameters())  # state_dict order
        n = self.numel()
        if flat is None:
            dev = params[0].device
            flat = torch.zeros((n + 3) // 4 * 4, device=dev, dtype=torch.float32)
            grad = torch.zeros_like(flat)
        off = base
        with torch.no_grad():
            for p in params:
                view = flat[off:off + p.numel()].view(p.shape)
                if view.data_ptr() != p.data_ptr():
                    view.copy_(p.data)
                    p.data = view
                p.grad = grad[off:off + p.numel()].view(p.shape)
                p._rac_off = off  # the parameter's place in the buffer the optimiser steps (optim._views)
                off += p.numel()
        assert off - base == n
        self._root = (flat, grad)
        self._flat, self._flat_grad = flat[base:base + n], grad[base:base + n]

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._flatten()
        return out

    def flat_parameters(self):
        """(parameter block, gradient block) in the layout of the module docstring."""
        p0 = self.predictor[0].weight
        if p0.data_ptr() != self._flat.data_ptr() or p0.grad is None or p0.grad.data_ptr() != self._flat_grad.data_ptr():
            self._flatten(*self._root, base=self._flat.storage_offset() - self._root[0].storage_offset())
        return self._flat, self._flat_grad

    def zero_grad(self, set_to_none: bool = False):
        """The kernels accumulate into the gradient block: zero it and keep the views attached."""
        _, grad = self.flat_parameters()
        grad.zero_()

    def forward(self, x, action):
        """The difference between the next and the current state after applying `action` (dynamics.py:290-302)."""
        if not (x.is_cuda and action.is_cuda and self._flat.is_cuda):
            raise _lib.RacError(f"{type(self).__name__} runs on the GPU only (no CPU fallback)")
        flat, grad = self.flat_parameters()
        return ops.Mlp4.apply(x, action, self.predictor[0].weight, flat, grad)


class JointPosPredictor(_Mlp4Predictor):
    """Predicts the change of the robot's joint positions (dynamics.py:269-302)."""
    _dim_field = "robot_joint_dim"


class GripperStatePredictor(_Mlp4Predictor):
    """Predicts the change of the end effector's pose / gripper state (dynamics.py:305-338)."""
    _dim_field = "robot_dim"


class RobotModels(nn.Module):
    """Both predictors in ONE flat parameter buffer (joint block, then the gripper block at the next 16-byte boundary) and
    one gradient buffer: what optim.make_optimizer steps in a single launch.  `parameters()` is
    `list(joint.parameters()) + list(gripper.parameters())`, the reference's optimiser order."""

    def __init__(self, joint_model: JointPosPredictor, gripper_model: GripperStatePredictor):
        super().__init__()
        self.joint_model, self.gripper_model = joint_model, gripper_model
        self._flatten()

    def _flatten(self):
        j, g = self.joint_model, self.gripper_model
        dev = next(j.parameters()).device
        if next(g.parameters()).device != dev:
            raise ValueError("RobotModels: both models must live on one device")
        self._gripper_off = (j.numel() + 3) // 4 * 4
        total = (self._gripper_off + g.numel() + 3) // 4 * 4
        self._flat = torch.zeros(total, device=dev, dtype=torch.float32)
        self._flat_grad = torch.zeros_like(self._flat)
        j._flatten(self._flat, self._flat_grad, 0)
        g._flatten(self._flat, self._flat_grad, self._gripper_off)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._flatten()
        return out

    def flat_parameters(self):
        for m in (self.joint_model, self.gripper_model):
            if m._root[0] is not self._flat:  # a model moved on its own (.to()) since: re-join the two
                self._flatten()
                break
        return self._flat, self._flat_grad

    def zero_grad(self, set_to_none: bool = False):
        self.flat_parameters()[1].zero_()


def resize_masks(rendered, height: int, width: int) -> np.ndarray:
    """The video trainer's `_img_transform` (trainer.py:87-88: ToTensor, then Resize((image_height, image_width))) and the
    `.type(torch.bool)` behind it (trainer.py:222-226), for a list of (H, W) renders of one shape: (n, height, width)
    bool.  uint8 renders are scaled by 1 / 255 as ToTensor does; the resize is the bilinear one without antialiasing of
    the reference's torchvision on tensors (and of this package's data path, data._resize), so a target pixel is set
    where any of its four taps is; renders that already have the target shape pass through unchanged."""
    arr = np.stack([np.asarray(m) for m in rendered])
    if arr.ndim != 3:
        raise ValueError(f"generate_masks must return (H, W) arrays, got {arr.shape[1:]}")
    t = torch.from_numpy(np.ascontiguousarray(arr))
    t = t.to(torch.float32) / 255 if t.dtype == torch.uint8 else t.to(torch.float32)
    if tuple(t.shape[-2:]) != (height, width):
        t = F.interpolate(t.unsqueeze(1), size=(height, width), mode="bilinear", align_corners=False).squeeze(1)
    return (t != 0).numpy()


_EXPERIMENT_ROBOT = {"finetune": "baxter", "finetune_baxter": "baxter", "finetune_widowx": "widowx",
                     "finetune_sawyer_view": "sawyer"}


def mjcf_mask_renderer(config, viewpoint, camera_table=None):
    """An `MjcfMaskRenderer` (render.py: masks rendered on the device) of `--robot_mjcf`, its camera
    `--robot_mjcf_camera` posed from the calibration `--model_use_heatmap` reads (heatmaps.CameraTable, key
    `<robot>_<viewpoint>` with the experiment's robot, or `viewpoint` itself).  NotImplementedError when the
    calibration has no such entry."""
    from .heatmaps import CameraTable
    from .render import MjcfMaskRenderer
    exp = getattr(config, "experiment", None)
    table = camera_table if camera_table is not None else CameraTable.from_config(config)
    keys = ([f"{_EXPERIMENT_ROBOT[exp]}_{viewpoint}"] if exp in _EXPERIMENT_ROBOT else []) + [str(viewpoint)]
    key = next((k for k in keys if k in table.world_to_camera), None)
    if key is None:
        raise NotImplementedError(
            f"no mask renderer for viewpoint {viewpoint!r}: --robot_mjcf {config.robot_mjcf} is set, but the camera "
            f"calibration (--camera_calibration, heatmaps.CameraTable) has no world_to_camera entry {' or '.join(keys)} "
            f"(it has {sorted(table.world_to_camera)}); pass renderers={{viewpoint: env}} to LearnedRobotModel, env being "
            f"any object with generate_masks(list_of_qpos) -> list of (H, W) arrays")
    camera = getattr(config, "robot_mjcf_camera", None) or "main_cam"
    env = MjcfMaskRenderer(config.robot_mjcf, camera=camera)
    env.set_opencv_camera_pose(camera, np.linalg.inv(table.world_to_camera[key]))
    return env


def mask_renderer(renderers, config, viewpoint, camera_table=None):
    """`renderers[viewpoint]`, built on first use: from `--robot_mjcf` when that is set (mjcf_mask_renderer), else from
    the reference's MuJoCo mask envs (trainer.py:183-203, joint_pos_trainer.py:481-500) where those import; shared by
    LearnedRobotModel and RobotPredictionTrainer.plot."""
    env = renderers.get(viewpoint)
    if env is not None:
        return env
    exp = getattr(config, "experiment", None)
    if getattr(config, "robot_mjcf", None):
        env = renderers[viewpoint] = mjcf_mask_renderer(config, viewpoint, camera_table)
        return env
    try:  # the reference's MuJoCo mask envs: only inside a full reference checkout
        from src.utils.camera_calibration import camera_to_world_dict
        if exp in ("finetune", "finetune_baxter"):
            from src.env.robotics.masks.baxter_mask_env import BaxterMaskEnv
            env = BaxterMaskEnv()
            env.arm = "left"
            cam_ext = camera_to_world_dict[f"baxter_{viewpoint}"]
        elif exp == "finetune_widowx":
            from src.env.robotics.masks.widowx_mask_env import WidowXMaskEnv
            env = WidowXMaskEnv()
            cam_ext = camera_to_world_dict[f"widowx_{viewpoint}"]
        elif exp == "finetune_sawyer_view":
            from src.env.robotics.masks.sawyer_mask_env import SawyerMaskEnv
            env = SawyerMaskEnv()
            cam_ext = camera_to_world_dict[f"sawyer_{viewpoint}"]
        else:
            raise ValueError(exp)
        env.set_opencv_camera_pose("main_cam", cam_ext)
    except Exception as e:
        raise NotImplementedError(
            f"no mask renderer for viewpoint {viewpoint!r}: pass renderers={{viewpoint: env}} to LearnedRobotModel, "
            f"env being any object with generate_masks(list_of_qpos) -> list of (H, W) arrays.  The reference's "
            f"MuJoCo mask envs (src.env.robotics.masks.*, experiment {exp!r}) exist only inside a full reference "
            f"checkout and could not be imported here ({type(e).__name__}: {e})") from e
    renderers[viewpoint] = env
    return env


class LearnedRobotModel:
    """`PredictionTrainer.robot_model` over the two learned predictors.  `renderers`: {viewpoint: object with the reference
    mask envs' `generate_masks(list_of_qpos) -> list of (H, W) arrays`}, looked up by `batch["folder"]`."""

    def __init__(self, config, joint_model, gripper_model, renderers=None, camera_table=None):
        self._config = config
        self.joint_model, self.gripper_model = joint_model, gripper_model
        self.renderers = dict(renderers or {})
        self.camera_table = camera_table  # heatmaps.CameraTable; None: read per the config on first use

    def rollout(self, qpos0, state0, actions):
        """qpos[t+1] = qpos[t] + joint(qpos[t], a[t]) and states[t+1] = states[t] + gripper(states[t], a[t]) for the T
        steps of actions (T, N, A), in one launch: (qpos (T+1, N, J), states (T+1, N, R)).  T = 0 launches nothing."""
        jp, gp = self.joint_model.flat_parameters()[0], self.gripper_model.flat_parameters()[0]
        if not (jp.is_cuda and gp.is_cuda):
            raise _lib.RacError("LearnedRobotModel runs on the GPU only (no CPU fallback)")
        dev = jp.device
        qpos0 = torch.as_tensor(qpos0).to(dev, torch.float32)
        state0 = torch.as_tensor(state0).to(dev, torch.float32)
        actions = torch.as_tensor(actions).to(dev, torch.float32)
        if actions.shape[0] == 0:
            return qpos0.unsqueeze(0).clone(), state0.unsqueeze(0).clone()
        if actions.shape[-1] != self.joint_model.action_dim or actions.shape[-1] != self.gripper_model.action_dim:
            raise ValueError(f"actions of width {actions.shape[-1]}, the models take {self.joint_model.action_dim}")
        return ops.robot_rollout(jp, gp, qpos0, state0, actions)

    def _renderer(self, viewpoint):
        return mask_renderer(self.renderers, self._config, viewpoint, self.camera_table)

    def _predict_candidates(self, data):
        """The planner's form of `predict_batch` (trajectory_sampler.py:86-109): `states` (T+1, N, R), `qpos` (T+1, N, J)
        with row 0 filled, `actions` (T, N, A) -> (states (T+1, N, R), masks (T+1, N, 1, h, w)) on the device, every
        row -- row 0 too -- rendered from its joint positions by the one renderer (or `default_viewpoint`'s)."""
        cf = self._config
        if len(self.renderers) == 1:
            env = next(iter(self.renderers.values()))
        else:
            vp = getattr(cf, "default_viewpoint", None)
            if vp is None:
                raise ValueError("LearnedRobotModel.predict_batch on a planner batch needs one renderer or "
                                 "config.default_viewpoint to choose one")
            env = self._renderer(vp)
        q, s = self.rollout(data["qpos"][0], data["states"][0], data["actions"])
        rows, N, J = q.shape
        h, w = int(cf.image_height), int(cf.image_width)
        if not hasattr(env, "render"):
            raise NotImplementedError("LearnedRobotModel.predict_batch on a planner batch renders every candidate on the "
                                      "device: its renderer needs render(qpos) (render.MjcfMaskRenderer)")
        return s, env.render(q.reshape(rows * N, J), out_hw=(h, w)).view(rows, N, 1, h, w)

    @torch.no_grad()
    def predict_batch(self, batch, thick=False):
        """The reference's `_generate_learned_robot_states` (trainer.py:164-257): (states, masks) shaped like the batch's,
        row 0 the ground truth, rows 1..T the models' rollout from row 0 over the window's actions (`raw_actions` when
        `preprocess_action != "raw"`) and the render of every predicted joint position from its sample's viewpoint.
        With `model_use_heatmap` a third tensor: the batch's `heatmaps` with rows 1..T rebuilt from the predicted states
        (trainer.py:234-256), each sample with its own `low` / `high` / `robot` / `folder`, in one launch.
        Renderers with `render` (render.MjcfMaskRenderer) take the device route: one launch per distinct viewpoint on
        the predicted joint positions where they are, written into the masks -- no copy to the host and none back.
        A batch without `folder` and `masks` is the planner's (`_predict_candidates`); `thick` is the analytical models'
        argument and changes nothing here (the reference's wx250s environment always renders every geom)."""
        cf = self._config
        if "folder" not in batch and "masks" not in batch:
            return self._predict_candidates(batch)
        use_heatmap = bool(getattr(cf, "model_use_heatmap", False))
        if use_heatmap and "heatmaps" not in batch:
            raise NotImplementedError("model_use_heatmap with the learned robot model: the batch carries no `heatmaps` "
                                      "to keep row 0 of (the heatmap rows 1..T are rebuilt from the predicted states, "
                                      "trainer.py:234-256)")
        states, mask, qpos = batch["states"], batch["masks"], batch["qpos"]
        ac = batch["actions"] if getattr(cf, "preprocess_action", "raw") == "raw" else batch["raw_actions"]
        folders = list(batch["folder"])
        envs = {v: self._renderer(v) for v in dict.fromkeys(folders)}
        q, s = self.rollout(qpos[0], states[0], ac)
        T, B = q.shape[0] - 1, q.shape[1]
        dev = q.device
        pred_states = torch.zeros(tuple(states.shape), device=dev, dtype=torch.float32)
        pred_states[:T + 1] = s
        pred_masks = torch.zeros(tuple(mask.shape), device=dev, dtype=mask.dtype)
        pred_masks[0] = torch.as_tensor(mask[0]).to(dev)
        if T and all(hasattr(env, "render") for env in envs.values()):
            h, w = int(cf.image_height), int(cf.image_width)
            if (h, w) != tuple(mask.shape[-2:]):
                raise ValueError(f"image_height x image_width is {h} x {w}, the batch's masks are {tuple(mask.shape[-2:])}")
            J = q.shape[-1]
            for vp, env in envs.items():
                cols = [b for b, f in enumerate(folders) if f == vp]
                if len(cols) == B and pred_masks.dtype == torch.float32 and tuple(mask.shape[2:]) == (1, h, w):
                    env.render(q[1:].reshape(T * B, J), out_hw=(h, w), out=pred_masks[1:T + 1].view(T * B, 1, h, w))
                else:
                    idx = torch.tensor(cols, device=dev)
                    rendered = env.render(q[1:].index_select(1, idx).reshape(T * len(cols), J), out_hw=(h, w))
                    pred_masks[1:T + 1, idx] = rendered.view((T, len(cols)) + tuple(mask.shape[2:])).to(mask.dtype)
        elif T:
            q_host = q[1:].cpu().numpy()  # the one device-to-host copy of the window
            h, w = int(cf.image_height), int(cf.image_width)
            if (h, w) != tuple(mask.shape[-2:]):
                raise ValueError(f"image_height x image_width is {h} x {w}, the batch's masks are {tuple(mask.shape[-2:])}")
            host = np.zeros((T, B) + tuple(mask.shape[2:]), dtype=np.bool_)
            for b, vp in enumerate(folders):
                rendered = envs[vp].generate_masks([q_host[t, b] for t in range(T)])
                host[:, b, 0] = resize_masks(rendered, h, w)
            pred_masks[1:T + 1] = torch.from_numpy(host).to(dev).to(mask.dtype)  # the one upload
        if use_heatmap:
            return pred_states, pred_masks, rebuilt_heatmaps(self, cf, batch, pred_states, T)
        return pred_states, pred_masks


def rebuilt_heatmaps(model, config, batch, pred_states, T: int, bounds=("low", "high")):
    """A clone of `batch["heatmaps"]` with rows 1..T made from `pred_states[1:T + 1]` (trainer.py:234-246,
    locobot_model.py:179-193); `model.camera_table` is read per the config on first use."""
    from .heatmaps import CameraTable, batch_heatmaps
    if model.camera_table is None:
        model.camera_table = CameraTable.from_config(config)
    heat = batch["heatmaps"]
    heat = torch.as_tensor(heat).to(pred_states.device, torch.float32).clone().contiguous()
    if T:
        batch_heatmaps(pred_states[1:T + 1], batch[bounds[0]], batch[bounds[1]], list(batch["robot"]),
                       list(batch["folder"]), model.camera_table, heat.shape[-2], heat.shape[-1], out=heat, first_row=1)
    return heat
