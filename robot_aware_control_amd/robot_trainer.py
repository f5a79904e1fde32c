"""Training of the learned robot model (reference src/prediction/joint_pos_trainer.py, `RobotPredictionTrainer`): the
joint-position and gripper-state predictors, trained teacher-forced on (qpos, states, actions) windows.

The reference loops over the window's steps (one forward, one loss and one `.item()` host sync per model and step); the
steps are independent under teacher forcing, so here they are batched as M = (T - 1) B rows: one forward, one loss and
one backward launch chain per model, one fused optimiser step and ONE host sync for the loss dict.  The reference's loss
`sum_i mean_{B,D}((pred_i - target_i)^2)` is then one sum of squares times 1 / (B D).  The autoregressive evaluation is
the rollout kernel (one launch for both models and all steps).

Differences from the reference, all on purpose:
  * `*_joint_eef_pos_loss` (forward kinematics of predicted vs. input joints, MuJoCo) is computed only when the trainer
    has a `forward_kinematics(qpos) -> xyz` callable, and the key is omitted otherwise;
  * `plot` (mask GIFs and IoU) is not built: `train` skips it;
  * loaders can be injected into `train`, in `PredictionTrainer.train`'s style.
Checkpoints are the reference's (`joint_model`, `gripper_model`, `optimizer`, `step`) and load in both directions.
"""
from __future__ import annotations

import os
from collections import defaultdict
from glob import glob
from math import floor

import numpy as np
import torch

from . import _lib, ops
from .optim import make_optimizer
from .robot_model import GripperStatePredictor, JointPosPredictor, RobotModels

FINETUNE_EXPERIMENTS = ("finetune", "finetune_sawyer_view", "finetune_widowx")  # joint_pos_trainer.py:427


class RobotPredictionTrainer(object):
    def __init__(self, config, logger=None, forward_kinematics=None):
        self._config = config
        if not torch.cuda.is_available():
            raise _lib.RacError("RobotPredictionTrainer needs an MI355X (no CPU fallback)")
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
        torch.cuda.set_device(device)
        self._device = config.device = device
        self._logger = logger
        self.forward_kinematics = forward_kinematics
        self._init_models(config)
        self._scheduled_sampling = getattr(config, "scheduled_sampling", False)
        self._step = 0
        self._wandb = None
        if getattr(config, "wandb", False):
            import wandb  # only when asked for (joint_pos_trainer.py:53-66)
            wandb.init(resume=config.jobname, project="robot-prediction", config=config, dir=config.log_dir,
                       entity=config.wandb_entity, group=config.wandb_group, job_type=config.wandb_job_type)
            self._wandb = wandb

    # ------------------------------------------------------------------ setup
    def _init_models(self, cf):
        """joint_pos_trainer.py:80-101: both models, ONE optimiser over joint + gripper parameters."""
        self.joint_model = JointPosPredictor(cf)
        self.gripper_model = GripperStatePredictor(cf)
        self.models = RobotModels(self.joint_model, self.gripper_model).to(self._device)
        self.optimizer = make_optimizer(cf, self.models, False)
        self._loss_dev = torch.zeros(2, device=self._device)

    def _schedule_prob(self):
        """joint_pos_trainer.py:103-110 (logged only: the training is teacher-forced)."""
        k = 10000
        use_truth = k / (k + np.exp(self._step / 3900))
        return [use_truth, 1 - use_truth]

    # ------------------------------------------------------------------ steps
    def _window(self, data, n):
        dev, f32 = self._device, torch.float32
        states = torch.as_tensor(data["states"]).to(dev, f32)
        ac = torch.as_tensor(data["actions"]).to(dev, f32)
        qpos = torch.as_tensor(data["qpos"]).to(dev, f32)
        if len(qpos) < n or len(states) < n or len(ac) < n - 1:
            raise ValueError(f"a window of {n} steps needs {n} states / qpos and {n - 1} actions, got "
                             f"{len(states)} / {len(qpos)} / {len(ac)}")
        return states, ac, qpos

    def _train_step(self, data):
        """Forward and backward pass of both models + one optimiser step (joint_pos_trainer.py:160-216)."""
        cf = self._config
        n = cf.n_past + cf.n_future
        states, ac, qpos = self._window(data, n)
        B = qpos.shape[1]
        a = ac[:n - 1].reshape((n - 1) * B, -1)
        for slot, (model, seq) in enumerate(((self.joint_model, qpos), (self.gripper_model, states))):
            D = seq.shape[-1]
            x, target = seq[:n - 1].reshape(-1, D), seq[1:n].reshape(-1, D)
            params, grads = model.flat_parameters()
            pred, acts = ops.mlp4_forward(params, x, a, residual=True, save=True)
            _, dy = ops.mse_rows(pred, target, 1.0 / (B * D), loss=self._loss_dev[slot:slot + 1], want_grad=True)
            ops.mlp4_backward(params, grads, x, a, acts, dy, accumulate=False)  # overwrites: no zero_grad pass
        self.models.flat_parameters()  # (re-joins the buffers had a model been moved on its own)
        self.optimizer.step()
        joint, gripper = self._loss_dev.tolist()  # the step's one host sync
        # joint_mse is the reference's second name of the same quantity (joint_pos_trainer.py:184-185)
        return {"joint_loss": joint / n, "joint_mse": joint / n, "gripper_loss": gripper / n}

    @torch.no_grad()
    def _eval_step(self, data, autoregressive=False):
        """One n_eval snippet, 1-step or autoregressive (joint_pos_trainer.py:269-325)."""
        cf = self._config
        n = cf.n_eval
        states, ac, qpos = self._window(data, n)
        B = qpos.shape[1]
        prefix = "autoreg" if autoregressive else "1step"
        jp, gp = self.joint_model.flat_parameters()[0], self.gripper_model.flat_parameters()[0]
        q_in = None
        if n > 1:
            if autoregressive:
                q_roll, s_roll = ops.robot_rollout(jp, gp, qpos[0], states[0], ac[:n - 1].contiguous())
                q_in, q_pred, s_pred = q_roll[:n - 1], q_roll[1:], s_roll[1:]
            else:
                a = ac[:n - 1].reshape((n - 1) * B, -1)
                q_in = qpos[:n - 1]
                q_pred, _ = ops.mlp4_forward(jp, q_in.reshape(-1, qpos.shape[-1]), a, residual=True)
                s_pred, _ = ops.mlp4_forward(gp, states[:n - 1].reshape(-1, states.shape[-1]), a, residual=True)
            ops.mse_rows(q_pred.reshape(-1), qpos[1:n].reshape(-1), 1.0 / (B * qpos.shape[-1]), loss=self._loss_dev[0:1])
            ops.mse_rows(s_pred.reshape(-1), states[1:n].reshape(-1), 1.0 / (B * states.shape[-1]),
                         loss=self._loss_dev[1:2])
            joint, gripper = self._loss_dev.tolist()
        else:
            joint = gripper = 0.0
        losses = {f"{prefix}_joint_loss": joint / n, f"{prefix}_joint_mse": joint / n}
        if self.forward_kinematics is not None and n > 1:
            # joint_pos_trainer.py:301-314: end-effector position of the prediction against that of the step's INPUT joints
            fk = self.forward_kinematics
            qp = q_pred.reshape(n - 1, B, -1).cpu().numpy()
            qi = q_in.reshape(n - 1, B, -1).cpu().numpy()
            eef = 0.0
            for t in range(n - 1):
                pred = np.asarray([fk(qp[t, b]) for b in range(B)], dtype=np.float64)
                true = np.asarray([fk(qi[t, b]) for b in range(B)], dtype=np.float64)
                eef += float(np.mean((pred - true) ** 2))
            losses[f"{prefix}_joint_eef_pos_loss"] = eef / n
        losses[f"{prefix}_gripper_loss"] = gripper / n
        return losses

    # ------------------------------------------------------------------ videos
    @staticmethod
    def _slice(data, s, e):
        return {"states": data["states"][s:e], "actions": data["actions"][s:e - 1], "qpos": data["qpos"][s:e],
                "robot": data.get("robot")}

    def _train_video(self, data):
        """Slice a video into n_past + n_future windows and train on each (joint_pos_trainer.py:135-158)."""
        T = data["qpos"].shape[0]
        window = self._config.n_past + self._config.n_future
        all_losses = defaultdict(float)
        for i in range(floor(T / window)):
            for k, v in self._train_step(self._slice(data, i * window, (i + 1) * window)).items():
                all_losses[k] += v / floor(T / window)
        return all_losses

    def _eval_video(self, data, autoregressive=False):
        """Evaluate a whole video in n_eval windows (joint_pos_trainer.py:245-267)."""
        T = data["qpos"].shape[0]
        window = self._config.n_eval
        all_losses = defaultdict(float)
        for i in range(floor(T / window)):
            for k, v in self._eval_step(self._slice(data, i * window, (i + 1) * window), autoregressive).items():
                all_losses[k] += v
        for k in all_losses:
            all_losses[k] /= floor(T / window)
        return all_losses

    def _compute_epoch_metrics(self, data_loader, name):
        """Mean of the 1-step and the autoregressive metrics over a loader (joint_pos_trainer.py:218-243).  Batches are
        batch-first as a DataLoader collates them, or already time-first dicts of a generator."""
        losses = defaultdict(list)
        for data in data_loader:
            data = process_batch(data, self._device)
            for autoregressive in (False, True):
                for k, v in self._eval_video(data, autoregressive=autoregressive).items():
                    losses[k].append(v)
        avg = {f"{name}/{k}": float(np.mean(v)) for k, v in losses.items()}
        if self._logger is not None:
            self._logger.info(", ".join(f"{k}: {v:.5f}" for k, v in avg.items()))
        return avg

    def train(self, batch_generator=None, test_loader=None):
        """Training, evaluation and checkpoint loop (joint_pos_trainer.py:327-368; no plots).  `batch_generator` yields
        time-first batches (qpos (T, B, J), states (T, B, R), actions (T - 1, B, A)); `test_loader` yields batch-first ones."""
        cf = self._config
        self._step = self._load_checkpoint(getattr(cf, "dynamics_model_ckpt", None))
        if batch_generator is None:
            raise NotImplementedError(
                "RobotPredictionTrainer.train: pass batch_generator (and test_loader); the reference's joint-position "
                "dataloaders (src/dataset/*/..._joint_pos_dataloaders.py) are not built")
        info = {}
        self.eval_history = []
        for epoch in range(cf.niter):
            self.models.train()
            for _ in range(cf.epoch_size):
                info = dict(self._train_video(next(batch_generator)))
                if self._scheduled_sampling:
                    info["sample_schedule"] = self._schedule_prob()[0]
                self._step += 1
                if self._wandb is not None:
                    self._wandb.log({f"train/{k}": v for k, v in info.items()}, step=self._step)
            if epoch % cf.checkpoint_interval == 0 and epoch > 0:
                self._save_checkpoint()
            if epoch % cf.eval_interval == 0 and test_loader is not None:
                self.models.eval()
                metrics = self._compute_epoch_metrics(test_loader, "test")
                self.eval_history.append((epoch, metrics))
                if self._wandb is not None:
                    self._wandb.log(metrics, step=self._step)
        return info

    # ------------------------------------------------------------------ checkpoints
    def _save_checkpoint(self):
        """joint_pos_trainer.py:371-379."""
        os.makedirs(self._config.log_dir, exist_ok=True)
        path = os.path.join(self._config.log_dir, f"ckpt_{self._step}.pt")
        clone = lambda sd: {k: v.detach().clone() for k, v in sd.items()}
        torch.save({"joint_model": clone(self.joint_model.state_dict()),
                    "gripper_model": clone(self.gripper_model.state_dict()),
                    "optimizer": self.optimizer.state_dict(), "step": self._step}, path)
        return path

    def _load_checkpoint(self, ckpt_path=None):
        """A given checkpoint, else the newest ckpt_*.pt of log_dir; returns the training step
        (joint_pos_trainer.py:381-432: a given path under the finetune experiments restarts at step 0 with a fresh
        optimiser)."""
        cf = self._config
        given = ckpt_path is not None
        if not given:
            best, best_step = None, 0
            for f in sorted(glob(os.path.join(cf.log_dir, "*.pt"))):
                try:
                    num = int(os.path.basename(f).split(".")[0].rsplit("_", 1)[-1])
                except ValueError:
                    continue
                if num > best_step:
                    best, best_step = f, num
            if best is None:
                return 0
            ckpt_path = best
        ckpt = torch.load(ckpt_path, map_location=self._device)
        self.joint_model.load_state_dict(ckpt["joint_model"])
        self.gripper_model.load_state_dict(ckpt["gripper_model"])
        if given and cf.experiment in FINETUNE_EXPERIMENTS:
            return 0
        self.optimizer.load_state_dict(ckpt["optimizer"])
        return ckpt["step"]


def process_batch(data, device):
    """A DataLoader's batch-first collation -> the trainers' time-first layout on the device (joint_pos_dataset.py
    `process_batch`); a batch that is already time-first (marked by `time_first`) only moves."""
    out = dict(data)
    first = bool(out.pop("time_first", False))
    for k in ("states", "actions", "qpos", "masks"):
        if k in out and torch.is_tensor(out[k]):
            t = out[k].to(device)
            out[k] = t if first else t.transpose(0, 1).contiguous()
    return out
