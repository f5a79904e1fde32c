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
  * the batches come from the device-resident split (joint_pos_data.DeviceBatches: one gather launch per batch, the host
    loader's order and bits), not from a DataLoader; the host dataset and loaders remain for `plot`'s true masks;
  * `plot` (mask GIFs and IoU) runs under `--plot True` only, needs `renderers` (the reference's MuJoCo mask envs where
    they import) and compares the masks in one `rac_mask_compare` launch;
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
from .joint_pos_data import DeviceBatches, mask_iou, mask_transform
from .optim import make_optimizer
from .robot_model import GripperStatePredictor, JointPosPredictor, RobotModels, mask_renderer

FINETUNE_EXPERIMENTS = ("finetune", "finetune_sawyer_view", "finetune_widowx")  # joint_pos_trainer.py:427


class RobotPredictionTrainer(object):
    def __init__(self, config, logger=None, forward_kinematics=None, renderers=None):
        """`renderers`: {viewpoint: object with the reference mask envs' `generate_masks(list_of_qpos)`}, for `plot`."""
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
        self.renderers = dict(renderers or {})
        self._plot_rng = np.random.RandomState(getattr(config, "seed", 0))
        self.train_loader = self.test_loader = self.training_batch_generator = self.testing_batch_generator = None
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

    def _setup_data(self):
        """joint_pos_trainer.py:434-447: the experiment's host loaders, and both batch generators from the device-resident
        splits.  `test_batches` is the test split's one-epoch form, what `_compute_epoch_metrics` walks."""
        cf = self._config
        if cf.experiment == "finetune_baxter":
            from .joint_pos_data import create_finetune_loaders as create_loaders
        elif cf.experiment == "finetune_widowx":
            from .joint_pos_data import create_loaders
        else:
            raise NotImplementedError(cf.experiment)
        self.train_loader, self.test_loader = create_loaders(cf)
        self.train_batches = DeviceBatches(self.train_loader, self._device)
        self.test_batches = DeviceBatches(self.test_loader, self._device)
        self.training_batch_generator = self.train_batches.forever()
        self.testing_batch_generator = self.test_batches.forever()

    def train(self, batch_generator=None, test_loader=None):
        """Training, evaluation and checkpoint loop (joint_pos_trainer.py:327-368).  Without arguments the data are the
        experiment's (`_setup_data`).  An injected `batch_generator` yields time-first batches (qpos (T, B, J), states
        (T, B, R), actions (T - 1, B, A)); an injected `test_loader` yields batch-first ones; that form never plots.  On the
        experiment's own data `--plot True` writes the mask GIF and IoU where the reference writes them: on an epoch's
        last batch and after each evaluation."""
        cf = self._config
        self._step = self._load_checkpoint(getattr(cf, "dynamics_model_ckpt", None))
        test_generator = None
        if batch_generator is None:
            self._setup_data()
            batch_generator, test_generator = self.training_batch_generator, self.testing_batch_generator
            if test_loader is None:
                test_loader = self.test_batches
        plot = bool(getattr(cf, "plot", False)) and test_generator is not None  # injected batches: no plot, as before
        info = {}
        self.eval_history = []
        self.plot_history = []
        for epoch in range(cf.niter):
            self.models.train()
            for i in range(cf.epoch_size):
                data = next(batch_generator)
                info = dict(self._train_video(data))
                if self._scheduled_sampling:
                    info["sample_schedule"] = self._schedule_prob()[0]
                self._step += 1
                if plot and i == cf.epoch_size - 1:
                    self.plot_history.append(self.plot(data, epoch, "train"))
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
                if plot:
                    self.plot_history.append(self.plot(next(test_generator), epoch, "test"))
        return info

    # ------------------------------------------------------------------ plot
    def _true_masks(self, data, name, b, start, length):
        """(b, length, w, w) true masks of the plotted window: the batch's own where it carries them (a host loader's
        batch), else the host dataset's by `idx` -- the device batches carry none."""
        if "masks" in data:
            return data["masks"][start:start + length, :b, 0].transpose(0, 1).to("cpu", torch.float32)
        loader = self.train_loader if name in ("comparison", "train") else self.test_loader
        if loader is None or "idx" not in data or "start" not in data:
            raise ValueError("plot: the batch has no masks and no (idx, start) of a host dataset to read them from")
        ds = loader.dataset
        return torch.stack([ds.masks(int(i), int(s) + start, length)[:, 0]
                            for i, s in zip(list(data["idx"])[:b], list(data["start"])[:b])])

    @torch.no_grad()
    def plot(self, data, epoch, name, random_start=True):
        """joint_pos_trainer.py:467-567: the joint model's autoregressive rollout of up to 10 videos, rendered to masks and
        compared with the true ones.  One rollout launch, one device-to-host copy of the joint positions, one
        `generate_masks` call per video, one upload of both mask stacks and one `rac_mask_compare` launch for the IoU
        counts and the GIF's frames (per video one row [true | predicted | xor], one GIF frame per time step).
        `data`: a time-first batch.  Returns {"file": <plot_dir>/<name>_<epoch>.gif, "IoU": mean IoU}."""
        from PIL import Image
        cf = self._config
        dev, f32 = self._device, torch.float32
        qpos, ac = torch.as_tensor(data["qpos"]).to(dev, f32), torch.as_tensor(data["actions"]).to(dev, f32)
        b = min(qpos.shape[1], 10)
        length = cf.n_past + cf.n_future if name in ("comparison", "train") else cf.n_eval
        if qpos.shape[0] < length or ac.shape[0] < length - 1:
            raise ValueError(f"plot: a window of {length} steps from a batch of {qpos.shape[0]}")
        start = int(self._plot_rng.randint(0, qpos.shape[0] - length + 1)) if random_start else 0
        folders = list(data["folder"])[:b]
        envs = {v: mask_renderer(self.renderers, cf, v) for v in dict.fromkeys(folders)}
        q0 = qpos[start, :b].contiguous()
        if length > 1:
            jp = self.joint_model.flat_parameters()[0]
            q_all, _ = ops.robot_rollout(jp, None, q0, None, ac[start:start + length - 1, :b].contiguous())
        else:
            q_all = q0.unsqueeze(0)
        q_host = q_all.cpu().numpy()  # the one device-to-host copy
        size = int(cf.image_width)
        pred = torch.stack([mask_transform(envs[vp].generate_masks([q_host[t, i] for t in range(length)]), size)[:, 0]
                            for i, vp in enumerate(folders)])
        true = self._true_masks(data, name, b, start, length)
        if pred.shape != true.shape:
            raise ValueError(f"plot: rendered masks {tuple(pred.shape)}, true masks {tuple(true.shape)}")
        both = torch.stack([pred, true]).to(dev)  # the one upload
        counts, frames = ops.mask_compare(both[0], both[1])
        iou = mask_iou(counts.cpu())
        imgs = [Image.fromarray(f) for f in frames.cpu().numpy()]
        plot_dir = getattr(cf, "plot_dir", None) or os.path.join(cf.log_dir, "plot")
        os.makedirs(plot_dir, exist_ok=True)
        fname = os.path.join(plot_dir, f"{name}_{epoch}.gif")
        imgs[0].save(fname, save_all=True, append_images=imgs[1:], duration=250, loop=0)
        if self._wandb is not None:
            self._wandb.log({f"{name}/gifs": self._wandb.Video(fname, format="gif")}, step=self._step)
            self._wandb.log({f"{name}/IoU": iou}, step=self._step)
        return {"file": fname, "IoU": iou}

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
