"""PredictionTrainer: the SVG train step (and the `--model det | copy` baselines) on librac_hip.so, API-compatible
with the reference `src/prediction/trainer.py` (`PredictionTrainer(config)`, `_train_step`, `_train_video`, `train`,
checkpoint format `{"model","optimizer","step"}`, ckpt_{step}.pt discovery).

MI355X-first differences:
  * no host sync inside the time loop: the 4 `.item()` calls per time step of the reference
    (trainer.py:433-458) become one device->host copy per train step;
  * zero_robot_region of the input frame is fused into the encoder's input packing;
  * parameter gradients accumulate in place in one flat buffer; the DDP gradient all-reduce
    (RCCL over xGMI, one process per GPU) runs on slices of that buffer, Adam is one launch.
"""
from __future__ import annotations

import os
from collections import defaultdict
from glob import glob
from math import floor
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

from . import ops, parallel_env
from .model import CopyModel, DeterministicConvModel, SVGConvModel
from .optim import FusedAdam, ShardedAdam, make_optimizer

# teacher-forced windows run the encoder / decoder once over all time steps (RAC_SEQUENCE_PATH=0: step by step)
SEQUENCE_PATH = os.environ.get("RAC_SEQUENCE_PATH", "1") == "1"


def _dist_on() -> bool:
    return parallel_env.active()


def allreduce_flat_grad(flat_grad: torch.Tensor, bucket_mb: int = 64):
    """Mean of the flat gradient over all ranks: bucketed async all-reduce (RCCL; each bucket is a
    contiguous slice, so there is no pack/unpack copy), then one scale."""
    if not _dist_on():
        return
    red = GradReducer(flat_grad, bucket_mb)
    red.finish()


class GradReducer:
    """Data-parallel mean of the flat gradient buffer, overlapped with the tail of backward.

    The ConvLSTM gate weights are 90 % of the parameters (214 M of 238.6 M at g512) and their gradients are the LAST
    thing backward produces (one time-batched wgrad launch per weight when `ops.deferred_wgrad()` exits).  `ready(p)`
    is called right after a weight's launch is enqueued: the all-reduce of that weight's slice starts on RCCL's
    stream while the next weight's wgrad computes.  `finish()` reduces whatever has not been reduced yet (vgg
    stack, input convs, heads, biases: 10 %), waits for everything and applies the 1/world scale once."""

    def __init__(self, flat_grad: torch.Tensor, bucket_mb: int = 64):
        self.flat = flat_grad
        self.step = max(1, bucket_mb * (1 << 20) // 4)
        self.works = []
        self.done = []  # reduced [start, end) element ranges

    def _reduce(self, start: int, end: int):
        for s in range(start, end, self.step):
            e = min(end, s + self.step)
            self.works.append(dist.all_reduce(self.flat[s:e], op=dist.ReduceOp.SUM, async_op=True))

    def ready(self, param: torch.Tensor):
        g = param.grad
        if g is None or g.untyped_storage().data_ptr() != self.flat.untyped_storage().data_ptr():
            return  # not a view of the flat buffer: left to finish()
        start = g.storage_offset() - self.flat.storage_offset()
        self._reduce(start, start + g.numel())
        self.done.append((start, start + g.numel()))

    def finish(self):
        pos = 0
        for start, end in sorted(self.done):
            if start > pos:
                self._reduce(pos, start)
            pos = max(pos, end)
        if pos < self.flat.numel():
            self._reduce(pos, self.flat.numel())
        for w in self.works:
            w.wait()
        self.flat.mul_(1.0 / dist.get_world_size())


class ShardReducer:
    """The sharded optimiser's half of the exchange (optim.ShardedAdam): a reduce-scatter (SUM) per bucket of the flat
    gradient, issued as soon as every weight gradient inside the bucket is final -- the ConvLSTM weights' buckets right
    after their time-batched wgrad launch (`ready`), the rest in `finish()`.  Rank r's slice of each bucket is reduced
    IN PLACE (output = that slice of the input bucket)."""

    def __init__(self, flat_grad: torch.Tensor, buckets, world: int, rank: int):
        self.flat, self.buckets, self.world, self.rank = flat_grad, buckets, world, rank
        self.covered = [0] * len(buckets)
        self.issued = [False] * len(buckets)
        self.works = []

    def _issue(self, b: int):
        start, size = self.buckets[b]
        n = size // self.world
        bucket = self.flat[start:start + size]
        self.works.append(dist.reduce_scatter_tensor(bucket[self.rank * n:(self.rank + 1) * n], bucket,
                                                     op=dist.ReduceOp.SUM, async_op=True))
        self.issued[b] = True

    def ready(self, param: torch.Tensor):
        g = param.grad
        if g is None or g.untyped_storage().data_ptr() != self.flat.untyped_storage().data_ptr():
            return
        lo = g.storage_offset() - self.flat.storage_offset()
        hi = lo + g.numel()
        for b, (start, size) in enumerate(self.buckets):
            ov = min(hi, start + size) - max(lo, start)
            if ov > 0 and lo <= start and start + size <= hi and not self.issued[b]:
                self._issue(b)  # the bucket lies inside this weight's gradient: final now

    def finish(self):
        for b in range(len(self.buckets)):
            if not self.issued[b]:
                self._issue(b)
        for w in self.works:
            w.wait()


def model_step(model, cf, i, x_j, masks, states, ac, heatmaps, skip, *, posterior, force_use_prior=False, dontcare):
    """One model step of a rollout: frame i's decoder output from the frame `x_j` fed as frame i - 1 and the window's
    (T, B, ...) `masks`, `states`, `ac` and `heatmaps` (None: no heatmap input).  Returns (x4, the skip maps for the
    next step, (mu, logvar, mu_p, logvar_p)) -- `--model det` has no latents: None.  The caller picks `x_j`,
    composites `x4` over it and scores the frame.  (The trainer's rollouts and `action_rollout.rollout` share it.)"""
    m_j, r_j, a_j = masks[i - 1], states[i - 1], ac[i - 1]
    if cf.last_frame_skip:
        skip = None
    m_in = torch.cat([m_j, masks[i]], 1) if cf.model_use_future_mask else m_j
    zero_mask = m_j if dontcare else None
    if cf.model == "det":  # trainer.py:383-384, 628-629: no prior / posterior, no future robot state, no heatmap
        x4, curr_skip = model.forward_maps(x_j, m_in, r_j, a_j, skip, zero_mask=zero_mask)
        latents = None
    else:
        r_in = (r_j, states[i]) if cf.model_use_future_robot_state else r_j
        hm_in = None
        if heatmaps is not None:
            hm_in = torch.cat([heatmaps[i - 1], heatmaps[i]], 1) if cf.model_use_future_heatmap else heatmaps[i - 1]
        x4, curr_skip, *latents = model.forward_maps(
            x_j, m_in, r_in, hm_in, a_j, posterior, states[i] if posterior else None, skip,
            force_use_prior=force_use_prior, zero_mask=zero_mask)
    return x4, (curr_skip if i <= cf.n_past else skip), latents  # the encoder's skip maps of the context frames only


class PredictionTrainer(object):
    """Video prediction training (reference trainer.py:53-897, hot path only)."""

    def __init__(self, config, logger=None):
        self._config = config
        if not torch.cuda.is_available():
            raise ops._lib.RacError("PredictionTrainer needs an MI355X (no CPU fallback)")
        local = int(os.environ.get("LOCAL_RANK", 0))
        device = torch.device("cuda", local)
        torch.cuda.set_device(device)
        self._device = config.device = device
        self._logger = logger
        self.robot_model = None  # finetune_* experiments: predict_batch(batch) -> (states, masks)
        self._init_models(config)
        self._scheduled_sampling = config.scheduled_sampling
        self._step = 0
        self._plot_rng = np.random.RandomState(self._config.seed)
        self._video_sample_rng = np.random.RandomState(self._config.seed)
        self._grad_seeds = {}
        self._loss_host = None  # pinned staging buffer of the per-step loss readback
        self.phase_events = None  # set to [] to record (name, cuda event) marks of every train step (bench.py)
        # the model / optimiser object graph is static from here on: keep the cyclic GC's full collections from
        # walking it (measured: one 33 ms host stall every ~10 train steps at cfg2, during which the GPU drains)
        if os.environ.get("RAC_GC_FREEZE", "0") == "1":  # opt-in (bench.py, the CLI): process-global and irreversible
            import gc
            gc.collect()
            gc.freeze()
        self._wandb = None
        if getattr(config, "wandb", False):
            import wandb  # only when asked for (reference trainer.py:70-84)
            wandb.init(resume=config.jobname, project=config.wandb_project, config=config, dir=config.log_dir,
                       entity=config.wandb_entity, group=config.wandb_group, job_type=config.wandb_job_type)
            self._wandb = wandb

    # ------------------------------------------------------------------ setup
    def _init_models(self, cf):
        # trainer.py:99-107: svg, det, copy (cdna_det is the reference's ValueError here too)
        if cf.model == "svg":
            self.model = SVGConvModel(cf).to(self._device)
        elif cf.model == "det":
            self.model = DeterministicConvModel(cf).to(self._device)
        elif cf.model == "copy":
            self.model = CopyModel()  # no parameters, no optimiser (trainer.py:103-105)
            self.optimizer = None
            return
        else:
            raise ValueError(f"{cf.model}: --model svg, det and copy are built on the HIP path")
        if _dist_on():  # identical initial weights on every rank
            dist.broadcast(self.model.flat_parameters()[0], src=0)
        # --optimizer adam | rmsprop | sgd (trainer.py:109-122); anything else is the reference's ValueError
        self.optimizer = make_optimizer(cf, self.model, bool(getattr(cf, "ddp_shard_optimizer", False) and _dist_on()))
        if ("finetune" in cf.experiment and cf.experiment != "finetune_locobot"
                and getattr(cf, "learned_robot_model", False)):
            # --learned_robot_model True: states and masks of the finetune windows from the learned MLPs (trainer.py:123-130)
            from .robot_model import GripperStatePredictor, JointPosPredictor, LearnedRobotModel
            self.joint_model = JointPosPredictor(cf).to(self._device)
            self.gripper_model = GripperStatePredictor(cf).to(self._device)
            self._load_robot_model_checkpoint(getattr(cf, "robot_model_ckpt", None))
            self.robot_model = LearnedRobotModel(cf, self.joint_model, self.gripper_model)

    def _load_robot_model_checkpoint(self, ckpt_path):
        """The two predictors of a RobotPredictionTrainer checkpoint (trainer.py:839-844)."""
        if not ckpt_path or not os.path.exists(ckpt_path):
            raise ValueError(f"--learned_robot_model True needs --robot_model_ckpt, a checkpoint written by "
                             f"RobotPredictionTrainer (keys joint_model, gripper_model); got {ckpt_path!r}")
        ckpt = torch.load(ckpt_path, map_location=self._device)
        self.joint_model.load_state_dict(ckpt["joint_model"])
        self.gripper_model.load_state_dict(ckpt["gripper_model"])

    def _schedule_prob(self):
        """Probability of feeding ground truth (trainer.py:132-140)."""
        k = self._config.scheduled_sampling_k
        use_truth = k / (k + np.exp(self._step / k))
        return [use_truth, 1 - use_truth]

    def _use_true_token(self):
        """Scheduled sampling coin (trainer.py:142-147)."""
        if not self._scheduled_sampling:
            return True
        return np.random.choice([True, False], p=self._schedule_prob())

    def _loss_kind(self):
        kind = self._config.reconstruction_loss
        if kind not in ops.LOSS_KINDS:
            raise NotImplementedError(f"{kind}")
        return ops.LOSS_KINDS[kind]

    def _recon_loss(self, prediction, target, mask=None, batch_weight=None):
        """trainer.py:149-161; returns the (3,) [loss, robot_mse, world_mse] tensor of the fused kernel."""
        cf = self._config
        rw = cf.robot_pixel_weight if "dontcare" in cf.reconstruction_loss else 0.0
        bw = batch_weight if cf.reconstruction_loss in ("l1", "dontcare_l1") else None
        return ops.ReconLoss.apply(prediction, target, mask, bw, self._loss_kind(), rw)

    def _mark(self, name):
        if self.phase_events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.phase_events.append((name, e))

    def _seed(self, value: float, n: int = 1, first_only: bool = False):
        key = (value, n, first_only)
        if key not in self._grad_seeds:
            t = torch.zeros(n, device=self._device)
            if first_only:
                t[0] = value
            else:
                t.fill_(value)
            self._grad_seeds[key] = t
        return self._grad_seeds[key]

    # ---------------------------------------------------------------- windows
    def _robot_windows(self):
        """Do this run's windows take their states and masks from `self.robot_model` (finetune_* experiments of a model
        that takes masks or robot states: trainer.py:294-319, 520-547, 1180-1202)?  Refuses such a run without one."""
        cf = self._config
        if not ("finetune" in cf.experiment and (cf.model_use_mask or cf.model_use_robot_state)):
            return False
        if getattr(self, "robot_model", None) is None:
            raise NotImplementedError(
                "finetune_* windows take their robot states and masks from an analytical / learned robot model: set "
                "`trainer.robot_model` to an object with predict_batch(batch) -> (states, masks[, heatmaps]) -- the "
                "reference's LocobotAnalyticalModel, robot_atlas.AtlasRobotModel or robot_model.LearnedRobotModel")
        return True

    def _window_batch(self, data, s, e, predicted_masks_key):
        """Frames [s, e) of a time-first video as the batch of one step.  Under `_robot_windows` the robot model's states,
        masks and (with `model_use_heatmap`) heatmaps replace the window's `states`, `predicted_masks_key` and `heatmaps`:
        training rolls out and scores on the predicted masks ("masks"); an evaluation rolls out on them ("pred_masks")
        and scores with the true ones, which stay in `masks`.  `qpos` and `folder` are the learned robot model's inputs
        and are carried whenever the video has them (views: no step reads them)."""
        cf = self._config
        batch = {"images": data["images"][s:e], "states": data["states"][s:e], "actions": data["actions"][s:e - 1],
                 "masks": data["masks"][s:e], "robot": data["robot"]}
        batch[predicted_masks_key] = batch["masks"]
        if "qpos" in data:
            batch["qpos"] = data["qpos"][s:e]
        if "folder" in data:  # the learned robot model renders each sample from its own viewpoint
            batch["folder"] = data["folder"]
        use_heatmap = getattr(cf, "model_use_heatmap", False)
        if use_heatmap:
            batch["heatmaps"] = data["heatmaps"][s:e]
        if self._robot_windows():
            if getattr(cf, "preprocess_action", "raw") != "raw":
                batch["raw_actions"], batch["raw_states"] = data["raw_actions"][s:e - 1], data["raw_states"][s:e]
                batch["raw_low"], batch["raw_high"] = data["raw_low"], data["raw_high"]
            batch["low"], batch["high"] = data["low"], data["high"]
            out = self.robot_model.predict_batch(batch)
            if use_heatmap:
                batch["states"], batch[predicted_masks_key], batch["heatmaps"] = out
            else:
                batch["states"], batch[predicted_masks_key] = out
        return batch

    # ------------------------------------------------------------- train step
    def _train_video(self, data):
        """Slice a video into n_past+n_future windows and train on each (trainer.py:259-324)."""
        cf = self._config
        x = data["images"]
        T = len(x)
        window = cf.n_past + cf.n_future
        self.steps_per_train_video = floor(T / window)
        all_losses = defaultdict(float)
        for i in range(floor(T / window)):
            if cf.random_snippet:
                s = self._video_sample_rng.randint(0, (T - window) + 1)
                e = s + window
            else:
                s, e = i * window, (i + 1) * window
            batch = self._window_batch(data, s, e, "masks")
            if cf.load_movement_info:
                batch["high_movement"] = data["high_movement"]
            losses = self._train_step(batch)
            for k, v in losses.items():
                all_losses[k] += v / floor(T / window)
        return all_losses

    def _model_step(self, i, x_j, masks, states, ac, heatmaps, skip, *, posterior, force_use_prior=False, dontcare):
        """`model_step` of this trainer's model and configuration."""
        return model_step(self.model, self._config, i, x_j, masks, states, ac, heatmaps, skip, posterior=posterior,
                          force_use_prior=force_use_prior, dontcare=dontcare)

    def _per_robot_losses(self, x_pred, x_i, m_i, robot_name, all_robots):
        """[(robot, its samples' (3,) [loss, robot_mse, world_mse])] of a batch that mixes robots: the per-robot logging
        metrics (trainer.py:442-452); nothing for a batch of one robot."""
        if len(all_robots) < 2:
            return []
        subs = []
        for r in all_robots:
            idx = torch.from_numpy(np.nonzero(robot_name == r)[0]).to(self._device)
            subs.append((r, ops.ReconLoss.apply(x_pred[idx].contiguous(), x_i[idx].contiguous(), m_i[idx].contiguous(),
                                                None, 0, 0.0)))
        return subs

    def _train_step(self, data, use_truth=None):
        """Forward and backward pass + optimiser step (trainer.py:326-465).  Returns the loss dict.
        `use_truth[i]` overrides the scheduled-sampling coin at time index i (parity tests)."""
        cf = self._config
        dev = self._device
        f32 = torch.float32
        det = cf.model == "det"  # trainer.py:383-384: no prior / posterior, no KL term, no heatmap input
        if cf.model == "copy":
            raise ValueError("--model copy has nothing to train (trainer.py:739-741: train() only evaluates it)")
        x = data["images"].to(dev, f32)
        states = data["states"].to(dev, f32)
        ac = data["actions"].to(dev, f32)
        mask = data["masks"].to(dev, f32)
        heatmaps = data["heatmaps"].to(dev, f32) if getattr(cf, "model_use_heatmap", False) and not det else None
        robot_name = np.array(data["robot"])
        all_robots = sorted(set(robot_name))
        batch_weight = None
        if cf.load_movement_info:
            mv = data["high_movement"].to(dev)
            batch_weight = (cf.movement_weight * mv).to(f32)
            batch_weight[~mv.bool()] = 1.0

        # (a sharded optimiser's parameter all-gather of the previous step is waited for inside the model: the encoder's
        # buckets before its first kernel, the rest behind the encoder's forward pass -- SVGConvModel._encode)
        ops.begin_step(x.device)
        self._mark("start")
        # (lazy: the large conv weights' gradients are written, not added to zeros, by their one launch per step)
        self.model.zero_grad(lazy=ops.LAZY_ZERO_GRAD)
        bs = min(cf.batch_size, x.shape[1])
        self.model.init_hidden(bs)
        dontcare = "dontcare" in cf.reconstruction_loss or cf.black_robot_input
        roots, seeds, log = [], [], []  # autograd roots, their incoming grads, (name, tensor, index) for the readback
        n_steps = cf.n_past + cf.n_future - 1

        def add_losses(x_pred, i, latents, kl_here=True):
            x_i, m_i = x[i], mask[i]
            rec = self._recon_loss(x_pred, x_i.contiguous(), m_i.contiguous(), batch_weight)
            roots.append(rec)
            seeds.append(self._seed(1.0, 3, first_only=True))
            log.extend([("recon_loss", rec, 0), ("robot_loss", rec, 1), ("world_loss", rec, 2)])
            with torch.no_grad():
                for r, sub in self._per_robot_losses(x_pred.detach(), x_i, m_i, robot_name, all_robots):
                    log.extend([(f"{r}_robot_loss", sub, 1), (f"{r}_world_loss", sub, 2)])
            if kl_here:
                add_kl(*latents)

        def add_kl(mu, logvar, mu_p, logvar_p):
            kl = ops.KLLoss.apply(mu, logvar, mu_p, logvar_p, bs)
            roots.append(kl)
            seeds.append(self._seed(float(cf.beta)))
            log.append(("kld", kl, 0))

        # scheduled-sampling coins of the window, drawn in the reference's order (nothing else uses np.random here)
        truths = [True] + [(self._use_true_token() if use_truth is None else bool(use_truth[i]))
                           for i in range(2, n_steps + 1)]
        H, W = x.shape[-2], x.shape[-1]
        sequence_taken = False
        # (the deterministic model always goes step by step: the time-batched window and the hand-scheduled core are SVG's)
        if SEQUENCE_PATH and not det and all(truths) and self.model.sequence_ok(bs, H, W) and x.shape[1] == bs:
            sequence_taken = True
            # every input frame is ground truth: encoder and decoder run once over the whole window
            T = n_steps
            m_all = torch.cat([mask[:T], mask[1:T + 1]], 2) if cf.model_use_future_mask else mask[:T]
            hm_all = None
            if heatmaps is not None:
                hm_all = torch.cat([heatmaps[:T], heatmaps[1:T + 1]], 2) if cf.model_use_future_heatmap else heatmaps[:T]
            robots = [((states[t], states[t + 1]) if cf.model_use_future_robot_state else states[t]) for t in range(T)]
            x4, mus, logvars, mu_ps, logvar_ps = self.model.forward_sequence_maps(
                x[:T], m_all, robots, hm_all, [ac[t] for t in range(T)], [states[t + 1] for t in range(T)],
                mask[:T] if dontcare else None)
            x_pred_all = ops.Composite.apply(x4, x[:T].reshape((T * bs,) + tuple(x.shape[2:])).contiguous())
            x_preds = x_pred_all.view((T, bs) + tuple(x_pred_all.shape[1:])).unbind(0)
            batched = self.model.sequence_batched
            if batched is not None and len(all_robots) == 1:
                # sum_t recon_t = sum_t mean_b f(t, b) = T * mean over ALL T*B samples: one launch over the window (every
                # loss kind normalises per sample, losses.py:11-50), seeded with T; the logged terms are scaled back
                bw_all = None if batch_weight is None else batch_weight.repeat(T)
                flatw = lambda t_: t_[1:T + 1].reshape((T * bs,) + tuple(t_.shape[2:])).contiguous()
                rec = self._recon_loss(x_pred_all, flatw(x), flatw(mask), bw_all)
                roots.append(rec)
                seeds.append(self._seed(float(T), 3, first_only=True))
                log.extend([("recon_loss", rec, 0, T), ("robot_loss", rec, 1, T), ("world_loss", rec, 2, T)])
            else:
                for t in range(T):
                    add_losses(x_preds[t], t + 1, (mus[t], logvars[t], mu_ps[t], logvar_ps[t]), kl_here=batched is None)
            if batched is not None:
                # sum_t KL_t: every term is a sum over its elements / bs (losses.py:97-106), so the window's KL is ONE
                # launch over all T*B samples' elements (and one backward launch writing the batched gradients)
                add_kl(*batched)
        else:
            x_pred = None
            skip = None
            for i in range(1, n_steps + 1):
                x_j = x[i - 1] if truths[i - 1] else x_pred  # scheduled sampling: gradients flow through the fed-back frame
                x4, skip, latents = self._model_step(i, x_j, mask, states, ac, heatmaps, skip, posterior=True,
                                                     dontcare=dontcare)
                x_pred = ops.Composite.apply(x4, x_j.contiguous())  # un-blacked x_j (trainer.py:406-407)
                add_losses(x_pred, i, latents, kl_here=not det)
        # the step's loss scalars are final once the forward pass is enqueued: start their device->host copy now (into
        # pinned memory) and collect it after the optimiser step is enqueued, so that the host never waits for the
        # backward pass or Adam (the reference likewise reads its losses before loss.backward(), trainer.py:433-458)
        self._mark("forward")
        with torch.no_grad():
            vals_dev = torch.stack([e[1].detach()[e[2]] for e in log])
        if self._loss_host is None or self._loss_host.numel() < vals_dev.numel():
            self._loss_host = torch.empty(max(64, vals_dev.numel()), dtype=vals_dev.dtype).pin_memory()
        vals_host = self._loss_host[:vals_dev.numel()]
        vals_host.copy_(vals_dev, non_blocking=True)
        copied = torch.cuda.Event()
        copied.record()
        # loss = sum_t recon_t + beta * sum_t kl_t (trainer.py:459): seed each term's gradient directly
        reducer = None
        if _dist_on():
            if isinstance(self.optimizer, ShardedAdam):
                reducer = ShardReducer(self.model.flat_parameters()[1], *self.optimizer.plan())
            else:
                reducer = GradReducer(self.model.flat_parameters()[1], getattr(cf, "ddp_bucket_mb", 64))
        # ConvLSTM weight gradients: one time-batched launch per weight, each followed by its slice's all-reduce.  In a window
        # that went step by step (scheduled sampling, GroupNorm cells) a weight's launch starts -- on the side stream -- the
        # moment its last step's operands exist (the backward pass reaches the window's first step last), under the rest of
        # that step's backward pass; the hand-scheduled core launches its chains' gradients itself
        stepped = not (sequence_taken and self.model.used_recurrent_core)
        try:
            with ops.deferred_wgrad(on_ready=reducer.ready if reducer is not None else None,
                                    flush_after=n_steps if stepped else None,
                                    vgg_steps=not sequence_taken):
                torch.autograd.backward(roots, seeds)
                self._mark("backward")
        finally:
            # a weight no launch wrote this step (none in the standard configurations) gets its zeros now -- also when
            # backward raised: a caller that catches the exception must not find last step's values in a .grad
            ops.finish_grads()
        self._mark("weight_grads")
        if reducer is not None:
            reducer.finish()
            self._mark("allreduce_exposed")
        self.optimizer.step()
        self._mark("adam")
        if not det:
            self.model.sequence_batched = None  # (graph references of this step)

        copied.synchronize()  # the one host wait of the step (normally already satisfied)
        vals = vals_host.tolist()
        losses = defaultdict(float)
        for e, v in zip(log, vals):
            losses[e[0]] += v * (e[3] if len(e) > 3 else 1)
        for k in losses:
            losses[k] = losses[k] / cf.n_future
        return losses

    # ------------------------------------------------------------------- eval
    def _compute_epoch_metrics(self, data_loader, name):
        """Average the per-video eval metrics over a loader (trainer.py:467-488)."""
        from .data import process_batch
        losses = defaultdict(list)
        for data in data_loader:
            data = process_batch(data, self._device)
            info = self._eval_video(data, autoregressive=True)
            for k, v in info.items():
                losses[k].append(v)
        return {f"{name}/{k}": float(np.mean(v)) for k, v in losses.items()}

    def _eval_video(self, data, autoregressive=False):
        """Evaluate a whole video in n_eval windows (trainer.py:490-564); ground-truth masks drive the rollout.

        `--eval_best_of_three True` (this repository's flag, default off): an autoregressive evaluation of `--model svg`
        under a `finetune*` experiment draws three prior samples per window, as the reference always does
        (trainer.py:497-499), and returns the sample whose summed `autoreg_psnr` is largest (trainer.py:558-559; a
        stable sort: ties keep the earlier sample); its index is left in `self.last_best_eval_sample`.  The robot model
        is asked once per window.  The three samples of a window run as one batch of 3 B videos
        (`RAC_PREDICT_BATCH_SAMPLES=0`: one after the other through the same scoring code), see `_eval_step`."""
        cf = self._config
        num_samples = 3 if (getattr(cf, "eval_best_of_three", False) and autoregressive and cf.model == "svg"
                            and "finetune" in cf.experiment) else 1
        self.last_best_eval_sample = 0
        batched = os.environ.get("RAC_PREDICT_BATCH_SAMPLES", "1") == "1"
        sampled = [defaultdict(float) for _ in range(num_samples)]
        self._robot_windows()  # (a finetune_* run without a robot model is refused before its first window)
        T = len(data["images"])
        window = cf.n_eval
        total = defaultdict(float)
        for i in range(floor(T / window)):
            batch = self._window_batch(data, i * window, (i + 1) * window, "pred_masks")
            if num_samples == 1:
                for k, v in self._eval_step(batch, autoregressive).items():
                    total[k] += v
                continue
            if batched:
                outs = self._eval_step(batch, autoregressive, num_samples=num_samples)
            else:
                outs = [self._eval_step(batch, autoregressive, num_samples=1)[0] for _ in range(num_samples)]
            for sample, losses in zip(sampled, outs):
                for k, v in losses.items():
                    sample[k] += v
        if num_samples > 1:
            self.last_best_eval_sample = self._best_eval_sample(sampled, autoregressive and cf.model == "svg")
            total = sampled[self.last_best_eval_sample]
        for k in total:
            total[k] /= floor(T / window)
        return total

    @staticmethod
    def _best_eval_sample(sampled, by_psnr=True):
        """Index of the sample `_eval_video` reports (trainer.py:558-560): the largest summed `autoreg_psnr`, ties to the
        earlier sample (`list.sort(reverse=True)` is stable); the first sample where nothing is sorted."""
        order = list(range(len(sampled)))
        if by_psnr:
            order.sort(key=lambda n: sampled[n]["autoreg_psnr"], reverse=True)
        return order[0]

    def _snippet(self, data, autoregressive, S=1):
        """An n_eval snippet on the device, ready for a prior-driven rollout of S samples as ONE batch of S B videos:
        the recurrent states are reset for S B videos and the rollout's inputs (`states`, `ac`, `masks`: the batch's
        `pred_masks`, `heatmaps`) repeated per sample group, group s in rows [s B, (s+1) B); the frames `x` and the
        scoring masks `true_masks` stay (B, ...), `frame_in(i)` is frame i for all groups."""
        cf = self._config
        dev, f32 = self._device, torch.float32
        svg = cf.model == "svg"  # det (trainer.py:628-629) and copy (:606-607) have no prior: no KL term, no heatmap
        if S > 1 and not svg:
            raise ValueError("only --model svg draws samples")
        sn = SimpleNamespace(svg=svg, prefix="autoreg" if autoregressive else "1step",
                             dontcare="dontcare" in cf.reconstruction_loss or cf.black_robot_input)
        sn.x = x = data["images"].to(dev, f32)
        sn.states = data["states"].to(dev, f32)
        sn.ac = data["actions"].to(dev, f32)
        sn.true_masks = data["masks"].to(dev, f32)
        sn.masks = data["pred_masks"].to(dev, f32)
        sn.heatmaps = data["heatmaps"].to(dev, f32) if getattr(cf, "model_use_heatmap", False) and svg else None
        sn.robot_name = np.array(data["robot"])
        sn.all_robots = sorted(set(sn.robot_name))
        sn.bs = min(cf.test_batch_size, x.shape[1])
        self.model.init_hidden(S * sn.bs)
        if S > 1:
            rep = lambda t: t.repeat((1, S) + (1,) * (t.dim() - 2))
            sn.states, sn.ac, sn.masks = rep(sn.states), rep(sn.ac), rep(sn.masks)
            sn.heatmaps = rep(sn.heatmaps) if sn.heatmaps is not None else None
        sn.frame_in = lambda i: x[i] if S == 1 else x[i].repeat(S, 1, 1, 1)
        return sn

    def _prior_rollout(self, sn, autoregressive, composite=None):
        """Roll the snippet `sn` (`_snippet`) out on the prior (`force_use_prior`; the posterior runs for the KL term):
        frame i is predicted from frame i - 1, or from the prediction of it when `autoregressive`.
        `composite(i, x4, x_j, x_i, true_mask_i)` makes the frame from the decoder's output (None: `ops.Composite` over
        the frame fed in).  `--model copy` has no model
        step and nothing to composite: its frame is the one fed in, on the rollout's masks (`pred_masks`).
        Yields (i, x_pred (S B, 3, H, W), latents or None, x[i], true_masks[i]) per step, for the caller to score."""
        cf = self._config
        x_pred = skip = None
        for i in range(1, cf.n_eval):
            x_j = x_pred if (autoregressive and i > 1) else sn.frame_in(i - 1)
            x_i, tm = sn.x[i].contiguous(), sn.true_masks[i].contiguous()
            if cf.model == "copy":
                x_pred, latents = self.model(x_j, sn.masks[i - 1], x_i, sn.masks[i]), None
            else:
                x4, skip, latents = self._model_step(i, x_j, sn.masks, sn.states, sn.ac, sn.heatmaps, skip,
                                                     posterior=True, force_use_prior=True, dontcare=sn.dontcare)
                x_pred = composite(i, x4, x_j, x_i, tm) if composite else ops.Composite.apply(x4, x_j.contiguous())
            yield i, x_pred, latents, x_i, tm

    @torch.no_grad()
    def _eval_step(self, data, autoregressive=False, num_samples=None):
        """Evaluate one n_eval snippet (trainer.py:566-734): prior-driven prediction (`force_use_prior`), optional
        autoregressive feeding, recon / robot / world losses, PSNR, SSIM, KL.  One host sync at the end.

        `num_samples` = S (the sampled evaluation of `_eval_video`; None: the path above, untouched) rolls S prior
        samples of the snippet as ONE batch of S B videos, as `_predict_video` does (inputs repeated per sample group,
        `model.eps_source` asked for (S B, z, h, w) per draw, sample s in rows [s B, (s+1) B)), scores each predicted
        frame with ONE `ops.eval_frames` launch into a (n_eval - 1, S B, 8) table, takes the KL per group on slices,
        and returns a list of S loss dicts with this method's keys.  Every scalar is an elementwise function of a
        video's table rows followed by sums in a fixed order, so a sample's numbers do not depend on S."""
        if num_samples is not None:
            return self._eval_step_sampled(data, autoregressive, int(num_samples))
        from .metrics import masked_psnr_ssim
        cf = self._config
        sn = self._snippet(data, autoregressive)
        prefix = sn.prefix
        log, klog = [], []
        for i, x_pred, latents, x_i, tm in self._prior_rollout(sn, autoregressive):
            rec = self._recon_loss(x_pred, x_i, tm)
            log += [(f"{prefix}_recon_loss", rec[0]), (f"{prefix}_robot_loss", rec[1]), (f"{prefix}_world_loss", rec[2])]
            p, s = masked_psnr_ssim(x_pred, x_i, tm)  # robot region blacked with the true mask
            p = p.mean()
            log += [(f"{prefix}_psnr", p), (f"{prefix}_ssim", s)]
            if autoregressive:
                klog += [(f"{i}_step_psnr", p), (f"{i}_step_ssim", s), (f"{i}_step_world_loss", rec[2])]
            for r, sub in self._per_robot_losses(x_pred, x_i, tm, sn.robot_name, sn.all_robots):
                log += [(f"{prefix}_{r}_robot_loss", sub[1]), (f"{prefix}_{r}_world_loss", sub[2])]
            if sn.svg:
                kl = ops.KLLoss.apply(*latents, sn.bs)
                log.append((f"{prefix}_kld", kl[0]))
        vals = torch.stack([t.reshape(()) for _, t in log + klog]).cpu().tolist()
        losses = defaultdict(float)
        for (name, _), v in zip(log, vals[:len(log)]):
            losses[name] += v
        for k in losses:
            losses[k] = losses[k] / (cf.n_eval - 1)
        for (name, _), v in zip(klog, vals[len(log):]):
            losses[name] = v
        return losses

    @torch.no_grad()
    def _eval_step_sampled(self, data, autoregressive, S):
        """`_eval_step(num_samples=S)`: the rollout of `_eval_step` on S B videos, one `ops.eval_frames` launch per frame."""
        from .metrics import table_scalars
        cf = self._config
        if cf.model != "svg":
            raise ValueError("only --model svg draws samples")
        sn = self._snippet(data, autoregressive, S)
        bs, prefix, robot_name, all_robots = sn.bs, sn.prefix, sn.robot_name, sn.all_robots
        n_steps = cf.n_eval - 1
        H, W = sn.x.shape[-2], sn.x.shape[-1]
        kind = self._loss_kind()
        rw = cf.robot_pixel_weight if "dontcare" in cf.reconstruction_loss else 0.0
        table = torch.empty((n_steps, S * bs, 8), device=self._device, dtype=torch.float32)
        kls = []
        for i, x_pred, (mu, logvar, mu_p, logvar_p), x_i, tm in self._prior_rollout(sn, autoregressive):
            # robot region blacked with, and the errors split by, the true mask
            ops.eval_frames(x_pred, x_i, tm, kind, rw, S, out=table[i - 1])
            for n in range(S):
                sl = slice(n * bs, (n + 1) * bs)
                kls.append(ops.KLLoss.apply(mu[sl], logvar[sl], mu_p[sl], logvar_p[sl], bs)[0])
        groups = table.view(n_steps, S, bs, 8)
        scal = table_scalars(groups, kind, 3 * H * W)
        names = [f"{prefix}_{k}" for k in ("recon_loss", "robot_loss", "world_loss", "psnr", "ssim")]
        cols = [scal[k] for k in ("recon_loss", "robot_loss", "world_loss", "psnr", "ssim")]
        if len(all_robots) > 1:
            for r in all_robots:
                sub = table_scalars(groups, kind, 3 * H * W, index=np.nonzero(robot_name == r)[0])
                names += [f"{prefix}_{r}_robot_loss", f"{prefix}_{r}_world_loss"]
                cols += [sub["robot_loss"], sub["world_loss"]]
        names.append(f"{prefix}_kld")
        cols.append(torch.stack(kls).view(n_steps, S))
        vals = torch.stack(cols).cpu().tolist()  # [key][step][sample]: the one host sync
        outs = []
        for n in range(S):
            losses = defaultdict(float)
            for name, per_step in zip(names, vals):
                for step in per_step:
                    losses[name] += step[n]
                losses[name] = losses[name] / n_steps
            if autoregressive:
                for i in range(1, cf.n_eval):
                    for key, col in (("psnr", 3), ("ssim", 4), ("world_loss", 2)):
                        losses[f"{i}_step_{key}"] = vals[col][i - 1][n]
            outs.append(losses)
        return outs

    # ------------------------------------------------------------ video export
    def predict_video(self, data):
        """Generate the predicted and the ground-truth videos of a batch for an FVD computation (trainer.py:1149-1224):
        windows of n_eval frames, each rolled out autoregressively on the prior (`_predict_video`).  Returns the scalar
        metrics averaged over the windows plus `gen_imgs` / `true_imgs`: lists with one uint8 (B, n_eval-1, H, W, 3)
        array per window, the robot region blacked with the true mask.  `--model svg` under a `finetune*` experiment
        draws three prior samples per window and returns the sample whose summed `autoreg_world_loss` is smallest (a
        stable sort: ties keep the earlier sample); its index is left in `self.last_best_sample`.

        The three samples of a window run as ONE batch of 3 B videos (`RAC_PREDICT_BATCH_SAMPLES=0`: one after the
        other, as the reference does).  The frozen path's arithmetic does not depend on what shares a video's batch, so
        both orders give the same frames; `model.eps_source` is asked for (3 B, z, h, w) per draw, sample s in rows
        [s B, (s+1) B).  Without an `eps_source` one `torch.randn` of that shape is drawn: the same distribution, but
        not the random stream three sequential passes would consume.

        finetune_* windows take their states and masks from `trainer.robot_model` under the condition `_eval_video`
        uses (the model takes masks or robot states).  The reference calls the robot model unconditionally under
        `finetune*`; the two differ only where the reference itself fails (a model without either input has no use for
        `pred_masks`, and `out` stays unbound for experiments other than finetune_locobot without a learned model)."""
        cf = self._config
        num_samples = 3 if (cf.model == "svg" and "finetune" in cf.experiment) else 1
        self._robot_windows()  # (a finetune_* run without a robot model is refused before its first window)
        batched = num_samples > 1 and os.environ.get("RAC_PREDICT_BATCH_SAMPLES", "1") == "1"
        T = len(data["images"])
        window = cf.n_eval
        sampled = [defaultdict(float) for _ in range(num_samples)]
        for i in range(floor(T / window)):
            # predicted states / masks drive the rollout, the true masks score and black the frames (trainer.py:1180-1202)
            batch = self._window_batch(data, i * window, (i + 1) * window, "pred_masks")
            if batched:
                outs = self._predict_video(batch, num_samples=num_samples)
            else:
                outs = [self._predict_video(batch) for _ in range(num_samples)]
            for sample, losses in zip(sampled, outs):
                for k, v in losses.items():
                    if k in ("true_imgs", "gen_imgs"):
                        if k not in sample:
                            sample[k] = []
                        sample[k].append(v)
                    else:
                        sample[k] += v
        order = list(range(num_samples))
        if cf.model == "svg":  # the best sample by world error (trainer.py:1216-1218; list.sort is stable)
            order.sort(key=lambda n: sampled[n]["autoreg_world_loss"])
        self.last_best_sample = order[0]
        best = sampled[order[0]]
        for k in best:
            if k not in ("true_imgs", "gen_imgs"):
                best[k] /= floor(T / window)
        return best

    @torch.no_grad()
    def _predict_video(self, data, autoregressive=True, num_samples=1):
        """Roll one n_eval snippet out on the prior and return its metrics and its frames (trainer.py:1227-1408): the
        loss keys of `_eval_step`, averaged over the n_eval - 1 predicted frames, the k-step keys as the reference's
        `_predict_video` defines them (which is not how `_eval_step` does), and `gen_imgs` / `true_imgs`, uint8
        (B, n_eval-1, H, W, 3), robot region blacked with the true mask.

        Per step ONE launch (`ops.predict_frames`) composites the decoder's output and writes both uint8 frames into the
        device-side video buffer; the call ends in one device->host copy of that buffer and one of the stacked scalars.

        `num_samples` = S > 1 rolls S prior samples of the snippet as one batch of S B videos (inputs repeated per
        sample group, metrics per group on contiguous slices, the true frames written once) and returns a list of S
        dicts that share one `true_imgs` array."""
        from .metrics import masked_psnr_ssim
        cf = self._config
        S = int(num_samples)
        sn = self._snippet(data, autoregressive, S)
        bs, prefix = sn.bs, sn.prefix
        n_steps = cf.n_eval - 1
        H, W = sn.x.shape[-2], sn.x.shape[-1]
        # gen frames of the S groups, then the true frames: one buffer, one copy to the host
        frames = torch.empty(((S + 1) * bs, n_steps, H, W, 3), device=self._device, dtype=torch.uint8)
        gen_u8, true_u8 = frames[:S * bs], frames[S * bs:]
        log, klog = [], []  # (sample, name, scalar tensor); (sample, step, psnr, ssim, world_mse)
        composite = lambda i, x4, x_j, x_i, tm: ops.predict_frames(x4, x_j, x_i, tm, gen_u8, true_u8, i - 1)
        for i, x_pred, latents, x_i, tm in self._prior_rollout(sn, autoregressive, composite):
            if cf.model == "copy":  # a finished frame: only the uint8 frames are written
                ops.predict_frames(None, None, x_i, tm, gen_u8, true_u8, i - 1, pred=x_pred)
            for n in range(S):
                sl = slice(n * bs, (n + 1) * bs)
                xp = x_pred[sl]
                rec = self._recon_loss(xp, x_i, tm)
                log += [(n, f"{prefix}_recon_loss", rec[0]), (n, f"{prefix}_robot_loss", rec[1]),
                        (n, f"{prefix}_world_loss", rec[2])]
                p, s = masked_psnr_ssim(xp, x_i, tm)  # robot region blacked with the true mask
                p = p.mean()
                log += [(n, f"{prefix}_psnr", p), (n, f"{prefix}_ssim", s)]
                if autoregressive:
                    klog.append((n, i, p, s, rec[2]))
                for r, sub in self._per_robot_losses(xp, x_i, tm, sn.robot_name, sn.all_robots):
                    log += [(n, f"{prefix}_{r}_robot_loss", sub[1]), (n, f"{prefix}_{r}_world_loss", sub[2])]
                if sn.svg:
                    kl = ops.KLLoss.apply(*(t[sl] for t in latents), bs)
                    log.append((n, f"{prefix}_kld", kl[0]))
        scalars = [t for _, _, t in log] + [t for e in klog for t in e[2:]]
        vals = torch.stack([t.reshape(()) for t in scalars]).cpu().tolist()
        host = frames.cpu().numpy()
        outs = self._video_scalars([(n, name) for n, name, _ in log], vals[:len(log)], [(n, i) for n, i, *_ in klog],
                                   vals[len(log):], n_steps, S)
        for n, losses in enumerate(outs):
            losses["gen_imgs"] = host[n * bs:(n + 1) * bs]
            losses["true_imgs"] = host[S * bs:]
        return outs[0] if S == 1 else outs

    @staticmethod
    def _video_scalars(log, vals, klog, kvals, n_steps, num_samples=1):
        """The host half of `_predict_video`'s metrics (trainer.py:1386-1393): `log[j]` = (sample, key) of the per-step
        scalar `vals[j]`, `klog[j]` = (sample, step i) of the (psnr, ssim, world_mse) triple `kvals[3j:3j+3]`.
        Returns one loss dict per sample."""
        outs = [defaultdict(float) for _ in range(num_samples)]
        for (n, name), v in zip(log, vals):
            outs[n][name] += v
        for losses in outs:
            for k in losses:
                losses[k] = losses[k] / n_steps  # don't count the first step
        # k-step keys (trainer.py:1362-1367): step i's values are added to every k in [i, n_eval - 1)
        k_losses = [defaultdict(float) for _ in range(num_samples)]
        for j, (n, i) in enumerate(klog):
            p, s, w = kvals[3 * j:3 * j + 3]
            for k in range(i, n_steps):
                k_losses[n][f"{k}_step_psnr"] += p
                k_losses[n][f"{k}_step_ssim"] += s
                k_losses[n][f"{k}_step_world_loss"] += w
        for n, losses in enumerate(outs):
            for key, v in k_losses[n].items():
                # the reference divides by the key's FIRST CHARACTER (trainer.py:1391), kept verbatim: that is k only
                # for k <= 9 ("12_step_psnr" is divided by 1)
                losses[key] = v / float(key[0])
        return outs

    # ------------------------------------------------------------------- plots
    @torch.no_grad()
    def plot(self, data, epoch, name, random_start=True, instance=None):
        """GIF of prior-driven autoregressive generations next to the ground truth (trainer.py:949-1147): per video one
        row [ground truth | 3 samples], one GIF frame per time step, written to `<plot_dir>/<name>_<epoch>.gif`.
        `data`: a time-first batch.  Returns the file name."""
        from PIL import Image
        cf = self._config
        if cf.model != "svg":
            raise NotImplementedError(f"plot() draws the svg model's prior samples; GIFs of --model {cf.model} are not built")
        dev, f32 = self._device, torch.float32
        b = min(data["images"].shape[1], 25)
        length = cf.n_past + cf.n_future if name in ("comparison", "train") else cf.n_eval
        total = data["images"].shape[0]
        starts = (self._plot_rng.randint(0, total - length + 1, size=b) if random_start else np.zeros(b, dtype=np.int64))

        def clip(key, shorten=0):  # every video's own [start, start + length) window, batch truncated to b
            t = data[key]
            return torch.stack([t[s:s + length - shorten, i] for i, s in enumerate(starts)], 1).to(dev, f32)
        x, states, ac, mask = clip("images"), clip("states"), clip("actions", 1), clip("masks")
        heatmaps = clip("heatmaps") if getattr(cf, "model_use_heatmap", False) else None
        if "finetune" in cf.experiment and (cf.model_use_mask or cf.model_use_robot_state):
            if getattr(self, "robot_model", None) is None:
                raise NotImplementedError("finetune_* plots roll out on trainer.robot_model's states and masks")
            batch = {"states": states, "actions": ac, "masks": mask, "qpos": clip("qpos"), "low": data["low"][:b],
                     "high": data["high"][:b]}
            if getattr(cf, "preprocess_action", "raw") != "raw":
                batch.update(raw_low=data["raw_low"][:b], raw_high=data["raw_high"][:b],
                             raw_actions=clip("raw_actions", 1), raw_states=clip("raw_states"))
            states, mask = self.robot_model.predict_batch(batch)[:2]
        dontcare = "dontcare" in cf.reconstruction_loss or cf.black_robot_input
        was_training = self.model.training
        self.model.eval()
        samples = []
        for _ in range(3):  # nsample of the svg model
            self.model.init_hidden(b)
            x_j = x[0]
            frames = [ops.ZeroRegion.apply(x_j.contiguous(), mask[0].contiguous()) if dontcare else x_j]
            skip = None
            for i in range(1, length):
                x4, skip, _ = self._model_step(i, x_j, mask, states, ac, heatmaps, skip, posterior=False,
                                               dontcare=dontcare)
                x_pred = ops.Composite.apply(x4, x_j.contiguous())
                x_j = x[i] if i < cf.n_past else x_pred
                frames.append(ops.ZeroRegion.apply(x_pred, mask[i].contiguous()) if dontcare else x_j)
            samples.append(torch.stack(frames))  # (length, b, 3, H, W)
        self.model.train(was_training)
        # one GIF frame per time step: b rows of [ground truth | sample 0 | sample 1 | sample 2]
        grid = torch.stack([x] + samples, 2)                      # (length, b, 4, 3, H, W)
        grid = grid.permute(0, 1, 4, 2, 5, 3).reshape(length, b * x.shape[-2], 4 * x.shape[-1], 3)
        imgs = [Image.fromarray(f) for f in (grid.clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()]
        plot_dir = getattr(cf, "plot_dir", None) or os.path.join(cf.log_dir, "plot")
        os.makedirs(plot_dir, exist_ok=True)
        stem = f"{name}_{epoch}" if instance is None else f"{name}_ep{epoch}_{instance}"
        fname = os.path.join(plot_dir, stem + ".gif")
        imgs[0].save(fname, save_all=True, append_images=imgs[1:], duration=250, loop=0)
        if self._wandb is not None:
            self._wandb.log({f"{name}/gifs": self._wandb.Video(fname, format="gif")}, step=self._step)
        return fname

    # ----------------------------------------------------------- outer loops
    def train(self, batch_generator=None, test_hook=None, test_loader=None, transfer_loader=None):
        """Epoch loop with checkpoint and evaluation cadence (trainer.py:736-792).  `batch_generator` yields time-first
        batches in the layout of `process_batch` (robonet_dataset.py:434-451); by default the loaders come from
        `_setup_data`.  Every `eval_interval` epochs the model is evaluated on the test loader
        (`_compute_epoch_metrics`, keys `test/*`) and, for `--experiment train_robonet` with locobot data under the data
        root, on the zero-shot transfer loader (`transfer/*`) as the reference does; with `--plot True` (this repo's
        switch, default off) a GIF of generations is written per epoch / evaluation (`plot`)."""
        cf = self._config
        if cf.model == "copy":
            return self.train_copy_baseline(test_loader=test_loader, transfer_loader=transfer_loader)
        self._step = self._load_checkpoint(cf.dynamics_model_ckpt)
        # this loop owns every reader of the parameters between two steps (forward passes and checkpoints, which wait):
        # the optimiser may finish the large weights' update under the next step's encoder (optim.FusedAdam)
        if os.environ.get("RAC_ADAM_OVERLAP", "1") == "1" and isinstance(self.optimizer, FusedAdam):
            self.optimizer.overlap_next_forward = True
        if batch_generator is None:
            batch_generator, test_loader = self._setup_data()
            transfer_loader = transfer_loader or getattr(self, "transfer_loader", None)
        plots = bool(getattr(cf, "plot", False)) and cf.model == "svg" and (not _dist_on() or dist.get_rank() == 0)

        def evaluate(loader, name, epoch):
            from .data import process_batch
            info_ = self._compute_epoch_metrics(loader, name)
            self.eval_history.append((epoch, info_))
            if self._wandb is not None:
                self._wandb.log(info_, step=self._step)
            if plots:
                self.plot(process_batch(next(iter(loader)), self._device), epoch, name)
        gen = batch_generator
        info = {}
        self.eval_history = []
        for epoch in range(cf.niter):
            self.model.train()
            for _ in range(cf.epoch_size):
                data = next(gen)
                info = self._train_video(data)
                if self._scheduled_sampling:
                    info["sample_schedule"] = self._schedule_prob()[0]
                self._step += self.steps_per_train_video
                if plots and _ == cf.epoch_size - 1:
                    self.plot(data, epoch, "train")
                if self._wandb is not None:
                    self._wandb.log({f"train/{k}": v for k, v in info.items()}, step=self._step)
            if epoch % cf.checkpoint_interval == 0 and epoch > 0:
                self._save_checkpoint()
            if epoch % cf.eval_interval == 0:
                self.model.eval()
                if test_loader is not None:
                    evaluate(test_loader, "test", epoch)
                if transfer_loader is not None:
                    evaluate(transfer_loader, "transfer", epoch)
                if test_hook is not None:
                    test_hook(self, epoch)
        self._save_checkpoint()
        # nothing of this loop's optimiser stays installed behind it (ops.PARAM_GATE is process-global: it would pin the
        # trainer's 4 GB and be asked about the next model's parameters)
        self.optimizer.wait_params()
        ops.release_gate(self.optimizer)
        return info

    def train_copy_baseline(self, train_loader=None, test_loader=None, transfer_loader=None):
        """Metrics of the copy baseline over the train and test sets (trainer.py:794-827), and over a transfer loader: the
        one the caller hands in, else the experiment's own for `--experiment train_sawyer_multiview` (the only one the
        reference walks here).  Nothing is trained or saved.  With --wandb every set is logged at steps 0 and 500000 (a
        horizontal line next to the trained models' curves).  Returns the metrics."""
        cf = self._config
        self._step = 0  # (trainer.py:798 loads a checkpoint's step; a model without parameters has none)
        if train_loader is None and test_loader is None:
            if cf.data_root == "synthetic":
                _, test_loader = self._setup_data()  # (the synthetic training stream has no end: the test set only)
            else:
                from . import data as D
                # (the loaders themselves: no device prefetch thread.  The reference walks a transfer set of its own for
                # train_sawyer_multiview only, trainer.py:818-825)
                walk_transfer = cf.experiment == "train_sawyer_multiview" and transfer_loader is None
                train_loader, test_loader, own_transfer = D.experiment_loaders(cf, transfer=walk_transfer)
                transfer_loader = own_transfer if walk_transfer else transfer_loader
        info = {}
        self.eval_history = []
        for loader, name, training in ((train_loader, "train", True), (test_loader, "test", False),
                                       (transfer_loader, "transfer", False)):
            if loader is None:
                continue
            self.model.train(training)
            part = self._compute_epoch_metrics(loader, name)
            self.eval_history.append((0, part))
            info.update(part)
        if self._wandb is not None:
            for step in (0, 500000):
                self._wandb.log(info, step=step)
        return info

    def _setup_data(self):
        """(infinite time-first batch generator, test loader).  `--data_root synthetic` feeds the deterministic
        generator of robot_aware_control_amd.synthetic; anything else goes through this package's RoboNet data path
        (data.py: the files, split and preprocessing of the experiment's own loaders in the reference, device
        prefetch)."""
        cf = self._config
        from . import data as D
        rank = dist.get_rank() if _dist_on() else 0
        if cf.data_root == "synthetic":
            from .synthetic import synth_video

            def gen():
                seed = cf.seed + 1000003 * rank  # every data-parallel rank trains on its own videos
                while True:
                    seed += 1
                    yield synth_video(seed, cf.video_length, cf.batch_size, cf.image_height, cf.image_width,
                                      cf.robot_dim, cf.action_dim)
            n_eval = getattr(cf, "n_eval", cf.n_past + cf.n_future)
            test = torch.utils.data.DataLoader(
                D.SyntheticVideoDataset(2 * getattr(cf, "test_batch_size", cf.batch_size), max(n_eval, cf.video_length),
                                        cf.image_height, cf.image_width, cf.robot_dim, cf.action_dim, seed=cf.seed + 7),
                batch_size=getattr(cf, "test_batch_size", cf.batch_size))
            return gen(), test
        # each --experiment's own split (trainer.py:899-947); a transfer loader measures zero-shot performance: on the
        # unseen locobot for train_robonet, on the unseen sawyer viewpoint for train_sawyer_multiview
        train_loader, test_loader, transfer_loader = D.experiment_loaders(cf)
        if transfer_loader is not None:
            self.transfer_loader = transfer_loader
        return D.get_batch(train_loader, self._device), test_loader

    def _save_checkpoint(self):
        """trainer.py:829-837.  Rank 0 writes the file; with the sharded optimiser EVERY rank first joins the collectives
        that assemble the full Adam moments (ShardedAdam.state_dict: all-gathers) and waits for the parameter all-gather of
        the last step, so that the parameters rank 0 clones are the updated ones."""
        opt_sd = None
        self.optimizer.wait_params()  # (parameters whose update is still in flight: FusedAdam's late group, an all-gather)
        if isinstance(self.optimizer, ShardedAdam):
            opt_sd = self.optimizer.state_dict()  # collective: before the rank check
        if _dist_on() and dist.get_rank() != 0:
            return
        os.makedirs(self._config.log_dir, exist_ok=True)
        path = os.path.join(self._config.log_dir, f"ckpt_{self._step}.pt")
        sd = {k: v.detach().clone().contiguous() if v.dim() != 4 else v.detach().clone()
              for k, v in self.model.state_dict().items()}
        if opt_sd is None:
            opt_sd = self.optimizer.state_dict()
        torch.save({"model": sd, "optimizer": opt_sd, "step": self._step}, path)
        return path

    def _load_checkpoint(self, ckpt_path=None):
        """Load a given checkpoint, else the newest ckpt_*.pt of log_dir (trainer.py:846-897)."""
        cf = self._config
        if ckpt_path is None:
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
            finetune_reset = False
        else:
            finetune_reset = "finetune" in cf.experiment
        ckpt = torch.load(ckpt_path, map_location=self._device)
        self.model.load_state_dict(ckpt["model"])
        if finetune_reset:
            return 0
        self.optimizer.load_state_dict(ckpt["optimizer"])
        return ckpt["step"]
