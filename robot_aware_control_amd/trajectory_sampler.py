"""TrajectorySampler: batched candidate rollouts through the frozen SVG model, on the GPU
(API of reference src/cem/trajectory_sampler.py:15-199).

Per (batch, step) the reference runs model.forward, two elementwise passes, a cost reduction and a
device->host copy (70 syncs per CEM iteration at N=1000).  Here the step tail -- compositing,
zero_robot_region, the image cost and its fp64 accumulation -- is one kernel and the per-candidate
sums stay on the device until the end: one D2H per call.  With `ret_obs` (the planner's --debug_cem) the step tail
writes every candidate's frame into a device store; the elites' frames leave it in one more D2H once the ranking is known,
and `rollout_sheet` composes the debug GIF's sheets from it (rac_cem_rollout_sheet).

Multi-GPU: candidates are independent, so with torch.distributed initialised each rank rolls out
its contiguous slice and ONE all-gather (RCCL over xGMI) of the per-candidate fp64 costs precedes
elite selection.
"""
from __future__ import annotations

import os
import time as timer
from collections import defaultdict

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, ops, parallel_env
from .losses import RobotWorldCost
from .state import DemoGoalState, State


def shard_bounds(n: int, world: int, rank: int):
    """Contiguous, near-equal candidate slices; the tail ranks get the remainder-free part."""
    base, rem = divmod(n, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def gather_costs(local: torch.Tensor, N: int, world: int, rank: int) -> np.ndarray:
    """All ranks' per-candidate fp64 cost sums -> one float64[N] on every rank (one all-gather; RCCL on the
    GPU path, any backend works).  Slices are padded to a common width because shards may differ by one."""
    if world == 1 and not (parallel_env.active() and dist.get_world_size() == 1):
        return local.cpu().numpy()  # (a one-rank group under RAC_DIST_FORCE=1 still runs the collective: RCCL rehearsal)
    width = (N + world - 1) // world
    send = torch.zeros(width, device=local.device, dtype=torch.float64)
    send[:local.numel()] = local
    parts = [torch.empty_like(send) for _ in range(world)]
    dist.all_gather(parts, send)
    out = []
    for r, part in enumerate(parts):
        lo, hi = shard_bounds(N, world, r)
        out.append(part[:hi - lo].cpu().numpy())
    return np.concatenate(out)


class TrajectorySampler(object):
    def __init__(self, cfg, model, cam_ext=None, franka_ik=None, wx250s_bot=None, push_height=None,
                 default_pitch=None, default_roll=None, robot_model=None) -> None:
        self.cfg = cfg
        self.model = model
        self.cost = RobotWorldCost(cfg)
        self.low = torch.tensor([[0.015, -0.3, 0.1, 0, 0]], dtype=torch.float32)   # trajectory_sampler.py:22-23
        self.high = torch.tensor([[0.55, 0.3, 0.4, 1, 1]], dtype=torch.float32)
        self.robot_model = robot_model
        self._refining = False  # inside the exact re-roll of the elites (no sharding, no nested refinement)
        self._robot_ctor = (cam_ext, franka_ik, wx250s_bot, push_height, default_pitch, default_roll)
        self._obs_store = None        # (T, n, 3, H, W) fp32 on the device: every candidate's frames of a `ret_obs` call
        self._obs_last = None         # (store, opt row or None) of the last `ret_obs` call, for rollout_sheet
        self.last_obs_d2h_bytes = 0   # what the last `ret_obs` call copied to the host for rollouts["obs"/"optimal_obs"]
        self.last_obs_d2h_copies = 0
        if os.environ.get("RAC_GC_FREEZE", "0") == "1":  # opt-in, see PredictionTrainer.__init__
            import gc
            gc.collect()
            gc.freeze()

    def _needs_robot(self):
        cfg = self.cfg
        return (cfg.model_use_robot_state or cfg.model_use_mask or cfg.black_robot_input
                or "dontcare" in cfg.reward_type)

    def _get_robot_model(self):
        """The analytical robot model (CPU IK + MuJoCo mask render, trajectory_sampler.py:26-33) is the
        reference's own; pass `robot_model=` or run inside the reference tree."""
        if self.robot_model is None:
            cam_ext, franka_ik, wx250s_bot, push_height, pitch, roll = self._robot_ctor
            if self.cfg.experiment == "control_franka":
                from src.dataset.franka.franka_model import FrankaAnalyticalModel
                self.robot_model = FrankaAnalyticalModel(self.cfg, franka_ik, cam_ext)
            else:
                from src.dataset.wx250s.wx250s_model import WX250sAnalyticalModel
                self.robot_model = WX250sAnalyticalModel(self.cfg, wx250s_bot, push_height, pitch, roll,
                                                         cam_ext=cam_ext)
        return self.robot_model

    def _robot_data(self, action_sequences, start, N, T):
        """The batch `predict_batch` is asked about: every candidate starts from the current robot state
        (trajectory_sampler.py:86-99)."""
        cfg = self.cfg
        states = torch.zeros((T + 1, N, 5), dtype=torch.float32)
        qpos = torch.zeros((T + 1, N, cfg.robot_joint_dim), dtype=torch.float32)
        start_state = torch.tensor(start.state)
        if cfg.experiment in ("control_franka", "control_wx250s"):
            from src.utils.camera_calibration import LOCO_FRANKA_DIFF, LOCO_WX250S_DIFF
            start_state[:2] = start_state[:2] + (LOCO_FRANKA_DIFF if cfg.experiment == "control_franka"
                                                 else LOCO_WX250S_DIFF)
        states[0, :] = (start_state - self.low) / (self.high - self.low)  # robonet_dataset.normalize
        qpos[0, :] = torch.tensor(start.qpos)
        return {"states": states, "qpos": qpos, "actions": action_sequences.permute(1, 0, 2),
                "low": self.low.repeat(N, 1), "high": self.high.repeat(N, 1)}

    def _predict_robot(self, action_sequences, start, N, T):
        """states (T+1,N,5) normalised, masks (T+1,N,1,H,W) for every candidate (trajectory_sampler.py:86-109)."""
        return self._get_robot_model().predict_batch(self._robot_data(action_sequences, start, N, T), thick=True)

    def _start_masks_shared(self, masks) -> bool:
        """Is row 0 of the robot model's masks (the start state's mask) the same for every candidate?  It is by
        construction of `_robot_data` (one start state for all candidates); answered WITHOUT a device readback on the
        planner's hot path: a model may say so itself (`shared_start_mask`: AtlasRobotModel does, from the host copy of
        the start states it was handed), host tensors (the analytical models return those) are compared on the host,
        and only an unknown model's device tensors cost one readback per call."""
        flag = getattr(self.robot_model, "shared_start_mask", None)
        if flag is not None:
            return bool(flag)
        m0 = masks[0]
        return bool((m0 == m0[:1]).all())  # CPU tensor: no device sync; device tensor: one readback per call

    def _refine_elites(self, sum_cost, action_sequences, start, goal):
        """`cfg.cem_exact_elites = M` with an atlas robot model that remembers the model it was rendered from
        (`AtlasRobotModel.exact`): the M best candidates of the atlas pass are rolled out again with EXACTLY rendered
        masks (the reference's own `predict_batch`, trajectory_sampler.py:86-109 -- M per-candidate renders instead of
        N) and their costs replaced, so the elite set is the one exact masks give whenever it lies inside the screened
        top M.  Every rank re-rolls the same M candidates (no collective when `sample_mean` or an `eps_source` makes the
        re-roll deterministic; otherwise rank 0's M costs are broadcast).  With `sample_mean=False` the re-rolled
        costs carry a fresh draw of the prior noise, like any second evaluation of a stochastic model would."""
        M = int(getattr(self.cfg, "cem_exact_elites", 0) or 0)
        exact = getattr(self.robot_model, "exact", None)
        if M <= 0 or exact is None or self._refining or not self._needs_robot():
            return sum_cost
        n = len(sum_cost)
        top = np.sort(np.argsort(-sum_cost, kind="stable")[:min(M, n)])
        atlas_model, self.robot_model, self._refining = self.robot_model, exact, True
        try:
            redo = self.generate_model_rollouts(action_sequences[:n][torch.from_numpy(top)].clone(), start, goal)
        finally:
            self.robot_model, self._refining = atlas_model, False
        redo_cost = np.asarray(redo["sum_cost"], dtype=np.float64)
        if not self.cfg.sample_mean and getattr(self.model, "eps_source", None) is None and parallel_env.active():
            # a stochastic re-roll draws its prior noise from each rank's own generator (the sharded pass consumed
            # different amounts of it): every rank takes rank 0's M costs, so that all ranks pick the same elites
            buf = torch.from_numpy(redo_cost.copy())
            if dist.get_backend() == "nccl":
                buf = buf.to(torch.device(self.cfg.device))
            dist.broadcast(buf, src=0)
            redo_cost = buf.cpu().numpy()
        sum_cost = sum_cost.copy()
        sum_cost[top] = redo_cost
        self.last_refined = top
        return sum_cost

    def _frame_store(self, T, n, H, W, dev):
        """The `ret_obs` frame store: one fp32 (T, n, 3, H, W) device buffer, kept on the sampler and reused while the
        shape stays (the planner asks with the same shape in every iteration but the last, which adds the opt row).
        T n 3 H W 4 bytes, uncapped: 0.52 GB at 1000 candidates x 14 steps of 48 x 64."""
        shape = (T, n, 3, H, W)
        st = self._obs_store
        if st is None or tuple(st.shape) != shape or st.device != dev:
            self._obs_store = self._obs_last = st = None  # free the old one before the new one is allocated
            st = self._obs_store = torch.empty(shape, device=dev, dtype=torch.float32)
        return st

    def release_obs_store(self):
        """Free the `ret_obs` frame store (the next `ret_obs` call allocates it again)."""
        self._obs_store = self._obs_last = None

    def _sheet_launch(self, rows, start_u8=None, goal_u8=None, goal_mask=None, want_obs=False, want_sheet=False):
        """One rac_cem_rollout_sheet launch over the last `ret_obs` call's store: (obs, sheet) device tensors."""
        if self._obs_last is None:
            raise _lib.RacError("no frame store: call generate_model_rollouts(ret_obs=True) first")
        store = self._obs_last[0]
        T, n, _, H, W = store.shape
        rows = [int(r) for r in rows]
        if not rows or min(rows) < 0 or max(rows) >= n:
            raise _lib.RacError(f"rollout rows {rows} outside the {n} candidates of the frame store")
        dev = store.device
        rows_dev = torch.tensor(rows, dtype=torch.int32).to(dev)
        R = len(rows)
        obs = torch.empty((R, T, 3, H, W), device=dev, dtype=torch.float32) if want_obs else None
        sheet = torch.empty((T + 1, R * H, 3 * W, 3), device=dev, dtype=torch.uint8) if want_sheet else None
        G = 1 if goal_u8 is None else goal_u8.shape[0]
        _lib.call("rac_cem_rollout_sheet", store.data_ptr(), store.stride(0), store.stride(1), rows_dev.data_ptr(), R, T,
                  _lib.ptr(start_u8), _lib.ptr(goal_u8), G, _lib.ptr(goal_mask), _lib.ptr(obs), _lib.ptr(sheet), H, W,
                  _lib.stream_ptr())
        return obs, sheet

    @torch.no_grad()
    def rollout_sheet(self, rows, start: State, goal: DemoGoalState, mask_goal=False) -> np.ndarray:
        """The unlabelled --debug_cem sheet (reference src/cem/cem.py:140-175), uint8 (T+1, R*H, 3W, 3): row block r of
        sheet t+1 is [zeros | frame of candidate rows[r] at step t | goal t], sheet 0 [zeros | start | goal 0].  `rows`
        index the candidates of the last `ret_obs` call (its opt_traj row is the last one).  `mask_goal`: goals blacked
        by `goal.masks` from sheet 1 on (push/cem.py:210-212).  One launch, one device-to-host copy."""
        if self._obs_last is None:
            raise _lib.RacError("no frame store: call generate_model_rollouts(ret_obs=True) first")
        store = self._obs_last[0]
        H, W = store.shape[3], store.shape[4]
        dev = store.device

        def u8(img):
            a = np.ascontiguousarray(np.asarray(img), dtype=np.uint8)
            if a.shape != (H, W, 3):
                raise _lib.RacError(f"rollout_sheet: image of shape {a.shape}, the frames are ({H}, {W}, 3)")
            return a
        start_u8 = torch.from_numpy(u8(start.img)).to(dev)
        goal_u8 = torch.from_numpy(np.stack([u8(g) for g in goal.imgs])).to(dev)
        goal_mask = None
        if mask_goal:
            if goal.masks is None or len(goal.masks) != len(goal.imgs):
                raise _lib.RacError("rollout_sheet: mask_goal needs one goal mask per goal image")
            m = np.stack([np.asarray(g).reshape(H, W) != 0 for g in goal.masks]).astype(np.uint8)
            goal_mask = torch.from_numpy(m).to(dev)
        _, sheet = self._sheet_launch(rows, start_u8, goal_u8, goal_mask, want_sheet=True)
        return sheet.cpu().numpy()

    @torch.no_grad()
    def generate_model_rollouts(self, action_sequences, start: State, goal: DemoGoalState, opt_traj=None,
                                ret_obs=False, ret_step_cost=False, suppress_print=True):
        """Roll the candidate action sequences through the learned model and return
        {"sum_cost": float64[N], ...} exactly as the reference does."""
        cfg, model = self.cfg, self.model
        dev = torch.device(cfg.device)
        if dev.type != "cuda":
            raise _lib.RacError("generate_model_rollouts needs cfg.device on the GPU (no CPU fallback)")
        if opt_traj is not None:  # appended as candidate N+1 (trajectory_sampler.py:62-68)
            opt = torch.cat([opt_traj, torch.zeros((len(opt_traj), 3))], 1).unsqueeze(0)
            action_sequences = torch.cat([action_sequences, opt])
        N, T = action_sequences.shape[0], action_sequences.shape[1]
        H, W = cfg.image_height, cfg.image_width
        start_time = timer.time()

        goal_imgs = torch.stack([torch.from_numpy(g).permute(2, 0, 1).float() / 255 for g in goal.imgs]).to(dev)
        goal_masks = None
        if goal.masks is not None:
            goal_masks = torch.stack([torch.from_numpy(np.asarray(g)) for g in goal.masks]).to(dev).to(torch.uint8)
        dontcare_in = "dontcare" in cfg.reconstruction_loss or cfg.black_robot_input
        dontcare_cost = "dontcare" in cfg.reward_type
        kind = 1 if dontcare_cost else 0
        w_world = float(cfg.world_cost_weight)

        # ---- candidate sharding over ranks (one process per GPU) ----
        world, rank = 1, 0
        # the debug outputs (predicted frames / per-step costs of the elites, indexed over ALL candidates) are not
        # gathered: a call that asks for them rolls every candidate out on every rank
        if getattr(cfg, "cem_shard", True) and not (ret_obs or ret_step_cost) and not self._refining:
            world, rank = parallel_env.world_rank()
        lo, hi = shard_bounds(N, world, rank)
        n_local = hi - lo
        # the robot model is asked about THIS rank's candidates only (the reference asks about all N,
        # trajectory_sampler.py:86-109; a candidate's states and masks depend on nothing but its own actions): at cfg4 a
        # rank builds (15, 1000, 1, 64, 64) masks, not (15, 8000, ...).  `states` / `masks` are indexed shard-locally.
        states = masks = None
        shared_mask0 = True
        if self._needs_robot() and n_local > 0:
            states, masks = self._predict_robot(action_sequences[lo:hi], start, n_local, T)
            shared_mask0 = self._start_masks_shared(masks)
            states = states.to(dev, non_blocking=True)
            masks = masks.to(dev, torch.float32, non_blocking=True)
        per = cfg.candidates_batch_size
        nb = max(n_local // per, 1)
        sum_cost_dev = torch.zeros(max(n_local, 1), device=dev, dtype=torch.float64)
        # ret_obs: every step's composite frame is written by the step tail straight into the device store (ret_obs
        # disables sharding: n_local == N); the elites' frames are picked out of it once the ranking is known
        store = None
        if ret_obs:
            self._obs_last = None  # the store is being overwritten: no sheet of it until this call has finished
            store = self._frame_store(T, n_local, H, W, dev)
        step_cost = np.zeros((N, T)) if ret_step_cost else None
        start_img = (torch.from_numpy(start.img.copy()).permute(2, 0, 1).float() / 255).to(dev)
        actions_dev = action_sequences.to(dev, torch.float32)
        # step 0: every candidate sees the start frame (and the start mask, row 0 of the robot model's answer): the encoder
        # runs on one image.  A future mask is the candidate's own.  Decided once per call, without a device readback.
        shared0 = (getattr(cfg, "cem_shared_start", True) and not cfg.model_use_future_mask
                   and not getattr(cfg, "model_use_heatmap", False)
                   and (shared_mask0 or not (cfg.model_use_mask or dontcare_in)))

        for b in range(nb if n_local > 0 else 0):
            s = lo + b * per
            e = lo + (b + 1) * per if b < nb - 1 else hi
            n = e - s
            ls, le = s - lo, e - lo  # shard-local rows of states / masks / sum_cost_dev
            model.init_hidden(batch_size=n)
            curr = start_img.expand(n, -1, -1, -1).contiguous()
            if dontcare_in:
                curr = ops.ZeroRegion.apply(curr, masks[0, ls:le].contiguous())
            for t in range(T):
                ac = actions_dev[s:e, t].contiguous()
                mask = masks[t, ls:le] if cfg.model_use_mask else None
                state = states[t, ls:le] if cfg.model_use_robot_state else None
                if cfg.model_use_future_mask:
                    mask = torch.cat([mask, masks[t + 1, ls:le]], 1)
                if cfg.model_use_future_robot_state:
                    state = (state, states[t + 1, ls:le])
                shared = t == 0 and shared0
                x4 = model.forward_maps(curr, mask, state, None, ac, False, sample_mean=cfg.sample_mean,
                                        shared_frame=shared)[0]
                gi = t if t < len(goal_imgs) else -1
                add = (not cfg.sparse_cost) or t == T - 1
                nxt = store[t, ls:le] if ret_obs else torch.empty_like(curr)  # (a contiguous slice of the store)
                before = sum_cost_dev[ls:le].clone() if ret_step_cost else None
                # locals: the (possibly copied) operands must outlive the raw-pointer launch
                next_mask = masks[t + 1, ls:le].contiguous() if (dontcare_in or dontcare_cost) else None
                goal_mask = goal_masks[gi].contiguous() if (dontcare_cost and goal_masks is not None) else None
                goal_img = goal_imgs[gi].contiguous()
                _lib.call(
                    "rac_cem_step_tail", x4.data_ptr(), curr.data_ptr(), _lib.ptr(next_mask) if dontcare_in else None,
                    goal_img.data_ptr(), _lib.ptr(next_mask) if dontcare_cost else None, _lib.ptr(goal_mask),
                    kind, w_world, 1 if (add and w_world != 0) else 0, nxt.data_ptr(),
                    sum_cost_dev[ls:le].data_ptr(), n, H * W, _lib.stream_ptr())
                if ret_step_cost:
                    step_cost[s:e, t] = (sum_cost_dev[ls:le] - before).cpu().numpy()
                curr = nxt

        # ---- gather the per-candidate costs: the only collective of a CEM iteration ----
        if getattr(self, "time_gather", False):  # bench.py: time the collective alone (drain the rollouts first)
            torch.cuda.synchronize()
        t_gather = timer.time()
        sum_cost = gather_costs(sum_cost_dev[:n_local], N, world, rank)
        self.last_gather_s = timer.time() - t_gather

        if not suppress_print:
            print("======= Samples Gathered  ======= | >>>> Time taken = %f " % (timer.time() - start_time))
        rollouts = defaultdict(float)
        if opt_traj is not None:
            rollouts["optimal_sum_cost"] = sum_cost[-1]
            if ret_obs:
                rollouts["optimal_obs"] = None  # (keeps its place among the keys; filled with the elites' frames below)
            sum_cost = sum_cost[:-1]
        sum_cost = self._refine_elites(sum_cost, action_sequences, start, goal)
        rollouts["sum_cost"] = sum_cost
        if ret_obs:
            topk_idx = np.argsort(sum_cost)[-cfg.topk:]
            rollouts["topk_idx"] = topk_idx
            # the elites' (and the opt row's) frames out of the store: one launch, one device-to-host copy
            opt_row = N - 1 if opt_traj is not None else None
            self._obs_last = (store, opt_row)
            rows = list(topk_idx) + ([opt_row] if opt_row is not None else [])
            self.last_obs_d2h_bytes = self.last_obs_d2h_copies = 0
            if rows:
                picked = self._sheet_launch(rows, want_obs=True)[0].cpu()
                self.last_obs_d2h_bytes, self.last_obs_d2h_copies = picked.numel() * picked.element_size(), 1
                picked = picked.numpy()
            else:
                picked = np.zeros((0, T, 3, H, W), np.float32)
            rollouts["obs"] = picked[:len(topk_idx)]
            if opt_row is not None:
                rollouts["optimal_obs"] = picked[-1]
        if ret_step_cost:
            rollouts["step_cost"] = step_cost[:len(sum_cost)]
        return rollouts
