"""The action-sweep probe (reference src/prediction/test_action_rollout.py): does a trained model follow its actions?

One test batch, its recorded actions replaced by constant pushes of +-`step_size` along x and y (the recorded z column
kept), the frozen model rolled out under every such action set, one GIF per sweep with rows
[ground truth | sample 0 | sample 1 | ...].  The reference runs sweeps x samples rollouts one after the other and builds
its sheets on the CPU; here all of them are ONE batch of S G b videos (`rollout`), and one launch
(`ops.action_rollout_sheet`) turns the frames left on the device into the sheets and into the response table: the mean
absolute difference of every predicted frame from the same sample's frame under the recorded actions.  The samples of
all sweeps share their prior noise, so that difference is what the actions did."""
from __future__ import annotations

import json
import os
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import ops
from .trainer import model_step

RECORDED = "recorded"
AXES = {"x": 0, "y": 1}
MAX_VIDEOS = 10  # test_action_rollout.py:79


def sweep_actions(actions: torch.Tensor, step_size: float = 0.02, axes: Sequence[str] = ("x", "y"),
                  directions: Sequence[int] = (-1, 1), include_recorded: bool = True):
    """(names, sets): the counterfactual action sets of test_action_rollout.py:196-213 for the time-first `actions`
    (T - 1, B, A), stacked as `sets` (S, T - 1, B, A).  Each sweep is zeros with column 2 (z) copied from `actions` and
    column `axis` set to `step_size * direction`; directions are the outer loop, axes the inner one; the names are the
    reference's GIF stems, `x_-20mm, y_-20mm, x_20mm, y_20mm` by default.  `include_recorded` (not in the reference)
    puts the batch's own actions first as sweep "recorded", the base of the response table."""
    names, sets = [], []
    if include_recorded:
        names.append(RECORDED)
        sets.append(actions.clone())
    for direction in directions:
        for ax in axes:
            if ax not in AXES:
                raise ValueError(ax)
            fake = torch.zeros_like(actions)
            fake[:, :, 2] = actions[:, :, 2]
            fake[:, :, AXES[ax]] = step_size * direction
            names.append(f"{ax}_{int(direction * step_size * 1000)}mm")
            sets.append(fake)
    return names, torch.stack(sets)


def _robot_inputs(config, data, sets, L, b, robot_model, dev):
    """States, masks and heatmaps (or None) of every sweep as (L, S, b, ...).  finetune_* experiments of a model that
    takes masks or robot states: from ONE `robot_model.predict_batch` call over all S b samples, sweep s in rows
    [s b, (s + 1) b) with its own actions (test_action_rollout.py:43-70).  Otherwise the batch's true ones for every
    sweep (:36-41)."""
    f32 = torch.float32
    S = sets.shape[0]
    use_heatmap = bool(getattr(config, "model_use_heatmap", False)) and config.model == "svg"
    clip = lambda key, n=L: data[key][:n, :b].to(dev, f32)
    per_sweep = lambda t: t.unsqueeze(1).expand((t.shape[0], S) + tuple(t.shape[1:]))
    if not ("finetune" in config.experiment and (config.model_use_mask or config.model_use_robot_state)):
        return per_sweep(clip("states")), per_sweep(clip("masks")), per_sweep(clip("heatmaps")) if use_heatmap else None
    if robot_model is None:
        raise NotImplementedError(
            "finetune_* windows take their robot states and masks from an analytical / learned robot model: set "
            "`trainer.robot_model` to an object with predict_batch(batch) -> (states, masks[, heatmaps]) -- the "
            "reference's LocobotAnalyticalModel, robot_atlas.AtlasRobotModel or robot_model.LearnedRobotModel")
    tile = lambda t: t.repeat((1, S) + (1,) * (t.dim() - 2))       # (n, b, ...) -> (n, S b, ...)
    rows = lambda t: t[:b].to(dev).repeat((S,) + (1,) * (t.dim() - 1))  # (B, ...) -> (S b, ...)
    batch = {"states": tile(clip("states")), "masks": tile(clip("masks")), "robot": list(data["robot"][:b]) * S,
             "actions": sets[:, :L - 1, :b].to(dev, f32).permute(1, 0, 2, 3).reshape(L - 1, S * b, -1),
             "low": rows(data["low"]), "high": rows(data["high"])}
    if "qpos" in data:
        batch["qpos"] = tile(clip("qpos"))
    if "folder" in data:
        batch["folder"] = list(data["folder"][:b]) * S
    if use_heatmap:
        batch["heatmaps"] = tile(clip("heatmaps"))
    if getattr(config, "preprocess_action", "raw") != "raw":  # the recorded raw tables, as the reference hands them over
        batch.update(raw_actions=tile(clip("raw_actions", L - 1)), raw_states=tile(clip("raw_states")),
                     raw_low=rows(data["raw_low"]), raw_high=rows(data["raw_high"]))
    out = robot_model.predict_batch(batch)
    split = lambda t: t.to(dev, f32).reshape((t.shape[0], S, b) + tuple(t.shape[2:]))
    return split(out[0]), split(out[1]), split(out[2]) if use_heatmap else None


@torch.no_grad()
def rollout(model, config, data, sets, video_len, nsample=3, robot_model=None):
    """`plot_rollout` (test_action_rollout.py:72-150) of every action set at once: the device tensor `gen`
    (S, G, L, b, 3, H, W) with L = `video_len`, b = min(B, 10) and G = `nsample` for --model svg, 1 for det and copy
    (the reference plots sample 0 only for those).  `data` is a time-first batch, `sets` (S, T - 1, B, A); the start
    frame is 0.

    The rules are the reference's.  The first frame is zero_robot_region(masks[0], x[0]) under a dontcare loss or
    `black_robot_input`; svg reads the blacked frame, det reads `x_j` as it stands (:119); the composite is
    (1 - m) x_j + m x_pred over the frame fed in; under dontcare the prediction is blacked by masks[i]; the stored frame
    is the one fed next, ground truth for i < n_past and the prediction after; `copy` calls the model on the pair and
    composites nothing; `last_frame_skip` and the i <= n_past skip rule are `trainer.model_step`'s.

    Under a finetune* experiment with `model_use_mask` or `model_use_robot_state` the states and masks (and heatmaps)
    of every sweep come from `robot_model.predict_batch`, asked once for all S b samples.  Otherwise every sweep rolls
    out on the batch's true states and masks, as the reference does: the masks then do NOT follow the fake actions, and
    only the action input of the model differs between sweeps.

    The pass is ONE batch of S G b videos, row (s G + g) b + i, with the model in eval() under no_grad: the frozen
    path's arithmetic does not depend on what shares a video's batch, so `gen[s]` is what rolling sweep s out alone
    gives.  Prior noise is drawn once per step for (G b, z, h, w) -- `model.eps_source`, when set, is asked for that
    shape -- and repeated over the sweeps: sweeps differ by their actions only."""
    cf = config
    dev, f32 = torch.device(cf.device), torch.float32
    S, L = int(sets.shape[0]), int(video_len)
    B = data["images"].shape[1]
    b = min(B, MAX_VIDEOS)
    if not (2 <= L <= data["images"].shape[0] and sets.shape[1] >= L - 1 and sets.shape[2] == B):
        raise ValueError(f"rollout: video_len {L} and action sets {tuple(sets.shape)} do not fit a batch of "
                         f"{tuple(data['images'].shape)}")
    G = int(nsample) if cf.model == "svg" else 1
    N = S * G * b
    states, masks, heatmaps = _robot_inputs(cf, data, sets, L, b, robot_model, dev)

    def batch_of(t):  # (n, S, b, ...) -> (n, S G b, ...), row (s G + g) b + i
        t = t.unsqueeze(2).expand((t.shape[0], S, G) + tuple(t.shape[2:]))
        return t.reshape((t.shape[0], N) + tuple(t.shape[4:])).contiguous()
    states, masks = batch_of(states), batch_of(masks)
    heatmaps = None if heatmaps is None else batch_of(heatmaps)
    ac = batch_of(sets[:, :L - 1, :b].to(dev, f32).permute(1, 0, 2, 3))
    x = data["images"][:L, :b].to(dev, f32).repeat(1, S * G, 1, 1, 1)
    dontcare = "dontcare" in cf.reconstruction_loss or cf.black_robot_input

    source = getattr(model, "eps_source", None)

    def shared_noise(shape):  # one draw for the G b videos of a sweep, the same for every sweep
        assert shape[0] == N, (shape, N)
        one = (G * b,) + tuple(shape[1:])
        e = source(one) if source is not None else torch.randn(one, device=dev)
        return e.to(dev, f32).repeat(S, 1, 1, 1)

    was_training = model.training
    model.eval()
    if cf.model == "svg":
        model.eps_source = shared_noise
    try:
        model.init_hidden(N)
        x_j = ops.ZeroRegion.apply(x[0].contiguous(), masks[0]) if dontcare else x[0]
        frames = [x_j]
        skip = None
        for i in range(1, L):
            if cf.model == "copy":
                x_pred = model(x_j, masks[i - 1], x[i], masks[i])
            else:
                x4, skip, _ = model_step(model, cf, i, x_j, masks, states, ac, heatmaps, skip, posterior=False,
                                         dontcare=dontcare and cf.model == "svg")
                x_pred = ops.Composite.apply(x4, x_j.contiguous())
                if dontcare:
                    x_pred = ops.ZeroRegion.apply(x_pred, masks[i])
            x_j = x[i] if i < cf.n_past else x_pred
            frames.append(x_j)
    finally:
        if cf.model == "svg":
            model.eps_source = source
        model.train(was_training)
    return torch.stack(frames).reshape(L, S, G, b, *x.shape[2:]).permute(1, 2, 0, 3, 4, 5, 6).contiguous()


def response_summary(names, response, base):
    """What `response.json` holds: per sweep the mean of the (S, G, L, b) table over samples and videos, per step and
    over the whole rollout (the conditioning frames, which no action can move, included), plus the table's shape."""
    r = np.asarray(response, dtype=np.float64)
    return {"base": base, "shape": list(r.shape), "layout": ["sweep", "sample", "step", "video"],
            "sweeps": {n: {"per_step": [float(v) for v in r[s].mean(axis=(0, 2))], "mean": float(r[s].mean())}
                       for s, n in enumerate(names)}}


class ActionRollout(NamedTuple):
    """A probe's result: `gen` (S, G, L, b, 3, H, W) on the device, `sheets` uint8 numpy (S, L, b H, (1 + G) W + G, 3)
    from one device-to-host copy, `response` numpy (S, G, L, b) or None without a "recorded" sweep."""
    names: list
    gen: torch.Tensor
    sheets: np.ndarray
    response: Optional[np.ndarray]

    def summary(self):
        return None if self.response is None else response_summary(self.names, self.response, RECORDED)

    def write(self, out_dir):
        """`<name>.gif` per sweep (250 ms per frame, as `PredictionTrainer.plot`) and `response.json`."""
        from PIL import Image
        os.makedirs(out_dir, exist_ok=True)
        files = []
        for name, sheet in zip(self.names, self.sheets):
            imgs = [Image.fromarray(f) for f in sheet]
            files.append(os.path.join(out_dir, name + ".gif"))
            imgs[0].save(files[-1], save_all=True, append_images=imgs[1:], duration=250, loop=0)
        if self.response is not None:
            files.append(os.path.join(out_dir, "response.json"))
            with open(files[-1], "w") as f:
                json.dump(self.summary(), f, indent=1)
        return files


def probe(model, config, data, step_size=0.02, video_len=5, nsample=3, include_recorded=True, robot_model=None):
    """Sweep, roll out, and make the sheets and the response table: one batched pass, one launch, one copy of the
    sheets to the host (and one of the small table)."""
    names, sets = sweep_actions(data["actions"], step_size, include_recorded=include_recorded)
    gen = rollout(model, config, data, sets, video_len, nsample, robot_model)
    base = names.index(RECORDED) if RECORDED in names else None
    sheets, response = ops.action_rollout_sheet(data["images"].to(gen.device), gen, base)
    return ActionRollout(names, gen, sheets.cpu().numpy(), None if response is None else response.cpu().numpy())
