"""CPU restatement of the deterministic baselines (reference dynamics.py:341-454, trainer.py:326-465 and :566-734 with
`--model det` / `--model copy`), built from the pieces of `oracle.svg_oracle`: forward, train step and eval step of
DeterministicConvModel, CopyModel and its eval step, and a name-keyed weight generator for the det state dict.
Checked against the reference's own outputs in tests/test_det_host.py (fixtures of tools/gen_golden_det.py)."""
import math
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import Tensor

from oracle import svg_oracle as orc


def width(cfg) -> int:
    """ConvLSTM width (dynamics.py:403)."""
    return cfg.g_dim + 2 + (2 if cfg.model_use_robot_state else 0)


def enc_in_channels(cfg) -> int:
    """dynamics.py:383-388: no heatmap channel, whatever the flags say."""
    c = cfg.channels
    if cfg.model_use_mask:
        c += 1 + (1 if cfg.model_use_future_mask else 0)
    return c


def param_spec(cfg):
    """(key, shape, kind) in the reference's state_dict order (dynamics.py:389-410)."""
    g, wd = cfg.g_dim, width(cfg)
    hw2 = 2 * (cfg.image_height // 8) * (cfg.image_width // 8)
    spec = []
    for name, chans in orc.ENC_PLAN:
        chans = [enc_in_channels(cfg) if c is None and i == 0 else (g if c is None else c) for i, c in enumerate(chans)]
        for i in range(len(chans) - 1):
            spec += orc._vgg_entries(f"encoder.{name}.{i}", chans[i], chans[i + 1])
    spec += [("action_encoder.0.weight", (hw2, cfg.action_dim), "lin_w"), ("action_encoder.0.bias", (hw2,), "conv_b")]
    if cfg.model_use_robot_state:
        spec += [("state_encoder.0.weight", (hw2, cfg.robot_dim), "lin_w"), ("state_encoder.0.bias", (hw2,), "conv_b")]
    spec += orc._lstm_entries("frame_predictor", wd)
    for name, chans in orc.DEC_PLAN:
        chans = [wd if c is None else c for c in chans]
        for i in range(len(chans) - 1):
            spec += orc._vgg_entries(f"decoder.{name}.{i}", chans[i], chans[i + 1])
    spec.append(("decoder.upc5.1.weight", (64, cfg.channels + 1, 3, 3), "convT_w"))
    spec.append(("decoder.upc5.1.bias", (cfg.channels + 1,), "conv_b"))
    return spec


def make_weights(cfg, seed: int = 0, randomize_bn_stats: bool = True) -> Dict[str, Tensor]:
    """Name-keyed synthetic det state dict, the scheme of `orc.make_weights` (Philox keyed by crc32(key)): He-scaled
    vgg convs, 1/sqrt(fan_in) gate convs and Linears."""
    out = {}
    for key, shape, kind in param_spec(cfg):
        rng = np.random.Generator(np.random.Philox(key=[zlib.crc32(key.encode()), seed]))
        normal = lambda std: torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * np.float32(std))
        if kind in ("conv_w", "convT_w"):
            fan_in = int(np.prod(shape[1:])) if kind == "conv_w" else shape[0] * shape[2] * shape[3]
            out[key] = normal(math.sqrt((1.0 if "gates." in key else 2.0) / fan_in))
        elif kind == "lin_w":
            out[key] = normal(1.0 / math.sqrt(shape[1]))
        elif kind == "conv_b":
            out[key] = normal(0.05)
        elif kind == "bn_w":
            out[key] = 1 + normal(0.1)
        elif kind == "bn_b":
            out[key] = normal(0.1)
        elif kind == "bn_rm":
            v = normal(0.1)
            out[key] = v if randomize_bn_stats else torch.zeros(shape)
        elif kind == "bn_rv":
            v = torch.from_numpy(rng.uniform(0.5, 1.5, shape).astype(np.float32))
            out[key] = v if randomize_bn_stats else torch.ones(shape)
        else:
            out[key] = torch.zeros((), dtype=torch.int64)
    return out


def init_hidden(cfg, batch: int):
    h, w = cfg.image_height // 8, cfg.image_width // 8
    return [(torch.zeros(batch, width(cfg), h, w), torch.zeros(batch, width(cfg), h, w)) for _ in range(2)]


def det_forward(sd, cfg, hidden, image, mask, robot, action, skip=None, training=False):
    """DeterministicConvModel.forward (dynamics.py:422-454); mutates `hidden`.  Returns (x_pred4, skip)."""
    x = torch.cat([image, mask], 1) if cfg.model_use_mask else image
    h, curr_skip = orc.encoder(sd, x, training)
    if skip is None:
        skip = curr_skip
    hh, ww = cfg.image_height // 8, cfg.image_width // 8
    lin = lambda name, v: torch.nn.functional.linear(v, sd[f"{name}.0.weight"], sd[f"{name}.0.bias"]).view(-1, 2, hh, ww)
    parts = [h, lin("action_encoder", action)]
    if cfg.model_use_robot_state:
        parts.append(lin("state_encoder", robot))
    h_pred = orc.convlstm(sd, "frame_predictor", torch.cat(parts, 1), hidden)
    return orc.decoder(sd, h_pred, skip, training), skip


@dataclass
class TrainState:
    sd: Dict[str, Tensor]
    cfg: object
    optimizer: torch.optim.Optimizer = None
    param_keys: List[str] = field(default_factory=list)

    @staticmethod
    def create(cfg, sd, optimizer: str = "adam") -> "TrainState":
        sd = {k: v.clone() for k, v in sd.items()}
        keys = [k for k, _, kind in param_spec(cfg) if not orc.is_buffer(kind)]
        for k in keys:
            sd[k].requires_grad_(True)
        params = [sd[k] for k in keys]
        if optimizer == "adam":  # trainer.py:109-116
            opt = torch.optim.Adam(params, lr=cfg.lr, betas=(cfg.beta1, 0.999))
        else:
            opt = {"rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD}[optimizer](params)
        return TrainState(sd, cfg, opt, keys)


def train_step(ts: TrainState, data, use_truth: Optional[List[bool]] = None, do_update: bool = True):
    """One `_train_step` with --model det (trainer.py:326-465); `use_truth[i]` replaces the scheduled-sampling coin
    at time index i, as in PredictionTrainer._train_step.  No `kld` key."""
    cfg, sd = ts.cfg, ts.sd
    x, states, ac, mask = data["images"], data["states"], data["actions"], data["masks"]
    losses = {"recon_loss": 0.0, "robot_loss": 0.0, "world_loss": 0.0}
    for k in ts.param_keys:
        sd[k].grad = None
    hidden = init_hidden(cfg, min(cfg.batch_size, x.shape[1]))
    dontcare = "dontcare" in cfg.reconstruction_loss or cfg.black_robot_input
    recon = 0
    x_pred = skip = None
    for i in range(1, cfg.n_past + cfg.n_future):
        truth = True if (i == 1 or use_truth is None) else use_truth[i]
        x_j = x[i - 1] if truth else x_pred.clone()
        m_j, r_j, a_j, x_i, m_i = mask[i - 1], states[i - 1], ac[i - 1], x[i], mask[i]
        x_j_black = orc.zero_robot_region(m_j, x_j) if dontcare else x_j
        if cfg.last_frame_skip:
            skip = None
        m_in = torch.cat([m_j, m_i], 1) if cfg.model_use_future_mask else m_j
        x4, curr_skip = det_forward(sd, cfg, hidden, x_j_black, m_in, r_j, a_j, skip, training=True)
        x_pred = orc.composite(x4, x_j)
        if i <= cfg.n_past:
            skip = curr_skip
        view = orc.recon_loss(cfg, x_pred, x_i, m_i)
        recon = recon + view
        losses["recon_loss"] += view.item()
        with torch.no_grad():
            losses["robot_loss"] += orc.robot_mse(x_pred, x_i, m_i).item()
            losses["world_loss"] += orc.world_mse(x_pred, x_i, m_i).item()
    recon.backward()
    if do_update:
        ts.optimizer.step()
    return {k: v / cfg.n_future for k, v in losses.items()}


def copy_forward(image, mask, next_image, next_mask):
    """CopyModel.forward (dynamics.py:346-357)."""
    keep = next_mask.type(torch.bool).repeat(1, 3, 1, 1)
    return torch.where(keep, next_image, image)


@torch.no_grad()
def eval_step(sd, cfg, data, n_eval: int, autoregressive: bool, model: str = "det"):
    """`_eval_step` with --model det (the model in eval mode) or --model copy (trainer.py:566-734): the rollout runs on
    `pred_masks`, the scores on `masks`.  No `*_kld` key."""
    x, states, ac, true_masks = data["images"], data["states"], data["actions"], data["masks"]
    masks = data.get("pred_masks", true_masks)
    hidden = init_hidden(cfg, x.shape[1])
    prefix = "autoreg" if autoregressive else "1step"
    dontcare = "dontcare" in cfg.reconstruction_loss or cfg.black_robot_input
    losses, k_losses = {}, {}
    add = lambda k, v: losses.__setitem__(k, losses.get(k, 0.0) + float(v))
    x_pred = skip = None
    for i in range(1, n_eval):
        x_j = x_pred.clone() if (autoregressive and i > 1) else x[i - 1]
        m_j, r_j, a_j, m_i, x_i, tm = masks[i - 1], states[i - 1], ac[i - 1], masks[i], x[i], true_masks[i]
        if model == "copy":
            x_pred = copy_forward(x_j, m_j, x_i, m_i)
        else:
            x_j_black = orc.zero_robot_region(m_j, x_j) if dontcare else x_j
            if cfg.last_frame_skip:
                skip = None
            m_in = torch.cat([m_j, m_i], 1) if cfg.model_use_future_mask else m_j
            x4, curr_skip = det_forward(sd, cfg, hidden, x_j_black, m_in, r_j, a_j, skip)
            x_pred = orc.composite(x4, x_j)
            if i <= cfg.n_past:
                skip = curr_skip
        add(f"{prefix}_recon_loss", orc.recon_loss(cfg, x_pred, x_i, tm))
        add(f"{prefix}_robot_loss", orc.robot_mse(x_pred, x_i, tm))
        wm = float(orc.world_mse(x_pred, x_i, tm))
        add(f"{prefix}_world_loss", wm)
        pb, tb = orc.zero_robot_region(tm, x_pred), orc.zero_robot_region(tm, x_i)
        p = float(orc.psnr(tb.clamp(0, 1), pb.clamp(0, 1)).mean())
        s_ = float(orc.ssim_map(tb, pb).mean())
        add(f"{prefix}_psnr", p)
        add(f"{prefix}_ssim", s_)
        if autoregressive:
            k_losses.update({f"{i}_step_psnr": p, f"{i}_step_ssim": s_, f"{i}_step_world_loss": wm})
    out = {k: v / (n_eval - 1) for k, v in losses.items()}
    out.update(k_losses)
    return out
