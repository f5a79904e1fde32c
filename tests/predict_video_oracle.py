"""CPU restatement of the video export (reference trainer.py:1149-1408: `PredictionTrainer.predict_video` and its worker
`_predict_video`), in plain torch on the pieces of `oracle.svg_oracle` (svg) and `tests/det_oracle.py` (det, copy), with
the prior's and the posterior's N(0,1) draws injected.  Checked against the reference's own outputs in
tests/test_predict_video_host.py (fixtures of tools/gen_golden_predict_video.py)."""
from math import floor

import numpy as np
import torch

from oracle import svg_oracle as orc

try:
    from tests import det_oracle as det
except ImportError:  # loaded by path next to det_oracle (tools/gen_golden_predict_video.py)
    import det_oracle as det

FRAME_SHARE = 255e-4  # frame criterion: at most this share of uint8 elements may differ, each by at most 1


class RolledRobotModel:
    """Stands in for the analytical robot model of the finetune_* experiments: `predict_batch` returns the window's own
    states and its true masks moved one pixel to the right, so the rollout's masks differ from the scoring masks and
    every window gets its own."""

    def predict_batch(self, batch, thick=True):
        return batch["states"].clone(), torch.roll(batch["masks"], 1, dims=-1)


RA_FLAGS = dict(model_use_mask=True, model_use_future_mask=True, model_use_robot_state=True,
                reconstruction_loss="dontcare_l1")


def best3_problem(syn):
    """(cfg, weights, video) of the three-sample fixture.  On `synth_video`'s independent random frames with the plain
    synthetic weights the three samples' world losses differ by ~1e-5 relative (the error against an unpredictable
    next frame swamps what z changes), and a selection test would be decided by rounding.  So: a static video (every
    frame is frame 0; masks, states and actions still move), a composite mask that starts near 0.02 (the prediction
    stays near the frame fed in), and gains of 8 on the z columns of the frame predictor's input conv and on the
    decoder's first conv, so that the sample drawn moves the frames.  The world losses then differ by percents."""
    cfg = orc.Cfg(g_dim=64, z_dim=16, batch_size=2, n_past=1, n_future=2, **RA_FLAGS)
    sd = orc.make_weights(cfg, seed=7)
    sd["frame_pred_input_conv.weight"][:, -cfg.z_dim:] *= 8
    sd["decoder.upc2.0.main.0.weight"] *= 8
    sd["decoder.upc5.1.bias"][3] = -4.0
    data = syn.synth_video(seed=62, T=8, B=2)
    data["images"] = data["images"][:1].repeat(8, 1, 1, 1, 1)
    data["low"], data["high"] = torch.zeros(2, 5), torch.ones(2, 5)  # handed to the robot model, which ignores them
    return cfg, sd, data


def eps_table(syn, seed, windows, samples, steps=3, B=2, z=16, h=8, w=8):
    """eps[w][s] = the per-step (prior, posterior) draws of window w, sample s."""
    return [[syn.synth_eps(seed=seed + 10 * win + s, steps=steps, B=B, z=z, h=h, w=w) for s in range(samples)]
            for win in range(windows)]


def to_uint8_video(frames):
    """trainer.py:1395-1407: list over time of (B, 3, H, W) -> uint8 (B, T, H, W, 3), truncating."""
    v = torch.stack(frames).transpose(0, 1)
    return (255 * v).permute(0, 1, 3, 4, 2).cpu().numpy().astype(np.uint8)


@torch.no_grad()
def predict_snippet(sd, cfg, data, n_eval, eps=None, model="svg", autoregressive=True):
    """`_predict_video` (trainer.py:1227-1408) with the model in eval mode; `eps[i-1]` = (prior, posterior) draws of
    step i (svg only).  `data["pred_masks"]` drives the rollout, `data["masks"]` scores and blacks the frames."""
    x, states, ac, true_masks = data["images"], data["states"], data["actions"], data["masks"]
    masks = data.get("pred_masks", true_masks)
    bs = x.shape[1]
    hidden = None if model == "copy" else (orc.init_hidden(cfg, bs) if model == "svg" else det.init_hidden(cfg, bs))
    prefix = "autoreg" if autoregressive else "1step"
    dontcare = "dontcare" in cfg.reconstruction_loss or cfg.black_robot_input
    robot_name = np.array(data["robot"])
    all_robots = sorted(set(robot_name))
    losses, k_losses = {}, {}
    add = lambda d, k, v: d.__setitem__(k, d.get(k, 0.0) + float(v))
    gen, true = [], []
    x_pred = skip = None
    for i in range(1, n_eval):
        x_j = x_pred.clone() if (autoregressive and i > 1) else x[i - 1]
        m_j, r_j, a_j, m_i, r_i, x_i, tm = masks[i - 1], states[i - 1], ac[i - 1], masks[i], states[i], x[i], true_masks[i]
        if model == "copy":
            x_pred = det.copy_forward(x_j, m_j, x_i, m_i)
        else:
            x_j_black, x_i_black = ((orc.zero_robot_region(m_j, x_j), orc.zero_robot_region(m_i, x_i)) if dontcare
                                    else (x_j, x_i))
            if cfg.last_frame_skip:
                skip = None
            m_in = torch.cat([m_j, m_i], 1) if cfg.model_use_future_mask else m_j
            if model == "det":
                x4, curr_skip = det.det_forward(sd, cfg, hidden, x_j_black, m_in, r_j, a_j, skip)
            else:
                r_in = (r_j, r_i) if cfg.model_use_future_robot_state else r_j
                m_next = m_i.repeat(1, 2, 1, 1) if cfg.model_use_future_mask else m_i
                x4, curr_skip, mu, logvar, mu_p, logvar_p = orc.svg_forward(
                    sd, cfg, hidden, x_j_black, m_in, r_in, None, a_j, x_i_black, m_next, r_i, None, skip,
                    force_use_prior=True, eps_prior=eps[i - 1][0], eps_post=eps[i - 1][1])
            x_pred = orc.composite(x4, x_j)
            if i <= cfg.n_past:
                skip = curr_skip
        add(losses, f"{prefix}_recon_loss", orc.recon_loss(cfg, x_pred, x_i, tm))
        add(losses, f"{prefix}_robot_loss", orc.robot_mse(x_pred, x_i, tm))
        wm = float(orc.world_mse(x_pred, x_i, tm))
        add(losses, f"{prefix}_world_loss", wm)
        pb, tb = orc.zero_robot_region(tm, x_pred), orc.zero_robot_region(tm, x_i)
        gen.append(pb)
        true.append(tb)
        p = float(orc.psnr(tb.clamp(0, 1), pb.clamp(0, 1)).mean())
        s_ = float(orc.ssim_map(tb, pb).mean())
        add(losses, f"{prefix}_psnr", p)
        add(losses, f"{prefix}_ssim", s_)
        if autoregressive:
            for k in range(i, n_eval - 1):
                add(k_losses, f"{k}_step_psnr", p)
                add(k_losses, f"{k}_step_ssim", s_)
                add(k_losses, f"{k}_step_world_loss", wm)
        if len(all_robots) > 1:
            for r in all_robots:
                idx = torch.from_numpy(robot_name == r)
                add(losses, f"{prefix}_{r}_robot_loss", orc.robot_mse(x_pred[idx], x_i[idx], tm[idx]))
                add(losses, f"{prefix}_{r}_world_loss", orc.world_mse(x_pred[idx], x_i[idx], tm[idx]))
        if model == "svg":
            add(losses, f"{prefix}_kld", orc.kl_loss(mu, logvar, mu_p, logvar_p, bs))
    out = {k: v / (n_eval - 1) for k, v in losses.items()}
    out.update({k: v / float(k[0]) for k, v in k_losses.items()})  # the key's first character (trainer.py:1391)
    out["gen_imgs"], out["true_imgs"] = to_uint8_video(gen), to_uint8_video(true)
    return out


def predict_video(sd, cfg, data, n_eval, eps=None, model="svg", experiment="train_robonet", robot_model=None):
    """`predict_video` (trainer.py:1149-1224).  `eps[w][s]` = the per-step draws of window w, sample s.  Returns
    (best sample's dict, its index, every sample's summed autoreg_world_loss)."""
    num_samples = 3 if (model == "svg" and "finetune" in experiment) else 1
    T = len(data["images"])
    windows = floor(T / n_eval)
    sampled = [dict() for _ in range(num_samples)]
    for w in range(windows):
        s, e = w * n_eval, (w + 1) * n_eval
        batch = {"images": data["images"][s:e], "states": data["states"][s:e], "actions": data["actions"][s:e - 1],
                 "masks": data["masks"][s:e], "robot": data["robot"]}
        batch["pred_masks"] = batch["masks"]
        if "finetune" in experiment:
            batch["states"], batch["pred_masks"] = robot_model.predict_batch(batch)
        for n in range(num_samples):
            out = predict_snippet(sd, cfg, batch, n_eval, None if eps is None else eps[w][n], model)
            for k, v in out.items():
                if k in ("true_imgs", "gen_imgs"):
                    sampled[n].setdefault(k, []).append(v)
                else:
                    sampled[n][k] = sampled[n].get(k, 0.0) + v
    world = [s_.get("autoreg_world_loss", 0.0) for s_ in sampled]
    order = list(range(num_samples))
    if model == "svg":
        order.sort(key=lambda n: sampled[n]["autoreg_world_loss"])
    best = sampled[order[0]]
    for k in best:
        if k not in ("true_imgs", "gen_imgs"):
            best[k] /= windows
    return best, order[0], world


def frame_differences(got, want):
    """(largest absolute difference, share of differing elements) of two uint8 videos."""
    d = np.abs(np.asarray(got).astype(np.int16) - np.asarray(want).astype(np.int16))
    return int(d.max()), float((d != 0).mean())


def assert_frames_close(got, want):
    """The frame criterion: every element within 1, at most 2.55 % of them different (a frame error inside the 1e-4
    parity gate moves 255 x across an integer with at most that probability)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    worst, share = frame_differences(got, want)
    print(f"frames: max |d| {worst}, differing share {share:.2e}")
    assert worst <= 1 and share <= FRAME_SHARE, (worst, share)
