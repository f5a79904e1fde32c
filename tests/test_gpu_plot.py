"""GPU: `PredictionTrainer.plot`.  The arrays it hands to `PIL.Image.fromarray` (the GIF encoder quantises colours, so
the file is no reference) against the ground truth and against a prior-driven rollout written out here with
`model.forward_maps`, `ops.Composite` and `ops.ZeroRegion`, fed the same draws.

Tolerance: none.  The frozen path's arithmetic does not depend on the call site, so the bytes are equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import svg_oracle as orc  # noqa: E402
from robot_aware_control_amd import synthetic as syn  # noqa: E402

B, N_PAST, N_FUTURE, H, W = 2, 2, 2, 64, 64  # (64 x 64 frames: 8 x 8 latent maps)
LENGTH = N_PAST + N_FUTURE
RA = dict(model_use_mask=True, model_use_future_mask=True, model_use_robot_state=True)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to_u8(t):
    return (t.clamp(0, 1) * 255).to(torch.uint8)


@torch.no_grad()
def rollout(tr, x, mask, states, ac):
    """One sample column by `plot`'s rules: x[i] is fed while i < n_past, else the prediction; the encoder's skip maps
    are kept only for i <= n_past; under dontcare every frame shown is blacked with its own mask, the first one too --
    otherwise the column shows the frame that is fed next (the ground truth while i < n_past)."""
    from robot_aware_control_amd import ops
    cf = tr._config
    dontcare = "dontcare" in cf.reconstruction_loss or cf.black_robot_input
    tr.model.init_hidden(x.shape[1])
    x_j = x[0]
    frames = [ops.ZeroRegion.apply(x_j.contiguous(), mask[0].contiguous()) if dontcare else x_j]
    skip = None
    for i in range(1, len(x)):
        m_j, m_i = mask[i - 1], mask[i]
        if cf.last_frame_skip:
            skip = None
        m_in = torch.cat([m_j, m_i], 1) if cf.model_use_future_mask else m_j
        r_in = (states[i - 1], states[i]) if cf.model_use_future_robot_state else states[i - 1]
        x4, curr_skip = tr.model.forward_maps(x_j, m_in, r_in, None, ac[i - 1], posterior=False, next_robot=None,
                                              skip=skip, zero_mask=m_j if dontcare else None)[:2]
        x_pred = ops.Composite.apply(x4, x_j.contiguous())
        if i <= cf.n_past:
            skip = curr_skip
        x_j = x[i] if i < cf.n_past else x_pred
        frames.append(ops.ZeroRegion.apply(x_pred, m_i.contiguous()) if dontcare else x_j)
    return torch.stack(frames)


@pytest.mark.parametrize("last_frame_skip,training", [(True, False), (False, True)])
@pytest.mark.parametrize("flags", [dict(reconstruction_loss="dontcare_l1"),
                                   dict(reconstruction_loss="l1", model_use_future_robot_state=True)],
                         ids=["dontcare_l1", "l1"])
def test_plot_frames_equal_a_rollout_written_out(dev, monkeypatch, tmp_path, flags, last_frame_skip, training):
    import PIL.Image
    from tests.test_gpu_predict_video import make_trainer
    cfg = orc.Cfg(g_dim=32, z_dim=8, batch_size=B, n_past=N_PAST, n_future=N_FUTURE, last_frame_skip=last_frame_skip,
                  **RA, **flags)
    tr = make_trainer(cfg, orc.make_weights(cfg, seed=5), dev, plot_dir=str(tmp_path))
    data = syn.synth_video(seed=81, T=LENGTH + 2, B=B, H=H, W=W)
    # one prior draw per step and sample, in the order plot asks for them
    eps = [e for e, _ in syn.synth_eps(seed=910, steps=3 * (LENGTH - 1), B=B, z=cfg.z_dim, h=H // 8, w=W // 8)]

    def source_of(queue):
        def source(shape):
            e = queue.pop(0)
            assert tuple(e.shape) == tuple(shape), (e.shape, shape)
            return e
        return source

    seen = []
    real = PIL.Image.fromarray
    monkeypatch.setattr(PIL.Image, "fromarray", lambda a, *k, **kw: (seen.append(np.array(a)), real(a, *k, **kw))[1])
    queue = list(eps)
    tr.model.eps_source = source_of(queue)
    tr.model.train(training)
    fname = tr.plot(data, 3, "comparison", random_start=False)
    assert not queue and tr.model.training is training               # (d)
    assert fname == str(tmp_path / "comparison_3.gif") and (tmp_path / "comparison_3.gif").stat().st_size > 0
    assert len(seen) == LENGTH and all(a.shape == (B * H, 4 * W, 3) and a.dtype == np.uint8 for a in seen)  # (a)
    got = np.stack(seen).reshape(LENGTH, B, H, 4, W, 3)              # [t, video, row, column block, col, rgb]

    x, mask, states = (data[k][:LENGTH].to(dev, torch.float32) for k in ("images", "masks", "states"))
    ac = data["actions"][:LENGTH - 1].to(dev, torch.float32)
    planes = lambda t: to_u8(t).permute(0, 1, 3, 4, 2).cpu().numpy()  # (t, video, H, W, 3)
    assert np.array_equal(got[:, :, :, 0], planes(x))                # (b)
    tr.model.eval()
    queue = list(eps)
    tr.model.eps_source = source_of(queue)
    for n in range(3):                                               # (c)
        want = planes(rollout(tr, x, mask, states, ac))
        assert np.array_equal(got[:, :, :, 1 + n], want), n
    assert not queue
    assert not np.array_equal(got[-1, :, :, 1], got[-1, :, :, 0])    # a prediction is no copy of the ground truth


def test_plot_of_the_deterministic_model_is_refused(dev, tmp_path):
    from tests.test_gpu_predict_video import make_trainer
    cfg = orc.Cfg(g_dim=32, batch_size=B, n_past=N_PAST, n_future=N_FUTURE, reconstruction_loss="dontcare_l1", **RA)
    tr = make_trainer(cfg, None, dev, model="det", plot_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="det"):            # (e)
        tr.plot(syn.synth_video(seed=81, T=LENGTH, B=B, H=H, W=W), 0, "comparison", random_start=False)
    assert not list(tmp_path.iterdir())
