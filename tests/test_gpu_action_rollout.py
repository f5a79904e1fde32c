"""GPU: the action-sweep probe.  `rac_action_rollout_sheet` against tests/action_rollout_refs.py, `action_rollout.rollout`
against rollouts written out here, and the command line end to end.

Kernel shapes (S, G, L, b, H, W) and what they reach (256 threads, one quad of 4 pixels per thread and trip):
  (1, 1, 1, 1, 1, 4)    one quad: 255 idle threads; a row of 27 bytes; S = 1, so the table is the base sweep alone
  (2, 3, 2, 2, 5, 8)    odd G: a sheet row of 105 bytes, so panels start at every address residue mod 4; 10 quads
  (3, 2, 2, 3, 6, 12)   even G: a row of 114 bytes, rows start at residues 0 and 2, panels 39 bytes apart; b = 3; 18 quads
  (2, 3, 2, 2, 48, 64)  the deployed frame: 768 quads, 3 trips of every thread, 4 image rows per wave
Sheets are compared byte for byte.  The response bound is `refs.response_bound` (derived there from the header's
reduction order, 24 u at the three small shapes and 48 u at 48 x 64, u = 2^-24), relative to the fp64 value of each
entry; the entries the fp64 reference itself gives as NaN or inf (the images that hold a NaN or the infinities) must be
NaN and inf, every other entry is held to the bound.

Rollouts: the frozen path's arithmetic does not depend on what shares a video's batch, so frames are `torch.equal`."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import svg_oracle as orc  # noqa: E402
from robot_aware_control_amd import synthetic as syn  # noqa: E402
from tests import action_rollout_refs as refs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1, 1, 1, 4), (2, 3, 2, 2, 5, 8), (3, 2, 2, 3, 6, 12), (2, 3, 2, 2, 48, 64)]
SPECIAL = np.concatenate([np.array([0.0, 1.0, 1.0 - 2.0 ** -24, -0.5, 1.5, -1e30, 1e30, np.inf, -np.inf], np.float32),
                          (np.arange(256, dtype=np.float32) / np.float32(255.0))])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def kernel_inputs(shape):
    """(big, truth view, gen): `truth` = big[1:1 + L, 1:1 + b] of a (L + 2, b + 2, 3, H, W) batch, so both strides and
    the base offset matter; uniform values in [-0.25, 1.25) with the SPECIAL values at the head of the first truth and
    the first rollout image (as many as fit), and a NaN in the last truth image and in the last rollout image."""
    S, G, L, b, H, W = shape
    g = np.random.Generator(np.random.Philox(key=[sum(shape), 31]))
    big = (g.random((L + 2, b + 2, 3, H, W), dtype=np.float32) * np.float32(1.5) - np.float32(0.25))
    gen = (g.random((S, G, L, b, 3, H, W), dtype=np.float32) * np.float32(1.5) - np.float32(0.25))
    n = min(len(SPECIAL), 3 * H * W)
    big[1, 1].reshape(-1)[:n] = SPECIAL[:n]
    gen[0, 0, 0, 0].reshape(-1)[:n] = SPECIAL[:n]
    big[L, b].reshape(-1)[-1] = np.nan
    gen[-1, -1, -1, -1].reshape(-1)[-1] = np.nan
    return big, big[1:1 + L, 1:1 + b], gen


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sheets_and_response_against_the_references(dev, shape):
    from robot_aware_control_amd import ops
    S, G, L, b, H, W = shape
    big, truth, gen = kernel_inputs(shape)
    want_sheets = refs.sheet_ref(truth, gen)
    d_big, d_gen = torch.from_numpy(big).to(dev), torch.from_numpy(gen).to(dev)
    d_truth = d_big[1:1 + L, 1:1 + b]
    assert d_truth.data_ptr() != d_big.data_ptr() and d_truth.stride() == d_big.stride()  # a view: offset and strides
    assert d_big.shape[0] > L and d_big.shape[1] > b
    bound = refs.response_bound(H, W)
    runs = {}
    for base in range(S):
        sheets, resp = ops.action_rollout_sheet(d_truth, d_gen, base)
        assert tuple(sheets.shape) == (S, L, b * H, (1 + G) * W + G, 3) and tuple(resp.shape) == (S, G, L, b)
        runs[base] = (sheets.cpu().numpy(), resp.cpu().numpy())
        assert np.array_equal(runs[base][0], want_sheets), base                      # byte for byte
        want = refs.response_ref(gen, base)
        got = runs[base][1]
        assert np.all(got[base] == 0.0)                                                # exactly 0, NaN frame included
        # the image with the NaN gives NaN and the one with the infinities gives inf, here as in fp64
        nan, inf = np.isnan(want), np.isinf(want)
        assert np.array_equal(np.isnan(got), nan) and nan.any() == (S > 1)
        assert np.array_equal(got[inf], want[inf]) and inf.any() == (S > 1)
        fin = ~nan & ~inf
        assert fin.sum() >= got.size - 2 * S
        err = np.abs(got.astype(np.float64)[fin] - want[fin])
        rel = float((err / np.maximum(want[fin], 1e-300)).max())
        print(f"[action_rollout_sheet {shape} base {base}] response rel err {rel:.2e} bound {bound:.2e}")
        assert np.all(err <= bound * want[fin]), (base, rel, bound)
    # two runs are bit-equal; sheet-only, response-only and both together give the same bits
    again_sheets, again_resp = ops.action_rollout_sheet(d_truth, d_gen, 0)
    only_sheets, none = ops.action_rollout_sheet(d_truth, d_gen, None)
    nothing, only_resp = ops.action_rollout_sheet(d_truth, d_gen, 0, sheets=False)
    assert none is None and nothing is None
    bits = lambda a: a.view(np.uint32)
    for s in (again_sheets, only_sheets):
        assert np.array_equal(s.cpu().numpy(), runs[0][0])
    for r in (again_resp, only_resp):
        assert np.array_equal(bits(r.cpu().numpy()), bits(runs[0][1]))
    # a contiguous truth of exactly (L, b) gives the same sheets as the strided view
    assert np.array_equal(ops.action_rollout_sheet(d_truth.contiguous(), d_gen, None)[0].cpu().numpy(), runs[0][0])


def test_rejected_arguments_launch_nothing(dev):
    from robot_aware_control_amd import _lib
    lib = _lib.load()
    S, G, L, b, H, W = 2, 3, 2, 2, 5, 8
    truth = torch.rand(L, b, 3, H, W, device=dev)
    gen = torch.rand(S, G, L, b, 3, H, W, device=dev)
    sheets = torch.full((S, L, b * H, (1 + G) * W + G, 3), 7, dtype=torch.uint8, device=dev)
    resp = torch.full((S, G, L, b), -3.0, device=dev)
    ok = dict(truth=truth.data_ptr(), ts=truth.stride(0), bs=truth.stride(1), gen=gen.data_ptr(), base=0,
              sheets=sheets.data_ptr(), resp=resp.data_ptr(), S=S, G=G, L=L, b=b, H=H, W=W)

    def status(**change):
        a = dict(ok, **change)
        return lib.rac_action_rollout_sheet(a["truth"], a["ts"], a["bs"], a["gen"], a["base"], a["sheets"], a["resp"],
                                            a["S"], a["G"], a["L"], a["b"], a["H"], a["W"], _lib.stream_ptr())
    bad = [dict(S=0), dict(G=0), dict(L=0), dict(b=0), dict(H=0), dict(W=0), dict(W=6), dict(W=-4), dict(truth=None),
           dict(gen=None), dict(sheets=None, resp=None), dict(base=-1), dict(base=S), dict(sheets=None, base=S),
           dict(ts=truth.stride(0) + 2), dict(bs=truth.stride(1) + 1), dict(truth=truth.data_ptr() + 4),
           dict(gen=gen.data_ptr() + 8)]
    for change in bad:
        assert status(**change) != 0, change
        assert b"rac_action_rollout_sheet" in lib.rac_last_error(), change
    torch.cuda.synchronize()
    assert bool((sheets == 7).all()) and bool((resp == -3.0).all())
    assert status(resp=None, base=-1) == 0  # without a response the base is not looked at
    assert status() == 0
    torch.cuda.synchronize()
    assert not bool((sheets == 7).all()) and bool((resp[0] == 0).all()) and bool((resp[1] > 0).all())


# ------------------------------------------------------------------ the rollout
B, H, W, L, NSAMPLE = 2, 64, 64, 3, 2
RA = dict(model_use_mask=True, model_use_future_mask=True, model_use_robot_state=True)
FLAGS = {"ra_dontcare": dict(reconstruction_loss="dontcare_l1", **RA),
         "vanilla_l1": dict(reconstruction_loss="l1", model_use_mask=False, model_use_future_mask=False,
                            model_use_robot_state=False)}


def make(dev, flags, n_past, model="svg", **extra):
    from tests.test_gpu_predict_video import make_trainer
    cfg = orc.Cfg(g_dim=64, z_dim=16, batch_size=B, n_past=n_past, n_future=L - n_past, **flags)
    sd = orc.make_weights(cfg, seed=5) if model == "svg" else None
    return make_trainer(cfg, sd, dev, model=model, **extra)


def batch_and_sets(dev, include_recorded=True):
    from robot_aware_control_amd.action_rollout import sweep_actions
    data = syn.synth_video(seed=81, T=L + 1, B=B, H=H, W=W)
    names, sets = sweep_actions(data["actions"], axes=("x",), include_recorded=include_recorded)
    return data, names, sets  # recorded, x_-20mm, x_20mm: S = 3


def draws(n):
    """One prior draw per step for the n = G b videos of a sweep."""
    return [e for e, _ in syn.synth_eps(seed=910, steps=L - 1, B=n, z=16, h=H // 8, w=W // 8)]


def source_of(queue):
    def source(shape):
        e = queue.pop(0)
        assert tuple(e.shape) == tuple(shape), (e.shape, shape)
        return e
    return source


@torch.no_grad()
def written_out(tr, x, mask, states, ac, eps):
    """One sample column of b videos by the rules of test_action_rollout.py:72-150, with `model.forward_maps`,
    `ops.Composite`, `ops.ZeroRegion` and `ops.copy_baseline` called directly."""
    from robot_aware_control_amd import ops
    cf, model = tr._config, tr.model
    dontcare = "dontcare" in cf.reconstruction_loss or cf.black_robot_input
    queue = list(eps)
    model.eps_source = source_of(queue)
    model.init_hidden(x.shape[1])
    x_j = ops.ZeroRegion.apply(x[0].contiguous(), mask[0].contiguous()) if dontcare else x[0]
    frames, skip = [x_j], None
    for i in range(1, len(x)):
        m_j, m_i = mask[i - 1].contiguous(), mask[i].contiguous()
        if cf.model == "copy":
            x_pred = ops.copy_baseline(x_j, x[i], m_i)
        else:
            if cf.last_frame_skip:
                skip = None
            m_in = torch.cat([m_j, m_i], 1) if cf.model_use_future_mask else m_j
            if cf.model == "det":  # reads x_j as it stands (:119)
                x4, curr_skip = model.forward_maps(x_j, m_in, states[i - 1], ac[i - 1], skip)
            else:
                r_in = (states[i - 1], states[i]) if cf.model_use_future_robot_state else states[i - 1]
                x4, curr_skip = model.forward_maps(x_j, m_in, r_in, None, ac[i - 1], posterior=False, next_robot=None,
                                                   skip=skip, zero_mask=m_j if dontcare else None)[:2]
            x_pred = ops.Composite.apply(x4, x_j.contiguous())
            if i <= cf.n_past:
                skip = curr_skip
            if dontcare:
                x_pred = ops.ZeroRegion.apply(x_pred, m_i)
        x_j = x[i] if i < cf.n_past else x_pred
        frames.append(x_j)
    assert not queue or cf.model != "svg"
    model.eps_source = None
    return torch.stack(frames)


@pytest.mark.parametrize("n_past", [1, 2])
@pytest.mark.parametrize("flags", list(FLAGS), ids=list(FLAGS))
def test_batched_sweeps_equal_each_sweep_alone_and_a_written_out_rollout(dev, flags, n_past):
    from robot_aware_control_amd.action_rollout import rollout
    tr = make(dev, FLAGS[flags], n_past)
    cf = tr._config
    data, names, sets = batch_and_sets(dev)
    S = len(names)
    eps = draws(NSAMPLE * B)
    queue = list(eps)
    tr.model.eps_source = source_of(queue)          # asked for (G b, z, h, w), once per step
    gen = rollout(tr.model, cf, data, sets, L, nsample=NSAMPLE)
    assert not queue and tuple(gen.shape) == (S, NSAMPLE, L, B, 3, H, W) and not tr.model.training
    for s in range(S):                              # the frozen path's batch independence, for this caller
        queue = list(eps)
        tr.model.eps_source = source_of(queue)
        alone = rollout(tr.model, cf, data, sets[s:s + 1], L, nsample=NSAMPLE)
        assert not queue and torch.equal(alone[0], gen[s]), names[s]
    assert not torch.equal(gen[1], gen[2]) and not torch.equal(gen[0], gen[1])  # the model reads its actions
    x, mask, states = (data[k][:L].to(dev, torch.float32) for k in ("images", "masks", "states"))
    for s in (0, 2):
        ac = sets[s][:L - 1].to(dev, torch.float32)
        for g in range(NSAMPLE):
            want = written_out(tr, x, mask, states, ac, [e[g * B:(g + 1) * B] for e in eps])
            assert torch.equal(gen[s, g], want), (names[s], g)
    if flags == "vanilla_l1":
        # without a dontcare loss the script's rules are `plot()`'s: the recorded sweep is what plot's loop gives
        from tests.test_gpu_plot import rollout as plot_rollout
        ac = data["actions"][:L - 1].to(dev, torch.float32)
        for g in range(NSAMPLE):
            tr.model.eps_source = source_of([e[g * B:(g + 1) * B] for e in eps])
            assert torch.equal(gen[0, g], plot_rollout(tr, x, mask, states, ac)), g
    tr.model.eps_source = None


def test_det_has_one_column_and_copy_gives_the_copy_baseline(dev):
    from robot_aware_control_amd import ops
    from robot_aware_control_amd.action_rollout import rollout
    data, names, sets = batch_and_sets(dev)
    x, mask, states = (data[k][:L].to(dev, torch.float32) for k in ("images", "masks", "states"))
    tr = make(dev, FLAGS["ra_dontcare"], 1, model="det")
    gen = rollout(tr.model, tr._config, data, sets, L, nsample=NSAMPLE)
    assert tuple(gen.shape) == (3, 1, L, B, 3, H, W)
    sheets, _ = ops.action_rollout_sheet(data["images"].to(dev), gen, 0)
    assert tuple(sheets.shape) == (3, L, B * H, 2 * W + 1, 3)
    for s in range(3):
        want = written_out(tr, x, mask, states, sets[s][:L - 1].to(dev, torch.float32), [])
        assert torch.equal(gen[s, 0], want), names[s]
    assert not torch.equal(gen[0], gen[1])
    tr = make(dev, FLAGS["vanilla_l1"], 1, model="copy")
    gen = rollout(tr.model, tr._config, data, sets, L, nsample=NSAMPLE)
    assert tuple(gen.shape) == (3, 1, L, B, 3, H, W)
    want = written_out(tr, x, mask, states, None, [])  # rac_copy_baseline's frames, whatever the actions
    assert all(torch.equal(gen[s, 0], want) for s in range(3))


class StubRobotModel:
    """predict_batch -> the states and masks it was built with, for however many samples it is asked."""

    def __init__(self, states, masks):
        self.states, self.masks, self.calls = states, masks, []

    def predict_batch(self, batch):
        self.calls.append(batch)
        return self.states, self.masks


def test_finetune_sweeps_ask_the_robot_model_once(dev):
    from robot_aware_control_amd.action_rollout import rollout
    tr = make(dev, FLAGS["ra_dontcare"], 1, experiment="finetune_locobot")
    cf = tr._config
    data, names, sets = batch_and_sets(dev)
    data["low"], data["high"] = torch.zeros(B, 5), torch.ones(B, 5)
    S = len(names)
    with pytest.raises(NotImplementedError, match="robot model"):
        rollout(tr.model, cf, data, sets, L, nsample=NSAMPLE)
    other = syn.synth_video(seed=7, T=L, B=S * B, H=H, W=W)
    stub = StubRobotModel(other["states"].to(dev), other["masks"].to(dev))
    eps = draws(NSAMPLE * B)
    tr.model.eps_source = source_of(list(eps))
    gen = rollout(tr.model, cf, data, sets, L, nsample=NSAMPLE, robot_model=stub)
    assert len(stub.calls) == 1
    batch = stub.calls[0]
    assert tuple(batch["states"].shape) == (L, S * B, 5) and tuple(batch["masks"].shape) == (L, S * B, 1, H, W)
    assert tuple(batch["low"].shape) == (S * B, 5) and len(batch["robot"]) == S * B
    for s in range(S):  # sweep s in rows [s b, (s + 1) b), with its own actions and the recorded states
        rows = slice(s * B, (s + 1) * B)
        assert torch.equal(batch["actions"][:, rows].cpu(), sets[s][:L - 1])
        assert torch.equal(batch["states"][:, rows].cpu(), data["states"][:L])
    # the rollout runs on what the robot model answered: sweep s on rows [s b, (s + 1) b) of its states and masks
    x = data["images"][:L].to(dev, torch.float32)
    for s in (0, 2):
        rows = slice(s * B, (s + 1) * B)
        want = written_out(tr, x, stub.masks[:, rows], stub.states[:, rows], sets[s][:L - 1].to(dev, torch.float32),
                           [e[:B] for e in eps])
        assert torch.equal(gen[s, 0], want), names[s]
    tr.model.eps_source = None


def test_command_line_writes_the_gifs_and_the_table(dev, tmp_path, capsys):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_robonet as mk
    from robot_aware_control_amd.config import argparser
    from robot_aware_control_amd.trainer import PredictionTrainer
    from src.prediction import test_action_rollout as cli
    root, out, ckpt = str(tmp_path / "data"), str(tmp_path / "out"), str(tmp_path / "model.pt")
    mk.write(root, per_view=4, length=10, seed=1)
    argv = ("--jobname t --wandb False --batch_size 2 --test_batch_size 2 --n_future 2 --n_past 1 --n_eval 4 --g_dim 32 "
            "--z_dim 8 --model svg --reconstruction_loss dontcare_l1 --last_frame_skip True --action_dim 4 "
            "--robot_dim 5 --robot_joint_dim 7 --data_threads 0 --experiment train_robonet --model_use_robot_state True "
            "--model_use_mask True --model_use_future_mask True --video_length 8 --image_height 64 --image_width 64 "
            f"--train_val_split 0.75 --data_root {root} --log_dir {tmp_path / 'log'}").split()
    cfg, _ = argparser(argv)
    cfg.device = dev
    torch.save({"model": PredictionTrainer(cfg).model.state_dict()}, ckpt)
    result = cli.main(argv + ["--dynamics_model_ckpt", ckpt, "--video_len", "4", "--nsample", "2", "--out", out])
    names = ["recorded", "x_-20mm", "y_-20mm", "x_20mm", "y_20mm"]
    assert result.names == names and sorted(os.listdir(out)) == sorted([n + ".gif" for n in names] + ["response.json"])
    assert result.sheets.shape == (5, 4, 2 * 64, 3 * 64 + 2, 3) and result.response.shape == (5, 2, 4, 2)
    for n in names:
        im = Image.open(os.path.join(out, n + ".gif"))
        assert im.n_frames == 4 and im.size == (3 * 64 + 2, 2 * 64), n  # [truth | 2 samples] x 2 videos, 4 frames
    table = json.load(open(os.path.join(out, "response.json")))
    assert table["base"] == "recorded" and table["shape"] == [5, 2, 4, 2] and list(table["sweeps"]) == names
    assert table["sweeps"]["recorded"]["mean"] == 0.0
    for n in names[1:]:
        steps = table["sweeps"][n]["per_step"]
        assert steps[0] == 0.0 and all(v > 0 for v in steps[1:]), (n, steps)  # frame 0 is given; the rest moved
    printed = capsys.readouterr().out
    assert all(n + ":" in printed for n in names)
