"""GPU: `rac_video_movement` / `ops.video_movement` (csrc/rac_frame.hip), the one call that gives the copy baseline's world
error of every video of a batch, and what is built on it: `movement.measure_obj_movement`, the table it writes, the
loaders that read the table and `evaluate_obj_movement.compute_metrics`.

Against fp64: `tests/movement_refs.movement_ref`, the header's formula restated in torch, under the rule of
tests/fp64_tools.py (e_gpu <= max(2e-6, 4 e_cpu32), both figures printed, nothing excluded); the world count 0 gives
exactly 0.0.  Layouts, positions and the two load paths of the kernel by `torch.equal`.

Shapes (V, T, H, W) and what they reach in `video_movement_kernel` (256 threads, one quad of 4 pixels per thread and trip):
  (1, 2, 8, 8)     one step; 16 quads: a frame smaller than the workgroup, 3 waves idle
  (3, 5, 21, 35)   H W = 735 is no multiple of 4: the scalar path with a ragged last quad; V no power of two
  (2, 31, 48, 64)  the reference's length on the deployed frame (768 quads: 3 trips)
  (2, 4, 64, 64)   a full vector path (1024 quads: 4 trips of every thread)
  (1, 3, 70, 67)   H W = 4690, scalar: 1173 quads = 4 trips and a ragged fifth, the last quad 2 pixels wide"""
import argparse
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.fp64_tools import F32, F64, Rule, assert_intact, guarded, refused, relerr  # noqa: E402
from tests.movement_refs import expected_order, movement_ref, write_movement_fixture  # noqa: E402

SHAPES = [(1, 2, 8, 8), (3, 5, 21, 35), (2, 31, 48, 64), (2, 4, 64, 64), (1, 3, 70, 67)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def uniform(seed, *shape):
    return torch.from_numpy(np.random.Generator(np.random.Philox(key=[seed, 77])).random(shape, dtype=np.float32))


def video(V, T, H, W, seed=500):
    """Time-first (T, V, 3, H, W) frames in [0, 1]: a base picture per video plus a per-frame change of up to 0.2."""
    base = uniform(seed, 1, V, 3, H, W)
    return (0.8 * base + 0.2 * uniform(seed + 1, T, V, 3, H, W)).contiguous()


def mask_set(V, T, H, W, seed=510):
    """name -> (T, V, 1, H, W) mask: random at 30 %; all zero; the random one with frame 1 of the last video all robot
    (its step 0 has world count 0); the random one with 0.5 in place of 1 (non-binary: still a robot pixel)."""
    rnd = (uniform(seed, T, V, 1, H, W) < 0.3).float()
    one = rnd.clone()
    one[1, V - 1] = 1.0
    return {"random": rnd, "zero": torch.zeros(T, V, 1, H, W), "one_frame_all_robot": one, "non_binary": rnd * 0.5}


def abi_call(ops, x, m, step, score):
    """The C ABI on contiguous time-first batches, outputs where the caller put them."""
    T, V, _, H, W = x.shape
    ops.call("rac_video_movement", ops.ptr(x), 3 * H * W, V * 3 * H * W, ops.ptr(m), H * W, V * H * W, ops.ptr(step),
             ops.ptr(score), V, T, H, W, ops.stream_ptr())


@pytest.mark.parametrize("V,T,H,W", SHAPES)
def test_step_err_and_score_vs_fp64(dev, V, T, H, W):
    from robot_aware_control_amd import ops
    rule = Rule(f"video_movement V{V} T{T} {H}x{W}")
    x = video(V, T, H, W)
    x_d = x.to(dev)
    results = {}
    for mname, mask in mask_set(V, T, H, W).items():
        score64, step64 = movement_ref(x, mask, F64)
        score32, step32 = movement_ref(x, mask, F32)
        mask_d = mask.to(dev)
        sbuf, step = guarded(dev, (V, T - 1))
        cbuf, score = guarded(dev, (V,))
        abi_call(ops, x_d, mask_d, step, score)
        torch.cuda.synchronize()
        assert_intact(sbuf, step, f"{mname} step_err")
        assert_intact(cbuf, score, f"{mname} score")
        rule.check(f"{mname} step_err", step.t().cpu(), step64, step32)
        rule.check(f"{mname} score", score.cpu(), score64, score32)
        # the public wrapper gives the same bits, as (B,) and (T - 1, B)
        o_score, o_step = ops.video_movement(x_d, mask_d)
        assert tuple(o_score.shape) == (V,) and tuple(o_step.shape) == (T - 1, V)
        assert torch.equal(o_score, score) and torch.equal(o_step, step.t())
        # the score is the running fp32 sum of the steps, in order
        run = step[:, 0].clone()
        for k in range(1, T - 1):
            run = run + step[:, k]
        assert torch.equal(run, score), mname
        if mname == "one_frame_all_robot":
            assert float(step[V - 1, 0]) == 0.0 and float(step64[0, V - 1]) == 0.0
        results[mname] = (score.clone(), step.clone())
    for a, b in zip(results["random"], results["non_binary"]):
        assert torch.equal(a, b), "mask 0.5 is a robot pixel like mask 1"
    rule.done()


@pytest.mark.parametrize("V,T,H,W", [(3, 6, 16, 24), (3, 6, 21, 35)])
def test_layouts_give_the_same_bits(dev, V, T, H, W):
    """Time-first, batch-first, a T-slice and a B-slice of a longer batch read in place, and a batch whose storage
    starts one float past 16-byte alignment (the scalar path, at (16, 24) where the aligned batch takes the vector
    path): every one `torch.equal` to the contiguous time-first call on the same videos."""
    from robot_aware_control_amd import ops
    x, m = video(V, T, H, W, seed=520).to(dev), mask_set(V, T, H, W, seed=530)["random"].to(dev)
    score, step = ops.video_movement(x, m)
    again = ops.video_movement(x, m)
    assert torch.equal(again[0], score) and torch.equal(again[1], step), "two calls on the same inputs"
    # batch-first storage
    bf = ops.video_movement(x.transpose(0, 1).contiguous(), m.transpose(0, 1).contiguous(), time_first=False)
    assert torch.equal(bf[0], score) and torch.equal(bf[1], step)
    # a time-first VIEW of batch-first storage, and the other way round
    tv = ops.video_movement(x.transpose(0, 1).contiguous().transpose(0, 1), m.transpose(0, 1).contiguous().transpose(0, 1))
    assert torch.equal(tv[0], score) and torch.equal(tv[1], step)
    # a T-slice: steps 1..2 of the longer batch, and their sum
    ts = ops.video_movement(x[1:4], m[1:4])
    alone = ops.video_movement(x[1:4].contiguous(), m[1:4].contiguous())
    assert torch.equal(ts[1], step[1:3]) and torch.equal(ts[0], alone[0]) and torch.equal(ts[1], alone[1])
    assert torch.equal(ts[0], step[1] + step[2])
    # a B-slice
    bs = ops.video_movement(x[:, 1:3], m[:, 1:3])
    assert torch.equal(bs[0], score[1:3]) and torch.equal(bs[1], step[:, 1:3])
    # one float past 16-byte alignment
    _, xo = guarded(dev, tuple(x.shape), init=x.cpu(), lead=1)
    _, mo = guarded(dev, tuple(m.shape), init=m.cpu(), lead=1)
    assert xo.data_ptr() % 16 == 4 and mo.data_ptr() % 16 == 4 and torch.equal(xo, x)
    off = ops.video_movement(xo, mo)
    assert torch.equal(off[0], score) and torch.equal(off[1], step), "the scalar and the vector path give the same bits"
    # only the mask off alignment, and a frame stride that is no multiple of 4 floats (T-slices of a (T, V, 3 H W + 1) buffer)
    half = ops.video_movement(x, mo)
    assert torch.equal(half[0], score) and torch.equal(half[1], step)
    wide = torch.zeros(T, V, 3 * H * W + 1, device=dev)
    wide[:, :, :3 * H * W] = x.view(T, V, -1)
    odd = ops.video_movement(wide[:, :, :3 * H * W].view(T, V, 3, H, W), m)
    assert torch.equal(odd[0], score) and torch.equal(odd[1], step)
    # frames that are not dense are copied, not misread
    turned = x.permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3)  # the same values, W-major in memory
    assert torch.equal(turned, x) and not turned[0, 0].is_contiguous()
    cl = ops.video_movement(turned, m)
    assert torch.equal(cl[0], score) and torch.equal(cl[1], step)


def test_a_video_depends_on_itself_alone(dev):
    """The bits of video v alone == inside V = 3 at each position."""
    from robot_aware_control_amd import ops
    for V, T, H, W in ((3, 5, 21, 35), (3, 4, 48, 64)):
        x, m = video(V, T, H, W, seed=540).to(dev), mask_set(V, T, H, W, seed=550)["one_frame_all_robot"].to(dev)
        score, step = ops.video_movement(x, m)
        for v in range(V):
            a_score, a_step = ops.video_movement(x[:, v:v + 1], m[:, v:v + 1])
            assert torch.equal(a_score[0], score[v]) and torch.equal(a_step[:, 0], step[:, v]), (H, W, v)
        for order in ([1, 2, 0], [2, 0, 1]):
            idx = torch.tensor(order, device=dev)
            p_score, p_step = ops.video_movement(x[:, idx], m[:, idx])
            assert torch.equal(p_score, score[idx]) and torch.equal(p_step, step[:, idx]), (H, W, order)


def test_bad_arguments_are_refused(dev):
    from robot_aware_control_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, device=dev)
    refused(_lib.RacError, lambda: ops.video_movement(z(1, 2, 3, 8, 8), z(1, 2, 1, 8, 8)), "rac_video_movement: bad args")
    refused(_lib.RacError, lambda: ops.video_movement(torch.zeros(3, 2, 3, 8, 8), torch.zeros(3, 2, 1, 8, 8)), "GPU only")
    refused(_lib.RacError, lambda: ops.video_movement(z(3, 2, 3, 8, 8), torch.zeros(3, 2, 1, 8, 8)), "GPU only")
    refused(_lib.RacError, lambda: ops.video_movement(z(3, 2, 3, 8, 8), z(3, 2, 1, 8, 4)), "video_movement: (T,B,3,H,W)")
    refused(_lib.RacError, lambda: ops.video_movement(z(3, 2, 4, 8, 8), z(3, 2, 1, 8, 8)), "video_movement: (T,B,3,H,W)")
    x, m, step, score = z(3, 2, 3, 8, 8), z(3, 2, 1, 8, 8), z(2, 2), z(2)
    args = lambda **kw: [kw.get("x", ops.ptr(x)), kw.get("ivs", 192), 384, ops.ptr(m), 64, 128, kw.get("step", ops.ptr(step)),
                         ops.ptr(score), kw.get("V", 2), kw.get("T", 3), 8, 8, ops.stream_ptr()]
    for kw in (dict(T=1), dict(V=0), dict(ivs=-192), dict(x=None), dict(step=None)):
        refused(_lib.RacError, lambda kw=kw: ops.call("rac_video_movement", *args(**kw)), "rac_video_movement: bad args")


def test_agrees_with_the_composed_existing_ops(dev):
    """`ops.copy_baseline` + `losses.world_mse_criterion` per video and step, summed as the reference sums them: another
    order of the same sums, so within the rule's bound of each other, max(2e-6, 4 e_cpu32) with e_cpu32 from the fp32
    and fp64 CPU references of the same numbers; and each within the rule of the fp64 reference."""
    from robot_aware_control_amd import losses, ops
    V, T, H, W = 2, 5, 48, 64
    x, m = video(V, T, H, W, seed=560), mask_set(V, T, H, W, seed=570)["random"]
    (score64, step64), (score32, step32) = movement_ref(x, m, F64), movement_ref(x, m, F32)
    x_d, m_d = x.to(dev), m.to(dev)
    score, step = ops.video_movement(x_d, m_d)
    c_step = torch.zeros(T - 1, V, device=dev)
    c_score = torch.zeros(V, device=dev)
    for v in range(V):
        for t in range(1, T):
            pred = ops.copy_baseline(x_d[t - 1, v:v + 1], x_d[t, v:v + 1], m_d[t, v:v + 1])
            c_step[t - 1, v] = losses.world_mse_criterion(pred, x_d[t, v:v + 1], m_d[t, v:v + 1])
            c_score[v] += c_step[t - 1, v]
    rule = Rule("video_movement vs composed ops")
    rule.check("kernel step_err", step, step64, step32)
    rule.check("kernel score", score, score64, score32)
    rule.check("composed step_err", c_step, step64, step32)
    rule.check("composed score", c_score, score64, score32)
    rule.done()
    for name, mine, theirs, r32, r64 in (("step_err", step, c_step, step32, step64), ("score", score, c_score, score32, score64)):
        e, bound = relerr(mine, theirs), max(2e-6, 4 * relerr(r32, r64))
        print(f"[video_movement vs composed ops] {name}: rel {e:.2e} bound {bound:.2e}")
        assert e <= bound, (name, e, bound)


def test_measure_write_load_and_evaluate(dev, tmp_path):
    from robot_aware_control_amd import config as rc
    from robot_aware_control_amd import data
    from robot_aware_control_amd.movement import measure_obj_movement
    from src.prediction.evaluation import evaluate_obj_movement as ev
    root = str(tmp_path / "robonet")
    views = (("baxter", "left_c0"), ("widowx", "widowx1_c0"))
    truth = write_movement_fixture(root, views=views, moving=3, static=3, T=8, h=16, w=21)
    cf, _ = rc.argparser(["--data_root", root, "--model", "copy", "--video_length", "8", "--n_past", "1", "--n_future", "7",
                          "--n_eval", "4", "--image_height", "16", "--image_width", "16", "--action_dim", "4",
                          "--impute_autograsp_action", "False", "--robot_dim", "5", "--batch_size", "4",
                          "--data_threads", "0", "--seed", "3", "--load_movement_info", "True",
                          "--log_dir", str(tmp_path / "logs")])
    cf.device = dev
    # the fp64 reference scores, from the frames the dataset's own image path makes (CPU)
    plain = argparse.Namespace(**{**vars(cf), "load_movement_info": False})
    files = sorted(truth)
    cpu_ds = data.RoboNetDataset(files, ["x"] * len(files), plain)
    items = [cpu_ds[i] for i in range(len(files))]
    assert tuple(items[0]["images"].shape) == (8, 3, 16, 16)
    images, masks = (torch.stack([it[k] for it in items], 1) for k in ("images", "masks"))
    ref = dict(zip(files, movement_ref(images, masks, F64)[0].tolist()))
    ref32 = dict(zip(files, movement_ref(images, masks, F32)[0].tolist()))
    top_static = max(s for f, s in ref.items() if not truth[f])
    low_moving = min(s for f, s in ref.items() if truth[f])
    assert low_moving >= 10 * top_static > 0, "the fixture must separate its halves by 10 x (a condition on the fixture)"
    threshold = float(np.sqrt(top_static * low_moving))
    all_flags = {}
    for robot, view in views:
        folder = os.path.join(root, f"{robot}_views", view)
        mine = sorted(f for f in files if f.startswith(folder + os.sep))
        scores, flags = measure_obj_movement(robot, view, cf, threshold=threshold)
        assert sorted(scores) == mine and len(mine) == 6
        got = torch.tensor([scores[f] for f in mine])
        r64, r32 = torch.tensor([ref[f] for f in mine], dtype=F64), torch.tensor([ref32[f] for f in mine], dtype=F64)
        e, bound = relerr(got, r64), max(2e-6, 4 * relerr(r32, r64))
        print(f"[measure {robot}/{view}] scores vs fp64: e_gpu {e:.2e} bound {bound:.2e}")
        assert e <= bound
        assert {f: flags[f] for f in mine} == {f: ref[f] >= threshold for f in mine} == {f: truth[f] for f in mine}
        with open(os.path.join(folder, "obj_movement.pkl"), "rb") as f:
            table = pickle.load(f)
        assert sorted(table) == mine and all(type(v) is bool for v in table.values()) and dict(table) == dict(flags)
        assert table["not a file of this folder"] is False  # a defaultdict(bool), as the reference pickles
        with open(os.path.join(folder, "obj_movement_scores.json")) as f:
            info = json.load(f)
        assert info["scores"] == scores and info["threshold"] == threshold and info["above_threshold"] == 3
        assert (info["T"], info["H"], info["W"], info["seed"], info["videos"]) == (8, 16, 16, 3, 6)
        assert sorted(os.listdir(folder)) == sorted([os.path.basename(f) for f in mine]
                                                    + ["obj_movement.pkl", "obj_movement_scores.json"])
        with pytest.raises(FileExistsError, match="overwrite"):
            measure_obj_movement(robot, view, cf, threshold=threshold)
        all_flags.update(flags)
    # a lower threshold with overwrite=True flags everything; then the first table is put back
    robot, view = views[0]
    _, low = measure_obj_movement(robot, view, cf, threshold=0.0, overwrite=True)
    assert all(low.values()) and len(low) == 6
    measure_obj_movement(robot, view, cf, threshold=threshold, overwrite=True)
    # --load_movement_info True: the dataset hands the flags out
    ds = data.RoboNetDataset(files, ["x"] * len(files), cf)
    assert [ds[i]["high_movement"] for i in range(len(files))] == [all_flags[f] for f in files]
    # the movement loader: exactly the flagged files, in the reference's order
    flagged = [f for f in files if all_flags[f]]
    loader = data.create_movement_loader(cf)
    assert loader.dataset._traj_names == expected_order(flagged, cf.seed) and len(flagged) == 6
    seen = [p for batch in loader for p in batch["file_path"]]
    assert sorted(seen) == flagged
    # a --model copy evaluation over that loader
    out = ev.compute_metrics(cf)
    assert set(out) == {"test/autoreg_psnr", "test/autoreg_ssim"}
    assert all(np.isfinite(v) for v in out.values()), out
