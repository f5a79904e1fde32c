"""GPU: `rac_eval_frames` / `ops.eval_frames` (csrc/rac_frame.hip), the one launch that scores every sample of every video
of a predicted frame, and `metrics.table_scalars`, which turns its table into what `_eval_step` logs.

Against fp64: every row assembled from `tests/frame_refs.py` (`recon_out` on the video alone, `psnr_ssim`), under the
rule `tests/test_gpu_frame.py` applies to `rac_recon_loss_fwd` and `rac_psnr_ssim` against the same references
(tests/fp64_tools.py: e_gpu <= max(2e-6, 4 e_cpu32), the robot count exact).  Row independence by `torch.equal`.  The
helper's scalars against `ops.ReconLoss` + `metrics.masked_psnr_ssim` under the same rule's bound.

Shapes (S, B, H, W) and what they reach in `eval_frames_kernel` (64 x 64 output super-tiles, 4 rows per thread):
  (1, 1, 8, 8)    the frame is smaller than the window: every tap row touches padding; 2 of 16 waves live
  (3, 2, 21, 35)  odd sizes: a ragged last row group (21 = 5 x 4 + 1) and 29 idle columns
  (3, 3, 48, 64)  the deployed frame, B no power of two, 12 of 16 waves live
  (2, 2, 64, 64)  a full super-tile
  (1, 1, 70, 67)  a second super-tile on both axes (the loop over tiles and the re-staging barrier)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import frame_refs as fr  # noqa: E402
from tests.fp64_tools import F32, F64, Rule, assert_intact, guarded, relerr  # noqa: E402

SHAPES = [(1, 1, 8, 8), (3, 2, 21, 35), (3, 3, 48, 64), (2, 2, 64, 64), (1, 1, 70, 67)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def uniform(seed, *shape):
    return torch.from_numpy(np.random.Generator(np.random.Philox(key=[seed, 77])).random(shape, dtype=np.float32))


def frames(S, B, H, W, seed=300):
    """(pred (S B, 3, H, W), target (B, 3, H, W)) in [0, 1]; the first sample group stays near the target."""
    target = uniform(seed, B, 3, H, W)
    pred = uniform(seed + 1, S * B, 3, H, W)
    pred[:B] = (target + 0.05 * (uniform(seed + 2, B, 3, H, W) - 0.5)).clamp(0, 1)
    return pred, target


def mask_set(B, H, W, seed=310):
    """name -> mask: random; all zero; all one for the last video (its world count is 0); NULL."""
    rnd = (uniform(seed, B, 1, H, W) < 0.3).float()
    one = rnd.clone()
    one[B - 1] = 1.0
    return {"random": rnd, "zero": torch.zeros(B, 1, H, W), "one_video_all_robot": one, "NULL": None}


def expected_rows(kind, rw, pred, target, mask, dt, ssim_parts):
    """The (S B, 8) table from the references, in dtype `dt`: the per-video loss / robot_mse / world_mse of `recon_out`
    on the video alone times their denominators, and `psnr_ssim`'s sq_err and per-channel map sums (`ssim_parts`)."""
    n, B = pred.shape[0], target.shape[0]
    n3 = 3 * pred.shape[2] * pred.shape[3]
    m = torch.zeros(B, 1, *pred.shape[2:]) if mask is None else mask  # NULL: no robot pixel anywhere
    rows = torch.zeros(n, 8, dtype=dt)
    for v in range(n):
        b = v % B
        loss, robot, world = fr.recon_out(kind, pred[v:v + 1].to(dt), target[b:b + 1].to(dt), m[b:b + 1].to(dt), rw)
        rob_n = 3.0 * float(m[b].sum())
        world_n = n3 - rob_n
        rows[v, 0] = loss * ((world_n + 1) if kind.startswith("dontcare") else n3)
        rows[v, 1], rows[v, 2], rows[v, 3] = robot * (rob_n + 1), world * (world_n + 1), rob_n
    rows[:, 4], rows[:, 5:8] = ssim_parts
    return rows


def ssim_parts(pred, target, mask, dt):
    S = pred.shape[0] // target.shape[0]
    rep = lambda t: t.repeat(S, 1, 1, 1).to(dt)
    smap, se, _ = fr.psnr_ssim(rep(target), pred.to(dt), None if mask is None else rep(mask))
    return se, smap.sum((2, 3))


@pytest.mark.parametrize("S,B,H,W", SHAPES)
def test_rows_vs_fp64(dev, S, B, H, W):
    from robot_aware_control_amd import ops
    rule = Rule(f"eval_frames S{S} B{B} {H}x{W}")
    pred, target = frames(S, B, H, W)
    pred_d, target_d = pred.to(dev), target.to(dev)
    for mname, mask in mask_set(B, H, W).items():
        mask_d = None if mask is None else mask.to(dev)
        parts64, parts32 = ssim_parts(pred, target, mask, F64), ssim_parts(pred, target, mask, F32)
        for kind in fr.LOSS_NAMES:
            for rw in (0.0, 0.5):
                what = f"{mname} {kind} rw{rw}"
                e64 = expected_rows(kind, rw, pred, target, mask, F64, parts64)
                e32 = expected_rows(kind, rw, pred, target, mask, F32, parts32)
                buf, rows = guarded(dev, (S * B, 8))
                out = ops.eval_frames(pred_d, target_d, mask_d, ops.LOSS_KINDS[kind], rw, S, out=rows)
                torch.cuda.synchronize()
                assert out is rows
                assert_intact(buf, rows, what)
                got = rows.cpu()
                assert torch.equal(got[:, 3], e64[:, 3].float()), f"{what}: the robot count is exact"
                for k, col in ((0, "main"), (1, "robot_sq"), (2, "world_sq"), (4, "psnr_sq")):
                    rule.check(f"{what} {col}", got[:, k], e64[:, k], e32[:, k])
                rule.check(f"{what} ssim", got[:, 5:8], e64[:, 5:8], e32[:, 5:8])
                if mname == "one_video_all_robot":
                    v = B - 1  # blacked frames are equal: no squared error, SSIM 1 in every pixel, no world error
                    assert float(got[v, 4]) == 0.0 and float(got[v, 2]) == 0.0 and float(got[v, 3]) == 3 * H * W
                    assert got[v, 5:8].tolist() == [float(H * W)] * 3
                if mname in ("zero", "NULL"):
                    assert float(got[:, 1].abs().max()) == 0.0 and float(got[:, 3].abs().max()) == 0.0
    # NULL is the all-zero mask to the bit
    a = ops.eval_frames(pred_d, target_d, None, 3, 0.5, S)
    b = ops.eval_frames(pred_d, target_d, torch.zeros(B, 1, H, W, device=dev), 3, 0.5, S)
    assert torch.equal(a, b)
    rule.done()


@pytest.mark.parametrize("S,B,H,W", [(3, 2, 21, 35), (3, 3, 48, 64)])
def test_a_row_depends_on_its_video_alone(dev, S, B, H, W):
    """Row s B + b of an S-group launch == the row of an S = 1, B = 1 launch on that video alone == the row after the
    sample groups are permuted == the same row of a second launch, bit for bit."""
    from robot_aware_control_amd import ops
    pred, target = frames(S, B, H, W, seed=320)
    masks = mask_set(B, H, W, seed=330)
    pred_d, target_d = pred.to(dev), target.to(dev)
    for mname in ("one_video_all_robot", "NULL"):
        mask_d = None if masks[mname] is None else masks[mname].to(dev)
        for kind, rw in ((3, 0.5), (0, 0.0)):
            rows = ops.eval_frames(pred_d, target_d, mask_d, kind, rw, S)
            again = ops.eval_frames(pred_d, target_d, mask_d, kind, rw, S)
            assert torch.equal(rows, again), "two launches on the same inputs"
            for v in range(S * B):
                b = v % B
                alone = ops.eval_frames(pred_d[v:v + 1], target_d[b:b + 1], None if mask_d is None else mask_d[b:b + 1],
                                        kind, rw, 1)
                assert torch.equal(alone[0], rows[v]), (mname, kind, v)
            order = [2, 0, 1]
            shuffled = torch.cat([pred_d[s * B:(s + 1) * B] for s in order])
            moved = ops.eval_frames(shuffled, target_d, mask_d, kind, rw, S)
            assert torch.equal(moved, torch.cat([rows[s * B:(s + 1) * B] for s in order])), (mname, kind)
            # S groups of B videos scored as one group of S B videos against the repeated targets
            flat = ops.eval_frames(pred_d, target_d.repeat(S, 1, 1, 1),
                                   None if mask_d is None else mask_d.repeat(S, 1, 1, 1), kind, rw, 1)
            assert torch.equal(flat, rows)


def test_helper_scalars_agree_with_the_existing_kernels(dev):
    """`table_scalars` on the table against `ops.ReconLoss` + `metrics.masked_psnr_ssim` on each sample group's slice,
    and its row subsets against `ReconLoss` on gathered frames (the per-robot losses of a two-robot batch).  Another
    order of the same sums, so not bit-equal: the bound is the fp64 rule's, max(2e-6, 4 e_cpu32), with e_cpu32 from the
    fp32 and fp64 CPU references of the same scalar."""
    from robot_aware_control_amd import metrics, ops
    S, B, H, W = 3, 3, 48, 64
    pred, target = frames(S, B, H, W, seed=340)
    robots = np.array(["sawyer", "widowx", "sawyer"])
    bad = []
    for mname, kind, rw in (("random", "dontcare_l1", 0.5), ("random", "mse", 0.0), ("zero", "dontcare_mse", 0.0),
                            ("random", "l1", 0.0)):
        mask = mask_set(B, H, W, seed=350)[mname]
        pred_d, target_d, mask_d = pred.to(dev), target.to(dev), mask.to(dev)
        k = ops.LOSS_KINDS[kind]
        table = ops.eval_frames(pred_d, target_d, mask_d, k, rw, S).view(S, B, 8)
        got = metrics.table_scalars(table, k, 3 * H * W)
        sub = {r: metrics.table_scalars(table, k, 3 * H * W, index=np.nonzero(robots == r)[0]) for r in set(robots)}
        for s in range(S):
            p, p_d = pred[s * B:(s + 1) * B], pred_d[s * B:(s + 1) * B].contiguous()
            rec = ops.ReconLoss.apply(p_d, target_d, mask_d, None, k, rw)
            psnr, ssim = metrics.masked_psnr_ssim(p_d, target_d, mask_d)
            pairs = [("recon_loss", got["recon_loss"][s], rec[0]), ("robot_loss", got["robot_loss"][s], rec[1]),
                     ("world_loss", got["world_loss"][s], rec[2]), ("psnr", got["psnr"][s], psnr.mean()),
                     ("ssim", got["ssim"][s], ssim)]

            def cpu(dt, p=p, idx=slice(None)):
                out = fr.recon_out(kind, p[idx].to(dt), target[idx].to(dt), mask[idx].to(dt), rw)
                ps, ss = fr.masked_psnr_ssim(p[idx].to(dt), target[idx].to(dt), mask[idx].to(dt))
                return {"recon_loss": out[0], "robot_loss": out[1], "world_loss": out[2], "psnr": ps.mean(), "ssim": ss}
            refs = {"": (cpu(F64), cpu(F32))}
            for r in sorted(set(robots)):
                idx = np.nonzero(robots == r)[0]
                idx_d = torch.from_numpy(idx).to(dev)
                one = ops.ReconLoss.apply(p_d[idx_d].contiguous(), target_d[idx_d].contiguous(),
                                          mask_d[idx_d].contiguous(), None, 0, 0.0)
                pairs += [(f"{r}:robot_loss", sub[r]["robot_loss"][s], one[1]),
                          (f"{r}:world_loss", sub[r]["world_loss"][s], one[2])]
                refs[r] = (cpu(F64, idx=idx), cpu(F32, idx=idx))
            for name, mine, theirs in pairs:
                who, _, key = name.rpartition(":")
                r64, r32 = refs[who][0][key], refs[who][1][key]
                bound = max(2e-6, 4 * relerr(r32.view(1), r64.view(1)))
                e = relerr(mine.view(1), theirs.view(1))
                print(f"[{mname} {kind} s{s}] {name}: table {float(mine):.8g} kernels {float(theirs):.8g} "
                      f"rel {e:.2e} bound {bound:.2e}")
                if not e <= bound:
                    bad.append((mname, kind, s, name, e, bound))
    assert not bad, bad


def test_bad_arguments_are_refused(dev):
    from robot_aware_control_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(_lib.RacError):   # 3 frames over 2 videos
        ops.eval_frames(z(3, 3, 8, 8), z(2, 3, 8, 8), None, 0, 0.0, 1)
    with pytest.raises(_lib.RacError):   # a mask of another batch
        ops.eval_frames(z(2, 3, 8, 8), z(2, 3, 8, 8), z(1, 1, 8, 8), 0, 0.0, 1)
    with pytest.raises(_lib.RacError, match="rac_eval_frames: bad args"):
        ops.call("rac_eval_frames", 4, ops.ptr(z(1, 3, 8, 8)), ops.ptr(z(1, 3, 8, 8)), None, 0.0, ops.ptr(z(1, 8)),
                 1, 1, 8, 8, ops.stream_ptr())
    with pytest.raises(_lib.RacError, match="rac_eval_frames: bad args"):
        ops.call("rac_eval_frames", 0, ops.ptr(z(1, 3, 8, 8)), ops.ptr(z(1, 3, 8, 8)), None, 0.0, ops.ptr(z(1, 8)),
                 0, 1, 8, 8, ops.stream_ptr())
    torch.cuda.synchronize()
