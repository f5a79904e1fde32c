"""Time of `PredictionTrainer._eval_video(data, autoregressive=True)` on the deployed evaluation shape (g 256, z 64,
`--lstm_group_norm True`, 48x64, batch 16, n_eval 6, robot-aware flags, `finetune_locobot`; synthetic loader, one window
per call, freshly initialised weights), in ONE process, alternating:

  best3_batched     : `--eval_best_of_three True`, the three samples as one batch of 48 videos, one `rac_eval_frames`
                      launch per predicted frame
  best3_sequential  : the same with RAC_PREDICT_BATCH_SAMPLES=0 (three S = 1 passes through the same scoring code)
  three_plain_passes: what three samples cost without this path -- the flag off and `_eval_video` called three times
                      (the plain `_eval_step`: `rac_recon_loss_fwd`, `rac_psnr_ssim`, per-robot gathers)
  one_plain_pass    : the flag off, one call (what an evaluation costs today)

Each figure is the mean over `--calls` calls of a host clock around calls that end in a device synchronise, after
`--warmup` calls, in `--rounds` alternating rounds.  Also counted, per predicted frame of one call: the metric entry
points of the C ABI that were called (`rac_recon_loss_fwd` is two kernels, the others one; the torch kernels of the
plain path's `mean`, index gathers and `contiguous` are not counted).  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_eval_best3.py --calls 10 --warmup 3 --rounds 3 --out profiles/eval_best3_bench.json
"""
import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import export_videos  # noqa: E402  (build, batches: the trainer on the synthetic test loader)
from robot_aware_control_amd import _lib, config as C, ops  # noqa: E402

FLAGS = ("--wandb False --data_root synthetic --model svg --g_dim 256 --z_dim 64 --lstm_group_norm True "
         "--image_height 48 --image_width 64 --batch_size 16 --test_batch_size 16 --n_past 1 --n_future 5 --n_eval 6 "
         "--video_length 6 --reconstruction_loss dontcare_l1 --last_frame_skip True --action_dim 5 --robot_dim 5 "
         "--data_threads 0 --model_use_robot_state True --model_use_mask True --model_use_future_mask True "
         "--model_use_future_robot_state True --experiment finetune_locobot --log_dir /tmp/rac_bench_eval_best3")
METRIC_CALLS = ("rac_eval_frames", "rac_recon_loss_fwd", "rac_psnr_ssim", "rac_kl_fwd")


class counted_calls:
    """Within: every C ABI call by name (ops and metrics reach `_lib.call` through their own names)."""

    def __enter__(self):
        self.counts, self.orig = collections.Counter(), _lib.call

        def call(name, *args):
            self.counts[name] += 1
            return self.orig(name, *args)
        ops.call = _lib.call = call
        return self.counts

    def __exit__(self, *exc):
        ops.call = _lib.call = self.orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_best3.py times the GPU: no device found")
    argv = FLAGS.split()
    cf = C.create_parser(C.create_env_probe(argv)).parse_args(argv)
    tr, loader = export_videos.build(cf)
    data = next(export_videos.batches(tr, loader))
    data["robot"] = ["sawyer" if b % 2 else "widowx" for b in range(len(data["robot"]))]  # a mixed batch: R = 2

    def run(best3, batched, passes):
        cf.eval_best_of_three = best3
        os.environ["RAC_PREDICT_BATCH_SAMPLES"] = "1" if batched else "0"
        for _ in range(passes):
            tr._eval_video(data, autoregressive=True)

    variants = [("best3_batched", (True, True, 1)), ("best3_sequential", (True, False, 1)),
                ("three_plain_passes", (False, True, 3)), ("one_plain_pass", (False, True, 1))]

    def timed(v, calls, warm):
        for _ in range(warm):
            run(*v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            run(*v)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    old = os.environ.get("RAC_PREDICT_BATCH_SAMPLES")
    try:
        ms = {name: [] for name, _ in variants}
        for rnd in range(args.rounds):
            for name, v in variants:
                ms[name].append(timed(v, args.calls, args.warmup if rnd == 0 else 1))
        frames = cf.n_eval - 1
        launches = {}
        for name, v in variants:
            with counted_calls() as counts:
                run(*v)
            launches[name] = {k: round(counts[k] / frames, 2) for k in METRIC_CALLS if counts[k]}
    finally:
        if old is None:
            os.environ.pop("RAC_PREDICT_BATCH_SAMPLES", None)
        else:
            os.environ["RAC_PREDICT_BATCH_SAMPLES"] = old
    out = {"config": "svg g 256 z 64 GroupNorm cell, 48x64, batch 16, n_eval 6, robot-aware, finetune_locobot, 2 robots",
           "calls": args.calls, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "ms_per_eval_video": {k: {"mean": round(sum(v) / len(v), 3), "rounds": [round(x, 3) for x in v]}
                                 for k, v in ms.items()},
           "metric_abi_calls_per_frame": launches}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
