"""Time of the object-movement pass, in ONE process:

  kernel : `ops.video_movement` on a time-first batch of V videos of T frames, against the same batch through the ops
           the pass would otherwise be made of -- per step one `ops.copy_baseline` and one `ops.ReconLoss` (which gives
           a batch mean, not a per-video score) -- at (V, T, H, W) = (16, 31, 64, 64) and (16, 31, 48, 64).  Each figure
           is device-event time around `--calls` back-to-back calls, after `--warmup` calls, the two forms alternating
           over `--rounds` rounds: a CALL time, host launch cost included, not a kernel time.  `effective_GBps` is
           16 V T H W bytes (every frame and every mask once, fp32) over the call time.
  pass   : `movement.score_videos` over a folder of synthetic npz trajectories (tools/make_synthetic_robonet.py,
           64 x 85 stored, 48 x 64 after the image path, 31 frames scored) with 0 and with `--data_threads` loader
           workers, in frames per second by a host clock (every batch ends in a device-to-host copy).

Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_movement.py --out profiles/movement_bench.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import make_synthetic_robonet  # noqa: E402
from robot_aware_control_amd import config as C, movement, ops  # noqa: E402

SHAPES = [(16, 31, 64, 64), (16, 31, 48, 64)]


def event_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def bench_kernel(V, T, H, W, calls, warmup, rounds):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.rand(T, V, 3, H, W, generator=g).to(dev)
    m = (torch.rand(T, V, 1, H, W, generator=g) < 0.3).float().to(dev)

    def fused():
        return ops.video_movement(x, m)

    def composed():
        total = None
        for t in range(1, T):
            pred = ops.copy_baseline(x[t - 1], x[t], m[t])
            world = ops.ReconLoss.apply(pred, x[t], m[t], None, 0, 0.0)[2]
            total = world if total is None else total + world
        return total

    ms = {"video_movement": [], "composed_ops": []}
    for rnd in range(rounds):
        for name, fn in (("video_movement", fused), ("composed_ops", composed)):
            ms[name].append(event_ms(fn, calls, warmup if rnd == 0 else 2))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    nbytes = 16 * V * T * H * W
    return {"shape_VTHW": [V, T, H, W], "bytes": nbytes,
            "ms_per_call": {k: {"mean": round(mean[k], 4), "rounds": [round(x, 4) for x in v]} for k, v in ms.items()},
            "launches_per_call": {"video_movement": 2, "composed_ops": 3 * (T - 1)},
            "composed_over_fused": round(mean["composed_ops"] / mean["video_movement"], 2),
            "effective_GBps": round(nbytes / (mean["video_movement"] * 1e-3) / 1e9, 1)}


def bench_pass(videos, batch, threads, rounds, dev):
    root = tempfile.mkdtemp(prefix="rac_movement_bench_")
    try:
        make_synthetic_robonet.write(root, per_view=videos, length=31, seed=5)
        folder = os.path.join(root, "baxter_views", "left_c0")
        out = {}
        for workers in (0, threads):
            argv = ["--data_root", root, "--video_length", "31", "--n_past", "1", "--n_future", "30", "--image_height", "48",
                    "--image_width", "64", "--action_dim", "5", "--robot_dim", "5", "--batch_size", str(batch),
                    "--data_threads", str(workers)]
            cf = C.create_parser(C.create_env_probe(argv)).parse_args(argv)
            fps = []
            for _ in range(rounds + 1):  # (the first walk warms the file cache and the kernel: not reported)
                t0 = time.perf_counter()
                scores = movement.score_videos(movement.folder_loader(folder, "baxter_left_c0", cf), dev)
                torch.cuda.synchronize()
                fps.append(len(scores) * 31 / (time.perf_counter() - t0))
            out[f"workers_{workers}"] = {"frames_per_s": round(sum(fps[1:]) / rounds, 1), "rounds": [round(f, 1) for f in fps[1:]]}
        return {"videos": videos, "batch_size": batch, "stored": "64x85 uint8", "scored": "31 frames of 48x64", **out}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--data_threads", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_movement.py times the GPU: no device found")
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "rounds": args.rounds,
           "kernel": [bench_kernel(*s, args.calls, args.warmup, args.rounds) for s in SHAPES],
           "score_videos": bench_pass(args.videos, 16, args.data_threads, args.rounds, torch.device("cuda:0"))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
