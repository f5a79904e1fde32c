"""Per-step time of `rac_predict_frames` against the chain it replaces in `_predict_video`, in ONE process, alternating:

  fused : ops.predict_frames -- composite + both blacked uint8 frames into the device-side video buffer (the one copy
          to the host happens once per call, outside the step: timed separately as `d2h_video`)
  chain : ops.Composite + two ops.ZeroRegion + two `(255 * x).permute(0, 2, 3, 1).cpu().numpy().astype(np.uint8)`
          (what the reference's step does with ATen, trainer.py:1317-1318, 1351-1355, 1398-1407, here on this
          package's kernels)

on the deployed evaluation shape: n = 48 images (3 samples x batch 16) of 48 x 64, n_eval 6.  A host clock around
`--iters` steps that end in a device synchronise, after `--warmup`; `--rounds` alternating rounds.  Prints one JSON line.

    python tools/bench_predict_frames.py --iters 200 --warmup 20 --rounds 3
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from robot_aware_control_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict_frames.py times the GPU: no device found")
    dev = torch.device("cuda:0")
    S, B, H, W, T = args.samples, args.batch, args.height, args.width, args.steps
    n = S * B
    g = torch.Generator(device="cpu").manual_seed(3)
    x4 = torch.rand((n, H, W, 4), generator=g).to(dev)
    prev = torch.rand((n, 3, H, W), generator=g).to(dev)
    target = torch.rand((B, 3, H, W), generator=g).to(dev)
    mask = (torch.rand((B, 1, H, W), generator=g) < 0.2).float().to(dev)
    mask_n = mask.repeat(S, 1, 1, 1)
    frames = torch.empty(((S + 1) * B, T, H, W, 3), dtype=torch.uint8, device=dev)
    gen_u8, true_u8 = frames[:n], frames[n:]

    def fused():
        ops.predict_frames(x4, prev, target, mask, gen_u8, true_u8, 1)

    def chain():
        pred = ops.Composite.apply(x4, prev)
        pb = ops.ZeroRegion.apply(pred, mask_n)
        tb = ops.ZeroRegion.apply(target, mask)
        (255 * pb).permute(0, 2, 3, 1).cpu().numpy().astype(np.uint8)
        (255 * tb).permute(0, 2, 3, 1).cpu().numpy().astype(np.uint8)

    def d2h_video():
        frames.cpu().numpy()

    def timed(fn, iters, warm):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    us = {"fused": [], "chain": [], "d2h_video": []}
    with torch.no_grad():
        for rnd in range(args.rounds):
            for name, fn in (("fused", fused), ("chain", chain), ("d2h_video", d2h_video)):
                us[name].append(timed(fn, args.iters, args.warmup if rnd == 0 else 5))
    moved = n * H * W * (16 + 12 + 12 + 4 + 3) + B * H * W * (12 + 3)  # bytes the fused launch reads and writes
    out = {"shape": f"{S} x {B} images of {H} x {W}, {T} steps in the video buffer", "iters": args.iters,
           "device": torch.cuda.get_device_name(0), "fused_bytes": moved,
           "us_per_step": {k: {"mean": round(sum(v) / len(v), 2), "rounds": [round(x, 2) for x in v]} for k, v in us.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
