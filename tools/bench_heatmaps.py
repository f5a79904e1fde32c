"""Time of the end-effector heatmaps of one batch, in ONE process, at the window sizes
(B, T, H, W) = (16, 6, 48, 64) and (16, 31, 48, 64):

  device : `heatmaps.batch_heatmaps` -- the view records packed on the host, their upload (B x 120 bytes) and one
           `rac_eef_heatmaps` launch; states and bounds already on the device, as in the prefetcher.  Device-event time
           around `--calls` back-to-back calls after `--warmup` calls: a CALL time, host cost included, not a kernel time.
           `effective_GBps` is the 4 T B H W bytes written over the call time.
  host   : the route it replaces, in the reference's structure (trainer.py:234-246): per video the states copied to the
           host, the fp64 restatement of `create_heatmaps` in numpy (tests/heatmap_refs.py), then one upload of the
           (T, B, 1, H, W) result; a host clock around `--host_calls` calls, each ending in a device synchronise.

The two forms alternate over `--rounds` rounds.  Cameras and bounds are the golden file's (tests/golden/heatmaps.npz);
states are seeded uniform draws in the unit cube.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_heatmaps.py --out profiles/heatmaps_bench.json
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

from robot_aware_control_amd import heatmaps as hm  # noqa: E402
from tests import heatmap_refs as hr  # noqa: E402

SHAPES = [(16, 6, 48, 64), (16, 31, 48, 64)]


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


def host_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def bench(B, T, H, W, args, golden, table, dev):
    robots = [list(hr.ROBOTS)[b % 4] for b in range(B)]
    folders = [hr.ROBOTS[r][3] for r in robots]
    g = np.random.Generator(np.random.Philox(key=[B, T]))
    states = torch.from_numpy(g.random((T, B, 5), dtype=np.float32)).to(dev)
    low_h = np.stack([golden[f"{r}_low"] for r in robots])
    high_h = np.stack([golden[f"{r}_high"] for r in robots])
    low, high = torch.from_numpy(low_h).to(dev), torch.from_numpy(high_h).to(dev)
    Ks, wTcs = [golden[f"{r}_K"] for r in robots], [golden[f"{r}_wTc"] for r in robots]

    def device():
        return hm.batch_heatmaps(states, low, high, robots, folders, table, H, W)

    def host():
        s = states.cpu().numpy()
        out = np.stack([hr.heatmaps(s[:, b], low_h[b], high_h[b], robots[b], Ks[b], wTcs[b], H, W)[0].astype(np.float32)
                        for b in range(B)], 1)
        return torch.from_numpy(out).to(dev)

    worst = float((device() - host()).abs().max())
    ms = {"batch_heatmaps": [], "host_route": []}
    for rnd in range(args.rounds):
        ms["batch_heatmaps"].append(event_ms(device, args.calls, args.warmup if rnd == 0 else 2))
        ms["host_route"].append(host_ms(host, args.host_calls, 2 if rnd == 0 else 1))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    nbytes = 4 * T * B * H * W
    return {"shape_BTHW": [B, T, H, W], "bytes_written": nbytes, "max_abs_diff": worst,
            "ms_per_call": {k: {"mean": round(mean[k], 4), "rounds": [round(x, 4) for x in v]} for k, v in ms.items()},
            "host_over_device": round(mean["host_route"] / mean["batch_heatmaps"], 1),
            "effective_GBps": round(nbytes / (mean["batch_heatmaps"] * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--host_calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_heatmaps.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    golden = hr.load_golden()
    table = hr.golden_table(golden)
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "host_calls": args.host_calls,
           "rounds": args.rounds, "shapes": [bench(B, T, H, W, args, golden, table, dev) for B, T, H, W in SHAPES]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
