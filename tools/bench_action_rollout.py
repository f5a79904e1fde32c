"""The action-sweep probe (robot_aware_control_amd/action_rollout.py) against the reference script's structure, on the
same build and in ONE process.

Deployed model (g 256, --lstm_group_norm True, 48 x 64, robot-aware inputs, dontcare_l1; random weights: the time does not
depend on them), b = 10 videos, 5 sweeps (recorded, x and y by +-2 cm) x 3 samples x 5 frames.

  batched    : `action_rollout.probe` without the file writes -- one pass over S G b = 150 videos, one
               `rac_action_rollout_sheet` launch, one copy of the sheets (and one of the table) to the host
  sequential : what src/prediction/test_action_rollout.py does -- S G = 15 rollouts of b videos one after the other
               (`action_rollout.rollout` on one sweep and one sample: the same per-step ops), each sweep's sheets
               composed with torch ops (a canvas of ones, the panels copied in, clamp, * 255, uint8) and copied to the
               host sweep by sweep; no response table, which the reference does not have

Both forms read the same prior noise, so their sheets are equal; that is asserted once, outside the timed calls.  The
two alternate over `--rounds` timed pairs after `--warmup` untimed ones, a host clock around each call (each ends in a
device-to-host copy) and a `gc.collect()` in front of it, outside the clock: without it the cyclic collector runs inside
whichever call crosses its threshold, and the batched times of one run spread from 19 to 57 ms.  Reported per form:
every time, the median and the spread (max - min) / median; their ratio; the device-event time of the sheet launch
alone; and, from five further untimed batched calls with a synchronise behind the rollout, how the call splits into the
rollout and the launch plus the copies.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_action_rollout.py --out profiles/action_rollout_bench.json
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from robot_aware_control_amd import action_rollout as ar  # noqa: E402
from robot_aware_control_amd import ops  # noqa: E402
from robot_aware_control_amd import synthetic as syn  # noqa: E402
from robot_aware_control_amd.model import SVGConvModel  # noqa: E402


def summary(ms):
    med = statistics.median(ms)
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def torch_sheets(x, gen_s):
    """One sweep's sheets (L, b H, (1 + G) W + G, 3) uint8 with torch ops: `x` (L, b, 3, H, W), `gen_s` (G, L, b, 3, H, W)."""
    G, L, b, _, H, W = gen_s.shape
    canvas = torch.ones((L, b, 3, H, (1 + G) * W + G), device=x.device)
    for p, panel in enumerate([x] + list(gen_s)):
        canvas[..., p * (W + 1):p * (W + 1) + W] = panel
    grid = canvas.permute(0, 1, 3, 4, 2).reshape(L, b * H, (1 + G) * W + G, 3)
    return (grid.clamp(0, 1) * 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--videos", type=int, default=10)
    ap.add_argument("--video_len", type=int, default=5)
    ap.add_argument("--nsample", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_action_rollout.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    b, L, G = args.videos, args.video_len, args.nsample
    cf = bench.namespace(dev, g_dim=256, lstm_group_norm=True, image_height=48, batch_size=b, n_future=L - 1)
    model = SVGConvModel(cf)
    model.eval()
    H, W = cf.image_height, cf.image_width
    data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in syn.synth_video(seed=3, T=L, B=b, H=H, W=W).items()}
    names, sets = ar.sweep_actions(data["actions"])
    S = len(names)
    noise = torch.randn(L - 1, G * b, cf.z_dim, H // 8, W // 8, device=dev)

    def source_for(rows):  # step k's draw, for the rows of one sample or of all
        state = {"k": 0}

        def source(shape):
            e = noise[state["k"]][rows]
            state["k"] += 1
            assert tuple(e.shape) == tuple(shape), (e.shape, shape)
            return e
        return source

    def batched(phases=None):
        gc.collect()  # (the other form's garbage is not this call's cost)
        t0 = time.perf_counter()
        model.eps_source = source_for(slice(None))
        gen = ar.rollout(model, cf, data, sets, L, G)
        if phases is not None:  # the untimed calls behind the rounds: where the time goes
            torch.cuda.synchronize()
            phases.append((time.perf_counter() - t0) * 1e3)
        sheets, response = ops.action_rollout_sheet(data["images"], gen, 0)
        host = sheets.cpu().numpy()
        table = response.cpu().numpy()
        return (time.perf_counter() - t0) * 1e3, host, table, gen

    def sequential():
        gc.collect()
        t0 = time.perf_counter()
        host = []
        for s in range(S):
            samples = []
            for g in range(G):
                model.eps_source = source_for(slice(g * b, (g + 1) * b))
                samples.append(ar.rollout(model, cf, data, sets[s:s + 1], L, 1)[0, 0])
            host.append(torch_sheets(data["images"][:L], torch.stack(samples)).cpu().numpy())
        return (time.perf_counter() - t0) * 1e3, np.stack(host)

    ms = {"batched": [], "sequential": []}
    for i in range(args.warmup + args.rounds):
        tb, sheets_b, table, gen = batched()
        ts, sheets_s = sequential()
        if i >= args.warmup:
            ms["batched"].append(tb)
            ms["sequential"].append(ts)
    rollout_ms, total_ms = [], []
    for _ in range(5):
        total_ms.append(batched(rollout_ms)[0])
    model.eps_source = None
    assert np.array_equal(sheets_b, sheets_s), "the two forms drew different sheets"
    assert np.all(table[0] == 0) and np.all(np.isfinite(table)) and np.all(table[1:, :, 1:] > 0)

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = 20
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        ops.action_rollout_sheet(data["images"], gen, 0)
    end.record()
    end.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "model": "svg g 256 z 64, --lstm_group_norm True, robot-aware, dontcare_l1",
           "frame_HW": [H, W], "videos": b, "sweeps": S, "samples": G, "frames": L, "rounds": args.rounds,
           "warmup": args.warmup, "batched": summary(ms["batched"]), "sequential": summary(ms["sequential"]),
           "sequential_over_batched": round(statistics.median(ms["sequential"]) / statistics.median(ms["batched"]), 4),
           "batched_phases": {"rollout_to_sync_ms": [round(x, 3) for x in rollout_ms],
                              "whole_call_ms": [round(x, 3) for x in total_ms]},
           "sheet_launch_ms": round(start.elapsed_time(end) / calls, 4), "sheet_bytes": int(sheets_b.nbytes),
           "gen_bytes": int(gen.numel() * 4), "sheets_equal": True,
           "response_mean_per_sweep": {n: float(table[s].mean()) for s, n in enumerate(names)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
