"""Cost of `--debug_cem True` in one CEM iteration of the deployed planner, in ONE process.

The planner is the one `bench.py` times as `side.deployed_cem`: this tool runs `bench.bench_cem(deployed=True)` for one
iteration and takes the configuration, model, policy arguments and planning problem that call built (nothing of it is
restated here; `--cem-candidates` / `--cem-batch` are bench.py's flags with bench.py's defaults).

  off : `CEMPolicy._get_rollouts` of a policy built with `debug_cem=False`, then a device synchronise
  on  : the same with `debug_cem=True` -- every iteration asks the sampler for `ret_obs`, as the reference does

The two alternate over `--repeats` timed pairs after `--warmup` untimed ones; a host clock around each call.  Reported
per form: every time, the median and the spread (max - min) / median.  Also: `last_obs_d2h_bytes` / `_copies` of the
`on` form, the device-event time of the rac_cem_rollout_sheet launch (elites' frames alone; sheet alone), and the host
time of the last iteration's plot (sheet launch, copy, labels, GIF file).  On a tree without the device frame store
those three read null.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_debug_cem.py --out profiles/debug_cem_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def deployed_planner(args, dev):
    """Everything `bench.bench_cem(deployed=True)` builds, recorded while it runs one iteration."""
    got = {}
    real = bench.CEMPolicy

    class Recorder(real):
        def __init__(self, cf, model, **kw):
            super().__init__(cf, model, **kw)
            got.update(cf=cf, model=model, kw=kw)
            inner = self.traj_sampler.generate_model_rollouts

            def record(actions, start, goal, **k):
                got.update(actions=actions, start=start, goal=goal)
                return inner(actions, start, goal, **k)
            self.traj_sampler.generate_model_rollouts = record

    bench.CEMPolicy = Recorder
    try:
        ba = argparse.Namespace(cem_candidates=args.cem_candidates, cem_batch=args.cem_batch, cem_iters=1, cem_warmup=0,
                                group_norm=False, no_cem_shared_start=False, full=False)
        line = bench.bench_cem(ba, dev, 0, 1, False, deployed=True)
    finally:
        bench.CEMPolicy = real
    got["bench_s_per_iter"] = line["s_per_iter"]
    return got


def summary(ms):
    med = statistics.median(ms)
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def event_ms(fn, calls=20, warmup=3):
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cem-candidates", type=int, default=1000)
    ap.add_argument("--cem-batch", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_debug_cem.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    p = deployed_planner(args, dev)
    log_dir = tempfile.mkdtemp(prefix="rac_debug_cem_")
    pols = {}
    for name, flag in (("off", False), ("on", True)):
        cf = argparse.Namespace(**dict(vars(p["cf"]), debug_cem=flag, log_dir=log_dir))
        pols[name] = bench.CEMPolicy(cf, p["model"], **p["kw"])
        pols[name].ep_num, pols[name].step = 0, 0
    actions, start, goal = p["actions"], p["start"], p["goal"]

    def iteration(name):
        t0 = time.perf_counter()
        ro = pols[name]._get_rollouts(actions, start, goal, None, False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ro

    ms = {"off": [], "on": []}
    for i in range(args.warmup + args.repeats):
        for name in ("off", "on"):
            t, ro = iteration(name)
            if i >= args.warmup:
                ms[name].append(t)
            last = ro
    assert np.all(np.isfinite(last["sum_cost"])) and len(last["obs"]) == p["cf"].topk
    sampler = pols["on"].traj_sampler
    res = {"device": torch.cuda.get_device_name(0), "candidates": int(actions.shape[0]), "steps": int(actions.shape[1]),
           "frame_HW": [p["cf"].image_height, p["cf"].image_width], "topk": p["cf"].topk, "repeats": args.repeats,
           "warmup": args.warmup, "bench_deployed_cem_ms_per_iteration": round(p["bench_s_per_iter"] * 1e3, 3),
           "debug_cem_off": summary(ms["off"]), "debug_cem_on": summary(ms["on"]),
           "on_over_off": round(statistics.median(ms["on"]) / statistics.median(ms["off"]), 4),
           "last_obs_d2h_bytes": getattr(sampler, "last_obs_d2h_bytes", None),
           "last_obs_d2h_copies": getattr(sampler, "last_obs_d2h_copies", None),
           "sheet_launch_ms": None, "plot_ms": None}
    if hasattr(sampler, "rollout_sheet"):
        rows = [int(i) for i in last["topk_idx"]]
        H, W = res["frame_HW"]
        start_u8 = torch.from_numpy(np.ascontiguousarray(start.img)).to(dev)
        goal_u8 = torch.from_numpy(np.stack(goal.imgs)).to(dev)
        res["sheet_launch_ms"] = {
            "obs_only": round(event_ms(lambda: sampler._sheet_launch(rows, want_obs=True)), 4),
            "sheet_only": round(event_ms(lambda: sampler._sheet_launch(rows, start_u8, goal_u8, want_sheet=True)), 4)}
        opt = actions[0, :, :2].clone()
        plot = []
        for _ in range(3):
            ro = pols["on"]._get_rollouts(actions, start, goal, opt, False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pols["on"]._plot_model_rollouts(ro, actions, start, goal, opt)
            plot.append((time.perf_counter() - t0) * 1e3)
        res["plot_ms"] = summary(plot)
        res["gif_bytes"] = os.path.getsize(pols["on"].last_gif)
        res["store_bytes"] = int(sampler._obs_store.numel() * 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
