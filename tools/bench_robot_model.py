"""Times of the learned robot model's fused kernels against the same arithmetic in eager torch on the same GPU.

  rollout_n16_t11    LearnedRobotModel.rollout at N = 16, T = 11 (a finetune window: n_past 2 + n_future 10): one launch
  rollout_n1000_t15  ... at N = 1000, T = 15
  train_step_b16     one RobotPredictionTrainer._train_step at B = 16, n_past 2 + n_future 10 (M = 176 rows per model)

  feed               (`--case feed`) the trainer's data path on a synthetic RoboNet root (tools/make_synthetic_robonet.py:
                     64 training trajectories of 31-33 frames, B = 16, window 31): batches per second of
                     joint_pos_data.DeviceBatches (one rac_joint_batch launch per batch; also the device-event time of a
                     batch), of the host DataLoader at `--data_threads 5` and of the same loader without workers, and `_train_video` steps per second fed
                     each way.  Every rate is over a wall-clock window of `--feed-batches` batches that ends in a
                     synchronise and follows an untimed warm-up pass; the median of `--feed-windows` windows.

The comparison is the restated `nn.Sequential` models of tests/robot_model_oracle.py on the device, looped step by step
as the reference loops them (cat, 4 Linears, 3 ReLUs and an add per model and step; its train step with torch.optim.Adam
and its per-step `.item()` reads) -- without the reference's per-step device-to-host copy of the rollout.

Every figure is the median over `--samples` samples (at least 20) of a device-event interval around `--reps` back-to-back
calls, divided by `--reps`, after `--warmup` untimed calls; the two sides alternate sample by sample so that a drift of
the box shows in both.  The outputs of the two sides are compared on the timed inputs.  Prints one JSON line per case and,
with --out, writes them to a file.

    python tools/bench_robot_model.py --samples 30 --reps 10 --warmup 5 --out profiles/robot_model_bench.json
    python tools/bench_robot_model.py --case feed --out profiles/joint_pos_feed_bench.json
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robot_aware_control_amd.robot_model import LearnedRobotModel  # noqa: E402
from robot_aware_control_amd.robot_trainer import RobotPredictionTrainer  # noqa: E402
from tests import robot_model_oracle as rmo  # noqa: E402

J, R, A = 7, 5, 5


def interval_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def alternate(sides, samples, reps, warmup):
    """{name: sorted per-call times in ms}; one sample of every side per round."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in sides}
    for _ in range(samples):
        for name, fn in sides.items():
            times[name].append(interval_ms(fn, reps))
    return {name: sorted(v) for name, v in times.items()}


def report(case, times, extra):
    row = {"case": case}
    for name, v in times.items():
        row[f"{name}_ms_median"] = round(statistics.median(v), 5)
        row[f"{name}_ms_min"] = round(v[0], 5)
        row[f"{name}_ms_max"] = round(v[-1], 5)
    row["speedup_median"] = round(statistics.median(times["eager"]) / statistics.median(times["hip"]), 3)
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def trainer(dev, log_dir, **data):
    cf = argparse.Namespace(robot_joint_dim=J, robot_dim=R, action_dim=A, n_past=2, n_future=10, n_eval=12,
                            optimizer="adam", lr=1e-4, beta1=0.9, experiment="finetune_widowx", log_dir=log_dir,
                            scheduled_sampling=False, wandb=False, dynamics_model_ckpt=None, device=dev, **data)
    tr = RobotPredictionTrainer(cf)
    tr.joint_model.load_state_dict(rmo.make_weights("joint", J, A, 1))
    tr.gripper_model.load_state_dict(rmo.make_weights("gripper", R, A, 1))
    return tr


def eager_models(dev):
    return (rmo.build(rmo.make_weights("joint", J, A, 1)).to(dev), rmo.build(rmo.make_weights("gripper", R, A, 1)).to(dev))


def rate(step, batches, windows):
    """Median calls per second of `step` over `windows` wall-clock windows of `batches` calls, each ending in a
    synchronise; one untimed window first."""
    out = []
    for w in range(windows + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            step()
        torch.cuda.synchronize()
        if w:
            out.append(batches / (time.perf_counter() - t0))
    return round(statistics.median(out), 2), round(min(out), 2), round(max(out), 2)


def feed_case(dev, args):
    from robot_aware_control_amd import joint_pos_data as jpd
    spec = importlib.util.spec_from_file_location("make_synthetic_robonet", os.path.join(ROOT, "tools",
                                                                                         "make_synthetic_robonet.py"))
    synth = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(synth)
    B, n_train, n_test = 16, 64, 16
    with tempfile.TemporaryDirectory() as root:
        synth.write(root, per_view=n_train + n_test, length=31)
        tr = trainer(dev, os.path.join(root, "log"), data_root=root, video_length=31, impute_autograsp_action=True,
                     image_width=64, seed=0, preprocess_action="raw", data_threads=5, batch_size=B, test_batch_size=B,
                     finetune_num_test=n_test, finetune_num_train=n_train, img_augmentation=False, world_error_dict=None)
        train_loader, _ = jpd.create_loaders(tr._config)
        host_loader, _ = jpd.create_loaders(tr._config)
        feed = jpd.DeviceBatches(train_loader, dev)
        device_gen, host_gen = feed.forever(), jpd.get_batch(host_loader, dev)
        for _ in range(args.warmup):
            next(device_gen)
        torch.cuda.synchronize()
        event_ms = sorted(interval_ms(lambda: next(device_gen), args.reps) for _ in range(args.samples))
        n, w = args.feed_batches, args.feed_windows
        row = {"case": "feed", "B": B, "trajectories": n_train, "window": 31, "data_threads": 5,
               "batches_per_window": n, "windows": w,
               "device_batch_ms_median": round(statistics.median(event_ms), 5), "device_batch_ms_min": round(event_ms[0], 5),
               "device_batch_ms_max": round(event_ms[-1], 5)}
        inline_loader, _ = jpd.create_loaders(argparse.Namespace(**dict(vars(tr._config), data_threads=0)))
        inline_gen = jpd.get_batch(inline_loader, dev)  # no workers: the per-item cost alone, nothing to restart per epoch
        for name, gen in (("device", device_gen), ("host", host_gen), ("host_threads0", inline_gen)):
            row[f"{name}_batches_per_s"] = rate(lambda: next(gen), n, w)
        for name, gen in (("device", device_gen), ("host", host_gen)):
            row[f"{name}_fed_train_videos_per_s"] = rate(lambda: tr._train_video(next(gen)), n, w)
        row["train_steps_per_video"] = 31 // 12
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("kernels", "feed"), default="kernels")
    ap.add_argument("--feed-batches", type=int, default=16, help="batches per timed window of the feed case")
    ap.add_argument("--feed-windows", type=int, default=5)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.samples < 20:
        raise SystemExit("at least 20 timed samples")
    if not torch.cuda.is_available():
        raise SystemExit("bench_robot_model.py times the GPU: no device found")
    dev = torch.device("cuda:0")
    if args.case == "feed":
        rows = [feed_case(dev, args)]
        return write(args, rows)
    tr = trainer(dev, "/tmp/rac_bench_robot_model")
    model = LearnedRobotModel(tr._config, tr.joint_model, tr.gripper_model)
    ej, eg = eager_models(dev)
    rows = []
    for N, T in ((16, 11), (1000, 15)):
        data = rmo.synth_window(7, T + 1, N, J, R, A)
        q0, s0, ac = data["qpos"][0].to(dev), data["states"][0].to(dev), data["actions"].to(dev)
        q, s = model.rollout(q0, s0, ac)
        eq, es = rmo.rollout(ej, eg, q0, s0, ac)
        diff = max(float((q - eq).abs().max()), float((s - es).abs().max()))
        times = alternate({"hip": lambda: model.rollout(q0, s0, ac), "eager": lambda: rmo.rollout(ej, eg, q0, s0, ac)},
                          args.samples, args.reps, args.warmup)
        rows.append(report(f"rollout_n{N}_t{T}", times, {"N": N, "T": T, "max_abs_diff_vs_eager": diff}))
    B = 16
    data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in rmo.synth_window(9, 12, B, J, R, A).items()}
    opt = torch.optim.Adam(list(ej.parameters()) + list(eg.parameters()), lr=1e-4, betas=(0.9, 0.999))
    first = tr._train_step(data)
    first_eager = rmo.train_step(ej, eg, opt, data, 2, 10)
    diff = max(abs(first[k] - first_eager[k]) for k in first)
    times = alternate({"hip": lambda: tr._train_step(data), "eager": lambda: rmo.train_step(ej, eg, opt, data, 2, 10)},
                      args.samples, args.reps, args.warmup)
    rows.append(report("train_step_b16", times, {"B": B, "window": 12, "first_step_loss_abs_diff_vs_eager": diff}))
    write(args, rows)


def write(args, rows):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "samples": args.samples, "reps": args.reps,
                       "warmup": args.warmup, "cases": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
