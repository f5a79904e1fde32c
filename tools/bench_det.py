"""Train-step time of `--model det` at BASELINE configs[1]'s flags (64x64, g 512, bs 16, n_past 1, n_future 5,
robot-aware), in ONE process, alternating:

  det_split : the default path -- the ConvLSTM stored at the padded width (516 -> 576) on the split-precision kernels
  det_exact : the same model with the frame predictor's gate convs (forward, data and weight gradient) on the
              exact-fp32 MFMA kernel, still at the padded width (everything else unchanged)
  svg       : the svg model's step-by-step path (RAC_SEQUENCE_PATH=0) and its default path, for context

Each figure is the mean over `--steps` steps of a host clock around steps that end in a device synchronise, after
`--warmup` steps; the three variants are timed in `--rounds` alternating rounds so that a drift of the box shows.
Prints one JSON line.

    python tools/bench_det.py --steps 10 --warmup 3 --rounds 3
"""
import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the flags of the flagship workload: bench.namespace)
from robot_aware_control_amd import ops, synthetic as syn  # noqa: E402
from robot_aware_control_amd import trainer as trainer_mod  # noqa: E402
from robot_aware_control_amd.trainer import PredictionTrainer  # noqa: E402


def build(dev, model):
    tr = PredictionTrainer(bench.namespace(dev, model=model))
    tr.model.load_state_dict(syn.synth_state_dict(tr.model, seed=11))
    tr.model.train()
    return tr


@contextlib.contextmanager
def patched(module, name, value):
    old = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, old)


def exact_gate_convs(width):
    """Within: ops.split_supported answers False for the gate conv's shape (Cin = 2 a_split, Cout = 4 a_split), so
    ops.LstmCell takes the exact-fp32 kernel for that conv's forward, data gradient and weight gradient."""
    orig = ops.split_supported
    return patched(ops, "split_supported", lambda H, W, k, Cin, Cout, a_split=0: (
        False if (a_split == width and Cin == 2 * width and Cout == 4 * width) else orig(H, W, k, Cin, Cout, a_split)))


def timed(tr, batches, steps, warmup):
    for i in range(warmup):
        tr._train_step(batches[i % 2])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr._train_step(batches[i % 2])
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_det.py times the GPU: no device found")
    dev = torch.device("cuda:0")
    det, svg = build(dev, "det"), build(dev, "svg")
    cf = det._config
    T, B = cf.n_past + cf.n_future, cf.batch_size
    batches = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in syn.synth_video(seed=100 + i, T=T, B=B).items()}
               for i in range(2)]
    gp = det.model.padded_width

    variants = [("det_split", det, contextlib.nullcontext), ("det_exact", det, lambda: exact_gate_convs(gp)),
                ("svg_stepped", svg, lambda: patched(trainer_mod, "SEQUENCE_PATH", False)),
                ("svg", svg, contextlib.nullcontext)]
    ms = {name: [] for name, _, _ in variants}
    for rnd in range(args.rounds):
        for name, tr, ctx in variants:
            with ctx():
                ms[name].append(timed(tr, batches, args.steps, args.warmup if rnd == 0 else 1))
    for tr in (det, svg):
        tr.optimizer.wait_params()
    out = {"config": "64x64, g 512, bs 16, n_past 1, n_future 5, robot-aware, adam", "det_width": det.model.width,
           "det_padded_width": gp, "steps": args.steps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           "ms_per_step": {k: {"mean": round(sum(v) / len(v), 3), "rounds": [round(x, 3) for x in v]} for k, v in ms.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
