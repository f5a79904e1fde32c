"""Time of the device mask renderer, in ONE process, for the two MJCF fixtures of tests/golden/mjcf
(wx250s: 12 460 triangles, native 48 x 64; widowx: 3 220 triangles, native 64 x 85), cameras posed through
`set_opencv_camera_pose` from the files' own camera poses, seeded joint positions uniform in +-0.8 rad:

  render        : `MjcfMaskRenderer.render` at P = 80 poses (a 16 x 5 training window) and P = 15 000 (1000 CEM
                  candidates x 15 steps), written at the native size and at 48 x 64.  Device-event time around `--calls`
                  back-to-back calls (`--big_calls` at P = 15 000) after a warm-up: a CALL time, host cost included.
  predict_batch : `LearnedRobotModel.predict_batch` on a T = 5, B = 16 window with random-weight models, (a) on the device
                  route and (b) on the host route fed by a STUB renderer that hands back ready-made native-size masks -- so
                  (b) is the host route's floor: its copies, its per-sample resize and its upload, and no rendering at all.
                  A host clock around calls that each end in a device synchronise.

The forms alternate over `--rounds` rounds.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_mask_render.py --out profiles/mask_render_bench.json
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

from robot_aware_control_amd import mjcf  # noqa: E402
from robot_aware_control_amd.render import MjcfMaskRenderer  # noqa: E402
from robot_aware_control_amd.robot_model import GripperStatePredictor, JointPosPredictor, LearnedRobotModel  # noqa: E402

FIXTURES = {"wx250s": os.path.join(ROOT, "tests", "golden", "mjcf", "wx250s", "model.xml"),
            "widowx": os.path.join(ROOT, "tests", "golden", "mjcf", "widowx", "robot.xml")}


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


def summary(ms):
    return {k: {"mean": round(sum(v) / len(v), 4), "rounds": [round(x, 4) for x in v]} for k, v in ms.items()}


class Stub:
    """Ready-made masks through the reference environments' call: what is left of the host route is its copies."""

    def __init__(self, masks):
        self.masks = masks

    def generate_masks(self, qpos_data, width=None, height=None):
        return self.masks[:len(qpos_data)]


def posed(which, dev):
    model = mjcf.load_mjcf(FIXTURES[which])
    r = MjcfMaskRenderer(model, device=dev)
    cam = model.cameras["main_cam"]
    ext = np.eye(4)
    ext[:3, :3], ext[:3, 3] = mjcf.quat_to_mat(cam.quat), cam.pos   # the files store the pose OpenCV-style
    r.set_opencv_camera_pose("main_cam", ext)
    return r


def bench(which, args, dev):
    r = posed(which, dev)
    H, W = r._img_height, r._img_width
    rs = np.random.RandomState(3)
    ms, mean_set = {}, {}
    shapes = [(80, args.calls), (15000, args.big_calls)]
    qs = {P: torch.tensor(rs.uniform(-0.8, 0.8, (P, 6)), dtype=torch.float32, device=dev) for P, _ in shapes}
    forms = [(f"P{P}_{'native' if hw == (H, W) else '48x64'}", P, calls, hw) for P, calls in shapes
             for hw in ((H, W), (48, 64))]
    forms = list(dict((f[0], f) for f in forms).values())               # wx250s: native IS 48 x 64
    for name, P, calls, hw in forms:
        ms[name] = []
        mean_set[name] = round(float(r.render(qs[P], out_hw=hw).mean()) * hw[0] * hw[1], 1)
    # predict_batch, T = 5 and B = 16, frames 48 x 64
    T, B = 5, 16
    cf = argparse.Namespace(robot_joint_dim=6, robot_dim=5, action_dim=5, image_height=48, image_width=64,
                            experiment="finetune_widowx", preprocess_action="raw", model_use_heatmap=False)
    torch.manual_seed(0)
    joint, gripper = JointPosPredictor(cf).to(dev), GripperStatePredictor(cf).to(dev)
    data = dict(qpos=torch.tensor(rs.uniform(-0.5, 0.5, (T + 1, B, 6)), dtype=torch.float32),
                states=torch.tensor(rs.uniform(0, 1, (T + 1, B, 5)), dtype=torch.float32),
                actions=torch.tensor(rs.uniform(-1, 1, (T, B, 5)), dtype=torch.float32),
                masks=torch.zeros(T + 1, B, 1, 48, 64), folder=["cam0"] * B)
    device_model = LearnedRobotModel(cf, joint, gripper, renderers={"cam0": r})
    ready = r.generate_masks(rs.uniform(-0.5, 0.5, (T, 6)))
    stub_model = LearnedRobotModel(cf, joint, gripper, renderers={"cam0": Stub(ready)})
    ms["predict_batch_device"], ms["predict_batch_host_stub"] = [], []
    for rnd in range(args.rounds):
        for name, P, calls, hw in forms:
            ms[name].append(event_ms(lambda: r.render(qs[P], out_hw=hw), calls, args.warmup if rnd == 0 else 2))
        ms["predict_batch_device"].append(host_ms(lambda: device_model.predict_batch(data), args.calls, 3))
        ms["predict_batch_host_stub"].append(host_ms(lambda: stub_model.predict_batch(data), args.calls, 3))
    out = summary(ms)
    for name, P, calls, hw in forms:
        out[name]["us_per_pose"] = round(out[name]["mean"] * 1e3 / P, 3)
        out[name]["mean_pixels_set"] = mean_set[name]
    return {"triangles": int(len(r.model.tri)), "links": r.model.n_links, "native_HW": [H, W],
            "depth_buffers": 1 if r.model.tri_robot.all() else 2, "ms_per_call": out,
            "host_stub_over_device": round(out["predict_batch_host_stub"]["mean"] / out["predict_batch_device"]["mean"], 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--big_calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_render.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "big_calls": args.big_calls,
           "rounds": args.rounds, "predict_batch_window_TB": [5, 16],
           "fixtures": {which: bench(which, args, dev) for which in FIXTURES}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
