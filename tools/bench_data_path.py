"""What the image half of the data path costs on the host and on the device (`--device_images`, data.py,
csrc/rac_augment.hip).

CPU half (no GPU needed): frames/s of ONE worker thread of `RoboNetDataset.__getitem__` over a
`tools/make_synthetic_robonet.py` tree, host mode against device mode, with and without augmentation, and the collation
of a batch.

GPU half: the time of one `rac_image_pipeline` launch by device events at the training shape (B 16, T 31, augmentation
on; 64x85 -> 48x64 and 64x64 -> 64x64), and loader-fed training: `PredictionTrainer._train_video` on batches from the
device prefetcher with `--img_augmentation True`, `--data_threads` 2 and 5, `device_images` off and on alternated over
three rounds in one process; every timed window ends in a synchronise.  The last line is one JSON record.

`--resident`: the same rounds also time `--device_resident True` (data.ResidentVideos: the split on the device, built
once outside the timed windows) -- training fed by it, the feed alone in batches/s (prefetcher drained, nothing
trained) -- and training on one batch that already lies on the device (no data path at all: the ceiling of any feed).
The record is also written to `--out` (profiles/resident_bench.json).

    python tools/bench_data_path.py --cpu-only
    python tools/bench_data_path.py [--root DIR] [--rounds 3] [--batches 12] [--threads 2,5] [--resident]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_synthetic_robonet as mk  # noqa: E402
from robot_aware_control_amd import _lib  # noqa: E402
from robot_aware_control_amd import data as D  # noqa: E402

T_VIDEO = 31


def data_config(root, **kw):
    d = dict(data_root=root, load_movement_info=False, video_length=T_VIDEO, n_past=1, n_future=5, action_dim=5,
             robot_dim=5, robot_joint_dim=7, impute_autograsp_action=True, image_width=64, image_height=48, seed=0,
             preload_ram=False, preprocess_action="raw", experiment="train_robonet", model_use_heatmap=False,
             train_val_split=0.8, img_augmentation=True, data_threads=0, batch_size=16, test_batch_size=16,
             device_images=False, random_snippet=True)
    d.update(kw)
    return argparse.Namespace(**d)


def cpu_half(root, n_items):
    """frames/s of one thread through __getitem__ (and ms per collated batch of 16)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # as in a DataLoader worker
    cf = data_config(root)
    files, _, labels, _ = D.split_files(cf)
    out = {}
    for augment in (False, True):
        for on in (False, True):
            ds = D.RoboNetDataset(files, labels, cf, augment_img=augment, device_images=on)
            random.seed(0)
            torch.manual_seed(0)
            ds[0]
            t0 = time.perf_counter()
            items = [ds[i % len(ds)] for i in range(n_items)]
            dt = time.perf_counter() - t0
            t0 = time.perf_counter()
            for _ in range(5):
                D.collate(items[:16])
            ct = (time.perf_counter() - t0) / 5
            key = f"{'device' if on else 'host'}_{'aug' if augment else 'plain'}"
            out[key] = {"frames_per_s": round(n_items * T_VIDEO / dt, 1), "ms_per_video": round(1e3 * dt / n_items, 3),
                        "collate_ms_per_batch16": round(1e3 * ct, 3)}
            print(f"cpu  {key:13s} {out[key]['frames_per_s']:9.1f} frames/s/thread  {out[key]['ms_per_video']:7.3f} ms/video  "
                  f"collate {out[key]['collate_ms_per_batch16']:.2f} ms/batch", flush=True)
    torch.set_num_threads(threads)  # the GPU half runs as a trainer process does
    return out


def kernel_half(dev, launches=50):
    """One launch at B 16, T 31, augmentation on (every video its own crop, factors and order), by device events."""
    out = {}
    for (Hs, Ws), (h, w) in (((64, 85), (48, 64)), ((64, 64), (64, 64))):
        g = np.random.Generator(np.random.Philox(key=[3, Hs]))
        random.seed(1)
        torch.manual_seed(1)
        items = []
        for _ in range(16):
            mask = np.zeros((T_VIDEO, Hs, Ws), np.uint8)
            mask[:, 10:30, 20:50] = 1
            items.append({"frames": torch.from_numpy(g.integers(0, 256, (T_VIDEO, Hs, Ws, 3), dtype=np.uint8)),
                          "raw_masks": torch.from_numpy(mask), "image_params": D.draw_image_params(h, w, True)})
        batch = D.collate(items)
        frames, masks, jobs = (batch[k].to(dev) for k in ("frames", "raw_masks", "image_jobs"))
        images = torch.empty(T_VIDEO, 16, 3, h, w, device=dev)
        out_masks = torch.empty(T_VIDEO, 16, 1, h, w, device=dev)

        def run():
            _lib.call("rac_image_pipeline", _lib.ptr(frames), _lib.ptr(masks), _lib.ptr(jobs), _lib.ptr(images),
                      _lib.ptr(out_masks), 16, T_VIDEO, h, w, _lib.stream_ptr())
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        times = []
        for _ in range(launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        times.sort()
        key = f"{Hs}x{Ws}->{h}x{w}"
        out[key] = {"us_median": round(times[len(times) // 2], 1), "us_min": round(times[0], 1),
                    "us_max": round(times[-1], 1), "bytes_in": frames.numel() + masks.numel(),
                    "bytes_out": 4 * (images.numel() + out_masks.numel())}
        print(f"gpu  rac_image_pipeline {key}: median {out[key]['us_median']} us (min {out[key]['us_min']}, max "
              f"{out[key]['us_max']}) for {16 * T_VIDEO} frames", flush=True)
    return out


def train_half(root, dev, threads, rounds, batches, warmup, resident=False):
    """Loader-fed `_train_video` frames/s: per (data_threads, device_images) a fresh loader + prefetcher per window,
    `warmup` batches untimed, `batches` timed, a synchronise at both ends.  `resident`: every round also has a window
    fed by the device-resident split, one of that feed alone and one of training on a batch that stays on the device."""
    import bench
    cf = bench.namespace(dev, **vars(data_config(root)))
    from robot_aware_control_amd import synthetic as syn
    from robot_aware_control_amd.trainer import PredictionTrainer
    tr = PredictionTrainer(cf)
    tr.model.load_state_dict(syn.synth_state_dict(tr.model, seed=11))
    tr.model.train()
    windows = {}

    def window(key, feed, label, train=True):
        step = tr._train_video if train else (lambda batch: None)
        for _ in range(warmup):
            step(next(feed))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            step(next(feed))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = batches * tr.steps_per_train_video
        rec = {"loaded_frames_per_s": round(batches * cf.batch_size * T_VIDEO / dt, 1), "ms_per_batch": round(1e3 * dt / batches, 2)}
        if train:
            rec["train_frames_per_s"] = round(steps * cf.batch_size * (cf.n_past + cf.n_future) / dt, 1)
        else:
            rec["batches_per_s"] = round(batches / dt, 1)
        windows.setdefault(key, []).append(rec)
        print(f"train {label}: {rec}", flush=True)

    def prefetched(key, loader, label, train=True):
        pf = D.DevicePrefetcher(loader, dev)
        window(key, pf, label, train)
        pf.close()
        pf.thread.join(60)

    resident_loader = still = None
    if resident:
        cf.data_threads, cf.device_images, cf.device_resident = 0, True, True
        t0 = time.perf_counter()
        resident_loader, _ = D.create_loaders(cf)
        store = resident_loader.dataset.store
        windows["resident_store"] = {"videos": len(store), "mb": round(store.nbytes() / 2 ** 20, 1),
                                     "build_s": round(time.perf_counter() - t0, 2)}
        print(f"resident store: {windows['resident_store']}", flush=True)
        cf.device_resident = False
        still = D.process_batch(next(iter(resident_loader)), dev)
    for r in range(rounds):
        for nt in threads:
            for on in (False, True):
                cf.data_threads, cf.device_images = nt, on
                train_loader, _ = D.create_loaders(cf)
                prefetched(f"threads{nt}_{'device' if on else 'host'}", train_loader,
                           f"round {r} data_threads {nt} device_images {on}")
                del train_loader
        if resident:
            prefetched("resident", resident_loader, f"round {r} device_resident")
            prefetched("resident_feed_alone", resident_loader, f"round {r} device_resident, feed alone", train=False)

            def same_batch():
                while True:
                    yield dict(still)
            window("device_batch_no_feed", same_batch(), f"round {r} one batch on the device, no feed")
    return windows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None, help="a make_synthetic_robonet tree (default: written to a temporary directory)")
    ap.add_argument("--per-view", type=int, default=20, help="trajectories per view of the written tree (4 views)")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--items", type=int, default=32, help="videos per CPU measurement")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--threads", default="2,5")
    ap.add_argument("--no-train", action="store_true", help="GPU half: the kernel timing only")
    ap.add_argument("--resident", action="store_true", help="also time the --device_resident feed; writes --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_bench.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        root = a.root
        if root is None:
            root = tmp
            mk.write(root, per_view=a.per_view, length=T_VIDEO, seed=0)
        h, w, Hs, Ws = 48, 64, 64, 85
        result = {"bytes_per_frame": {"host_fp32": 16 * h * w, "device_u8_64x85": 4 * Hs * Ws, "device_u8_240x320": 4 * 240 * 320},
                  "cpu": cpu_half(root, a.items)}
        if not a.cpu_only:
            assert torch.cuda.is_available(), "the GPU half needs the MI355X (or pass --cpu-only)"
            dev = torch.device("cuda:0")
            result["kernel"] = kernel_half(dev)
            if not a.no_train:
                result["train"] = train_half(root, dev, [int(t) for t in a.threads.split(",")], a.rounds, a.batches,
                                             a.warmup, a.resident)
        if a.resident and "train" in result:
            result["shape"] = {"batch": 16, "video_length": T_VIDEO, "stored": [Hs, Ws], "model": [h, w],
                               "rounds": a.rounds, "batches": a.batches, "warmup": a.warmup}
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
        print(json.dumps(result))


if __name__ == "__main__":
    main()
