"""What NuScenesDetectionScore.compute() takes for a synthetic set of nuScenes-val size (6019 frames, about 200
detections and 35 ground truths a frame, ten classes) on the GPU, split into the device part (`_matches`: torch
sorting and flags, the two kernels of csrc/nuscenes_eval.hip, the one host read) and the host curves, with the two
kernels timed by device events; and the CPU path at 1/100 of that size for scale. Needs a GPU (no fallback).

    python tools/nuscenes_eval_time.py [--frames 6019] [--repeat 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robustpointclouds_amd import nuscenes_eval as ne  # noqa: E402


def synthetic(frames, seed, device):
    """-> (preds, gts): per frame ~35 ground truths inside 55 m, ~200 detections of which 60 % lie within 1.5 m of a
    ground truth of their class."""
    rng = np.random.default_rng(seed)
    preds, gts = [], []
    for _ in range(frames):
        ng, nd = int(rng.integers(20, 51)), int(rng.integers(150, 251))
        gt = np.zeros((ng, 9), np.float32)
        gt[:, :2] = rng.uniform(-55, 55, (ng, 2))
        gt[:, 3:6] = rng.uniform(0.5, 5.0, (ng, 3))
        gt[:, 6] = rng.uniform(-np.pi, np.pi, ng)
        gt[:, 7:9] = rng.normal(0, 2, (ng, 2))
        gl = rng.integers(0, 10, ng)
        src = rng.integers(0, ng, nd)
        near = rng.random(nd) < 0.6
        det = gt[src] + rng.normal(0, 0.5, (nd, 9)).astype(np.float32)
        det[~near, :2] = rng.uniform(-55, 55, (int((~near).sum()), 2))
        det[:, 3:6] = np.abs(det[:, 3:6]) + 0.1
        dl = np.where(near, gl[src], rng.integers(0, 10, nd))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        preds.append(dict(bboxes_3d=t(det).to(device), scores_3d=t(rng.random(nd).astype(np.float32)).to(device),
                          labels_3d=t(dl.astype(np.int64)).to(device)))
        gts.append(dict(bboxes_3d=t(gt), labels_3d=t(gl.astype(np.int64)), attr_labels=t(rng.integers(-1, 8, ng)),
                        num_pts=t(rng.integers(0, 40, ng))))
    return preds, gts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6019)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nuscenes_eval_time needs a GPU")
    dev = torch.device("cuda")
    metric = ne.NuScenesDetectionScore()
    preds, gts = synthetic(a.frames, 0, dev)
    for k in range(0, a.frames, 64):
        metric.update(preds[k:k + 64], gts[k:k + 64])
    kernel_ms = {}

    def timed(name, fn):
        def run(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args, **kw)
            e1.record()
            e1.synchronize()
            kernel_ms.setdefault(name, []).append(e0.elapsed_time(e1))
            return out
        return run

    rows = []
    for it in range(a.repeat + 1):   # the first pass warms up (code objects, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metric._matches()
        t1 = time.perf_counter()
        out = metric.compute()
        t2 = time.perf_counter()
        if it:
            rows.append(dict(device_part_s=t1 - t0, compute_s=t2 - t1, host_curves_s=(t2 - t1) - (t1 - t0)))
    # the kernels by device events, in passes of their own (the event waits would sit inside the timings above)
    orig = ne.center_matches, ne._tp_errors
    ne.center_matches, ne._tp_errors = timed("rpc_nus_match", orig[0]), timed("rpc_nus_tp_errors", orig[1])
    for _ in range(a.repeat):
        metric._matches()
    ne.center_matches, ne._tp_errors = orig
    med = lambda k: statistics.median(r[k] for r in rows)
    spread = lambda k: (min(r[k] for r in rows), max(r[k] for r in rows))
    small = ne.NuScenesDetectionScore()
    n_small = max(1, a.frames // 100)
    small.update([{k: v.cpu() for k, v in p.items()} for p in preds[:n_small]], gts[:n_small])
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        small.compute()
        cpu.append(time.perf_counter() - t0)
    res = dict(frames=a.frames, detections=sum(metric._nd), ground_truths=sum(metric._ng), repeat=a.repeat,
               compute_s=med("compute_s"), compute_s_min_max=spread("compute_s"),
               device_part_s=med("device_part_s"), device_part_s_min_max=spread("device_part_s"),
               host_curves_s=med("host_curves_s"), host_curves_s_min_max=spread("host_curves_s"),
               kernel_ms={k: statistics.median(v) for k, v in kernel_ms.items()},
               cpu_path_frames=n_small, cpu_path_compute_s=statistics.median(cpu),
               mAP=out["NuScenes/mAP"], NDS=out["NuScenes/NDS"], device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
