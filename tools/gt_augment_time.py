"""What GpuObjectSample + GpuObjectNoise take at the headline workload's size (batch 6 synthetic KITTI frames,
3 classes, sample_groups 15/10/10, num_try 100), the two transforms that have to hide under the training step
on the prefetch stream. The database is cropped from other synthetic frames with GtDatabase.from_frames and
filtered with prepare. Reported: the host draws (`sample`), and the device work by device events and by a host
clock around a synchronised call, candidates and noise tables drawn beforehand. Needs a GPU (no fallback).

    python tools/gt_augment_time.py [--batch 6] [--repeat 30] [--out FILE.json]
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
from robustpointclouds_amd import GpuObjectNoise, GpuObjectSample, GtDatabase  # noqa: E402
from robustpointclouds_amd.pipeline import concat_frames  # noqa: E402
from robustpointclouds_amd.synthetic import kitti_batch  # noqa: E402

CLASSES = ("Car", "Pedestrian", "Cyclist")
GROUPS = dict(Car=15, Pedestrian=10, Cyclist=10)


def packed(boxes, labels, M, dev):
    gb = torch.zeros(len(boxes), M, 7)
    gb[..., 3:6] = 1.0
    gl = torch.full((len(boxes), M), -1, dtype=torch.long)
    for i, (b, l) in enumerate(zip(boxes, labels)):
        gb[i, :len(b)] = torch.from_numpy(np.asarray(b, np.float32))
        gl[i, :len(l)] = torch.from_numpy(np.asarray(l, np.int64))
    return gb.to(dev), gl.to(dev), gl.numpy().copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--db-frames", type=int, default=48)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gt_augment_time needs a GPU")
    dev = torch.device("cuda")
    pts, boxes, labels = kitti_batch(a.db_frames, seed0=1000, num_classes=3)
    x, off = concat_frames(pts, dev)
    gb, gl, _ = packed(boxes, labels, 16, dev)
    db = GtDatabase.from_frames(x, off, gb, gl, CLASSES).prepare(
        filter_by_difficulty=[-1], filter_by_min_points=dict(Car=5, Pedestrian=5, Cyclist=5))
    sampler = GpuObjectSample(db, GROUPS, CLASSES)
    noise = GpuObjectNoise(num_try=100)
    pts, boxes, labels = kitti_batch(a.batch, seed0=0, num_classes=3)
    x, off = concat_frames(pts, dev)
    gb0, gl0, gl_host = packed(boxes, labels, a.slots, dev)
    rng = np.random.RandomState(0)
    rows = []
    for it in range(a.repeat + 3):   # the first passes warm up (code objects, allocator)
        t0 = time.perf_counter()
        samples = sampler.sample(gl_host, rng)
        tables = noise.sample(a.batch, a.slots, rng)
        t1 = time.perf_counter()
        gb, gl = gb0.clone(), gl0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        e0.record()
        p1, o1, gb, gl, accept = sampler(x, off, gb, gl, samples=samples)
        p2, gb, chosen = noise(p1, o1, gb, gl, noise=tables)
        e1.record()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if it >= 3:
            rows.append(dict(host_draws_ms=1e3 * (t1 - t0), device_events_ms=e0.elapsed_time(e1),
                             call_synchronised_ms=1e3 * (t3 - t2)))
    med = lambda k: statistics.median(r[k] for r in rows)
    spread = lambda k: (min(r[k] for r in rows), max(r[k] for r in rows))
    res = dict(batch=a.batch, points=int(x.shape[0]), slots=a.slots, database_objects=len(db),
               database_points=int(db.points.shape[0]), candidates=int((samples[0] >= 0).sum()),
               accepted=int((accept >= 0).sum()), noise_moved_boxes=int((chosen >= 0).sum()), num_try=100,
               out_points=int(o1[-1]), repeat=a.repeat)
    for k in ("host_draws_ms", "device_events_ms", "call_synchronised_ms"):
        res[k] = med(k)
        res[k + "_min_max"] = spread(k)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
