"""What KittiAP.compute() takes on a synthetic set of KITTI-val size (3769 frames, 50 detections and 12 ground truths
each, 3 classes, the frames given in one `update` call) on the GPU: the default two metrics without a calibration
(the evaluator as it was before the calibration), and all four metrics with a calibration and DontCare regions, by
HIP events, `--repeat` runs after a warm-up; and the new kernels' share, each timed by events in passes of their own.
Needs a GPU (no fallback).

    python tools/kitti_calib_time.py [--frames 3769] [--repeat 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robustpointclouds_amd import kitti_eval as ke  # noqa: E402

CLASSES = ["Car", "Pedestrian", "Cyclist"]
SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])
P2 = [[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]
TR = [[0.0, -1.0, 0.0, -0.004], [0.0, 0.0, -1.0, -0.076], [1.0, 0.0, 0.0, -0.272]]


def synthetic(frames, seed, device, calibrated):
    """-> (preds, gts): per frame 12 ground truths in front of the camera, 50 detections of which 70 % are jittered
    copies of a ground truth; with `calibrated`, lidar2img / img_shape and three DontCare boxes a frame."""
    rng = np.random.default_rng(seed)
    l2i = ke.lidar2img(P2, np.eye(3), TR)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    preds, gts = [], []
    for _ in range(frames):
        ng, nd = 12, 50
        gl = rng.integers(0, 3, ng)
        x = rng.uniform(5, 68, ng)
        gt = np.stack([x, rng.uniform(-0.6, 0.6, ng) * x, rng.uniform(-2.2, -1.0, ng), *(SIZES[gl] * rng.uniform(0.9, 1.1, (ng, 3))).T,
                       rng.uniform(-np.pi, np.pi, ng)], 1).astype(np.float32)
        src = rng.integers(0, ng, nd)
        near = rng.random(nd) < 0.7
        det = gt[src] + (rng.normal(0, 0.15, (nd, 7)) * [1, 1, 0.3, 0.3, 0.2, 0.2, 0.3]).astype(np.float32)
        far = int((~near).sum())
        det[~near, 0], det[~near, 1] = rng.uniform(2, 75, far), rng.uniform(-42, 42, far)
        det[:, 3:6] = np.maximum(det[:, 3:6], 0.2)
        dl = np.where(near, gl[src], rng.integers(0, 3, nd))
        preds.append(dict(bboxes_3d=t(det).to(device), scores_3d=t(rng.random(nd).astype(np.float32)).to(device),
                          labels_3d=t(dl.astype(np.int64)).to(device)))
        g = dict(bboxes_3d=t(gt), labels_3d=t(gl.astype(np.int64)), occluded=t(rng.integers(0, 3, ng).astype(np.float32)),
                 truncated=t((rng.random(ng) * 0.4).astype(np.float32)))
        if calibrated:
            x1, y1 = rng.uniform(0, 1100, 3), rng.uniform(0, 300, 3)
            g.update(lidar2img=l2i, img_shape=(375, 1242),
                     dontcare=np.stack([x1, y1, x1 + rng.uniform(40, 300, 3), y1 + rng.uniform(30, 120, 3)], 1).astype(np.float32))
        gts.append(g)
    return preds, gts


def event_ms(fn, repeat):
    """Median, min and max of `repeat` runs of fn by device events after one warm-up run."""
    fn()
    ms = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kitti_calib_time needs a GPU")
    dev = torch.device("cuda")
    plain = ke.KittiAP(CLASSES)
    plain.update(*synthetic(a.frames, 0, dev, calibrated=False))
    four = ke.KittiAP(CLASSES, metrics=ke.ALL_METRICS)
    four.update(*synthetic(a.frames, 0, dev, calibrated=True))
    two_cal = ke.KittiAP(CLASSES)
    two_cal.update(*synthetic(a.frames, 0, dev, calibrated=True))
    res = dict(frames=a.frames, detections=sum(four._nd), ground_truths=sum(four._ng), repeat=a.repeat,
               device=torch.cuda.get_device_name(0),
               compute_two_metrics_ms=event_ms(plain.compute, a.repeat),
               compute_two_metrics_calibrated_ms=event_ms(two_cal.compute, a.repeat),
               compute_four_metrics_ms=event_ms(four.compute, a.repeat))
    # the new kernels by device events, in passes of their own (the event waits would sit inside the timings above)
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

    orig = ke.project_boxes, ke._overlaps_2d, ke._stuff_bits, ke._match_counts
    ke.project_boxes = timed("rpc_kitti_project (one side)", orig[0])
    ke._overlaps_2d = timed("rpc_kitti_overlaps_2d mode 0", orig[1])
    ke._stuff_bits = timed("rpc_kitti_overlaps_2d mode 1", orig[2])
    ke._match_counts = lambda *args, **kw: (timed("rpc_kitti_match_counts_aos" if kw.get("ext") else
                                                  "rpc_kitti_match_counts (one family)", orig[3]))(*args, **kw)
    for _ in range(a.repeat + 1):
        four.compute()
    ke.project_boxes, ke._overlaps_2d, ke._stuff_bits, ke._match_counts = orig
    res["kernel_ms"] = {k: statistics.median(v[len(v) // (a.repeat + 1):]) for k, v in kernel_ms.items()}
    out = four.compute()
    res["values"] = {k: out[k] for k in ("KITTI/Car_BEV_AP40_moderate_strict", "KITTI/Car_2D_AP40_moderate_strict",
                                         "KITTI/Car_AOS_AP40_moderate_strict", "KITTI/Car_BEV_AP40_easy_strict")}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
