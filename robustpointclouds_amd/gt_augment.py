"""GT-database augmentation on the GPU: points in rotated boxes, ObjectSample, ObjectNoise.

configs/_base_/kitti-3d-car.py:42-68 opens its training pipeline with ObjectSample (paste objects of a
ground-truth database into the frame) and ObjectNoise (jitter every object with its points); the other five
transforms are `pipeline.GpuTrainAugment`. Both are geometry on boxes and points, and the database itself is
"the points inside each ground-truth box of the training frames": a points-in-boxes crop (csrc/gt_augment.hip;
the rules are written out in DESIGN.md "GT-database augmentation").

* `points_in_boxes` — per point the first containing box of its frame, a bitmask of all of them, and the
  points per box (mmcv `points_in_boxes_part` / `_all` in one pass).
* `GtDatabase` — the objects on the device: one concatenated point tensor centred on each box's (x, y, z),
  offsets, a box table; boxes, labels, difficulty and points per object also on the host for the sampler.
* `GpuObjectSample` — `sample` draws candidates on the host with upstream's BatchSampler cursor semantics;
  the collision tests, the choice, the slot filling and the point compaction run on the device.
* `GpuObjectNoise` — `sample` draws upstream's noise tables on the host; picking each box's first free try
  and moving points and boxes run on the device.

As in `GpuTrainAugment`, all random numbers come from a numpy RNG on the host in upstream's order, no
`__call__` reads a count back from the device (dropped rows are NaN, which the voxeliser rejects), and there
is no CPU path. Upstream mmdet3d / mmcv are not vendored: parity w.r.t. upstream itself is unpinned.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _ffi


def _need_cuda(t: torch.Tensor, who: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{who} runs on the HIP kernels only (no CPU path)")


def _upload(a: np.ndarray, device) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a))
    if torch.device(device).type != "cuda" or t.numel() == 0:
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def points_in_boxes(points: torch.Tensor, offsets: torch.Tensor, boxes: torch.Tensor, labels: torch.Tensor,
                    with_mask: bool = True):
    """points [P, F] (frames concatenated, cuda), offsets [B+1] int32, boxes [B, M, 7], labels [B, M] int64
    (-1 = padding) -> (first [P] int32, mask [P, ceil(M/32)] int32 bit pattern or None, counts [B, M] int32)."""
    lib = _ffi.load()
    _need_cuda(points, "points_in_boxes")
    if boxes.dim() != 3 or boxes.shape[-1] != 7 or boxes.dtype != torch.float32 or labels.dtype != torch.int64:
        raise TypeError("boxes float32 [B, M, 7] and labels int64 [B, M] expected")
    points = points.float().contiguous()
    dev = points.device
    offsets = offsets.to(device=dev, dtype=torch.int32).contiguous()
    boxes, labels = boxes.to(dev).contiguous(), labels.to(dev).contiguous()
    B, M = labels.shape
    if offsets.numel() != B + 1:
        raise ValueError("offsets must have one entry more than boxes has frames")
    P, F = points.shape
    first = torch.empty(P, dtype=torch.int32, device=dev)
    mask = torch.empty((P, (M + 31) // 32), dtype=torch.int32, device=dev) if with_mask else None
    counts = torch.empty((B, M), dtype=torch.int32, device=dev)
    _ffi.check(lib.rpc_points_in_boxes(_ffi.ptr(points), F, P, _ffi.ptr(offsets), B, _ffi.ptr(boxes),
                                       _ffi.ptr(labels), M, _ffi.ptr(first), _ffi.ptr(mask), _ffi.ptr(counts),
                                       _ffi.stream_of(points)), "rpc_points_in_boxes")
    return first, mask, counts


class GtDatabase:
    """Ground-truth objects on the device (points centred on the box's (x, y, z), as upstream's
    create_gt_database stores them) with the host copy the sampler needs. A database may be held on the CPU
    (to filter it, or to draw candidates); the transforms that use it need it on the GPU."""

    def __init__(self, points: torch.Tensor, offsets_host: np.ndarray, boxes_host: np.ndarray,
                 labels_host: np.ndarray, difficulty_host: np.ndarray, class_names: Sequence[str]):
        dev = points.device
        self.class_names = list(class_names)
        self.points = points.float().contiguous()
        self.offsets_host = np.asarray(offsets_host, np.int32)
        self.boxes_host = np.asarray(boxes_host, np.float32).reshape(-1, 7)
        self.labels_host = np.asarray(labels_host, np.int64)
        self.difficulty_host = np.asarray(difficulty_host, np.int64)
        self.num_points_host = np.diff(self.offsets_host).astype(np.int64)
        self.offsets = _upload(self.offsets_host, dev)
        self.boxes = _upload(self.boxes_host, dev)
        self.labels = _upload(self.labels_host, dev)

    def __len__(self) -> int:
        return int(self.labels_host.shape[0])

    @property
    def device(self):
        return self.points.device

    def object_points(self, i: int) -> torch.Tensor:
        return self.points[int(self.offsets_host[i]):int(self.offsets_host[i + 1])]

    @classmethod
    def from_objects(cls, objects, class_names: Sequence[str], device="cuda") -> "GtDatabase":
        """objects: (points [n, F] centred on the box, box [7], label, difficulty) per object."""
        objects = list(objects)
        F = objects[0][0].shape[1] if objects else 4
        pts = [np.asarray(o[0], np.float32).reshape(-1, F) for o in objects]
        off = np.zeros(len(objects) + 1, np.int32)
        off[1:] = np.cumsum([p.shape[0] for p in pts])
        allp = np.concatenate(pts, 0) if pts else np.zeros((0, F), np.float32)
        boxes = np.array([np.asarray(o[1], np.float32) for o in objects], np.float32).reshape(-1, 7)
        labels = np.array([int(o[2]) for o in objects], np.int64)
        diff = np.array([int(o[3]) for o in objects], np.int64)
        return cls(_upload(allp, torch.device(device)), off, boxes, labels, diff, class_names)

    @classmethod
    def from_frames(cls, points: torch.Tensor, offsets: torch.Tensor, boxes: torch.Tensor, labels: torch.Tensor,
                    class_names: Sequence[str], difficulty: Optional[torch.Tensor] = None) -> "GtDatabase":
        """Crop every existing box of every frame (a point inside two boxes belongs to both objects).
        Offline: this reads the bitmask and the counts on the host."""
        _, mask, counts = points_in_boxes(points, offsets, boxes, labels)
        points = points.float()
        B, M = labels.shape
        off = offsets.cpu().numpy().astype(np.int64)
        lab = labels.cpu().numpy()
        box = boxes.detach().cpu().numpy().astype(np.float32)
        dif = np.zeros((B, M), np.int64) if difficulty is None else difficulty.cpu().numpy().astype(np.int64)
        exists = (lab >= 0) & (box[..., 3:6] > 0).all(-1)
        chunks, n_obj, keep = [], [], []
        for b in range(B):
            fm = mask[off[b]:off[b + 1]]
            fp = points[off[b]:off[b + 1]]
            for m in np.nonzero(exists[b])[0]:
                inside = ((fm[:, m // 32] >> (m % 32)) & 1).bool()
                o = fp[inside].clone()
                o[:, :3] -= boxes[b, m, :3].to(o.device)
                chunks.append(o)
                n_obj.append(o.shape[0])
                keep.append((b, m))
                assert o.shape[0] == int(counts[b, m])
        o_off = np.zeros(len(keep) + 1, np.int32)
        o_off[1:] = np.cumsum(n_obj)
        allp = torch.cat(chunks, 0) if chunks else points.new_zeros((0, points.shape[1]))
        idx = tuple(np.array(keep, np.int64).reshape(-1, 2).T)
        return cls(allp, o_off, box[idx], lab[idx], dif[idx], class_names)

    def prepare(self, filter_by_difficulty: Sequence[int] = (-1,),
                filter_by_min_points: Optional[Dict[str, int]] = None) -> "GtDatabase":
        """Upstream's `prepare`: drop objects whose difficulty is listed and objects with fewer points than
        their class's minimum. Returns a new database (offline: gathers on the device)."""
        keep = ~np.isin(self.difficulty_host, np.asarray(list(filter_by_difficulty), np.int64))
        for name, least in (filter_by_min_points or {}).items():
            c = self.class_names.index(name)
            keep &= ~((self.labels_host == c) & (self.num_points_host < int(least)))
        sel = np.nonzero(keep)[0]
        rows = [np.arange(self.offsets_host[i], self.offsets_host[i + 1]) for i in sel]
        rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        off = np.zeros(len(sel) + 1, np.int32)
        off[1:] = np.cumsum(self.num_points_host[sel])
        pts = self.points[torch.from_numpy(rows.astype(np.int64)).to(self.device)]
        return GtDatabase(pts, off, self.boxes_host[sel], self.labels_host[sel], self.difficulty_host[sel],
                          self.class_names)


class GpuObjectSample:
    """ObjectSample(db_sampler=DataBaseSampler(rate, sample_groups, classes)) for a batch of frames."""

    def __init__(self, db: GtDatabase, sample_groups: Dict[str, int], classes: Sequence[str], rate: float = 1.0):
        self.db = db
        self.rate = float(rate)
        self.classes = list(classes)
        self.sample_groups = {k: int(v) for k, v in sample_groups.items()}
        # per class: the database indices, a permutation of them and the cursor (upstream BatchSampler)
        self._label = {c: db.class_names.index(c) for c in self.classes}
        self._members = {c: np.nonzero(db.labels_host == self._label[c])[0] for c in self.classes}
        self._perm: Dict[str, Optional[np.ndarray]] = {c: None for c in self.classes}
        self._cursor = {c: 0 for c in self.classes}

    def _draw(self, c: str, num: int, rng) -> np.ndarray:
        """BatchSampler._sample: a short tail when the cursor would reach the end, then a reshuffle."""
        mem = self._members[c]
        if self._perm[c] is None:
            self._perm[c] = rng.permutation(len(mem))
        idx, n = self._cursor[c], len(mem)
        if idx + num >= n:
            ret = self._perm[c][idx:].copy()
            self._perm[c] = rng.permutation(n)
            self._cursor[c] = 0
        else:
            ret = self._perm[c][idx:idx + num]
            self._cursor[c] = idx + num
        return mem[ret]

    def need(self, c: str, labels: np.ndarray) -> int:
        have = int(np.sum(np.asarray(labels) == self._label[c]))
        return int(np.round(self.rate * (self.sample_groups[c] - have)))

    def sample(self, labels_host, rng=np.random) -> Tuple[np.ndarray, np.ndarray]:
        """labels_host [B][M] (-1 = padding) -> (cand [B, S] int32 database indices, -1 padded; draw [B, S]
        int32, the class-draw each candidate came from, -1 padded). S is the widest frame."""
        rows: List[List[int]] = []
        draws: List[List[int]] = []
        for labels in labels_host:
            row, drw = [], []
            for d, c in enumerate(self.classes):
                num = self.need(c, labels)
                if num <= 0 or len(self._members[c]) == 0:
                    continue
                got = self._draw(c, num, rng)
                row += [int(g) for g in got]
                drw += [d] * len(got)
            rows.append(row)
            draws.append(drw)
        S = max([len(r) for r in rows], default=0)
        if S > _ffi.GT_MAX_CAND:
            raise ValueError(f"{S} candidates in one frame: more than {_ffi.GT_MAX_CAND}")
        cand = np.full((len(rows), S), -1, np.int32)
        draw = np.full((len(rows), S), -1, np.int32)
        for b, (r, d) in enumerate(zip(rows, draws)):
            cand[b, :len(r)] = r
            draw[b, :len(r)] = d
        return cand, draw

    def __call__(self, points: torch.Tensor, offsets: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
                 samples: Optional[Tuple[np.ndarray, np.ndarray]] = None, labels_host=None, rng=np.random):
        """points [P, F] / offsets [B+1] (cuda), gt_boxes [B, M, 7] float32 / gt_labels [B, M] int64 (updated
        in place) -> (points', offsets', gt_boxes, gt_labels, accept [B, S] int32: slot or -1).
        The candidates come from `samples` (= `sample(...)`) or are drawn here from `labels_host`, the host
        copy of the labels every loader has: the device labels are never read back."""
        lib = _ffi.load()
        _need_cuda(points, "GpuObjectSample")
        _need_cuda(self.db.points, "GpuObjectSample (database)")
        if gt_labels.dtype != torch.int64 or gt_boxes.dtype != torch.float32:
            raise TypeError("gt_boxes float32 [B, M, 7] and gt_labels int64 [B, M] expected")
        if not (gt_boxes.is_cuda and gt_boxes.is_contiguous() and gt_labels.is_cuda and gt_labels.is_contiguous()):
            raise RuntimeError("gt_boxes / gt_labels are updated in place: contiguous cuda tensors expected")
        if samples is None:
            if labels_host is None:
                raise ValueError("pass samples=sample(labels_host, rng) or labels_host (no device read here)")
            samples = self.sample(labels_host, rng)
        cand_h, draw_h = (np.ascontiguousarray(a, np.int32) for a in samples)
        db = self.db
        points = points.float().contiguous()
        dev = points.device
        offsets = offsets.to(device=dev, dtype=torch.int32).contiguous()
        B, M = gt_labels.shape
        P, F = points.shape
        S = cand_h.shape[1]
        if cand_h.shape[0] != B or offsets.numel() != B + 1:
            raise ValueError("samples, offsets and gt_labels disagree on the batch size")
        if db.points.shape[1] != F and len(db):
            raise ValueError("database points and scene points differ in width")
        extra = int(db.num_points_host[cand_h[cand_h >= 0]].sum())
        cap = P + extra
        cand, draw = _upload(cand_h, dev), _upload(draw_h, dev)
        accept = torch.empty((B, S), dtype=torch.int32, device=dev)
        out = torch.empty((cap, F), dtype=torch.float32, device=dev)
        out_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
        st = _ffi.stream_of(points)
        N = len(db)
        _ffi.check(lib.rpc_object_sample_select(_ffi.ptr(db.boxes), _ffi.ptr(db.labels), N, _ffi.ptr(cand),
                                                _ffi.ptr(draw), B, S, _ffi.ptr(gt_boxes), _ffi.ptr(gt_labels), M,
                                                _ffi.ptr(accept), st), "rpc_object_sample_select")
        wsz = lib.rpc_object_sample_points_workspace_size(P, B, S)
        ws = _ffi.workspace(wsz, dev)
        _ffi.check(lib.rpc_object_sample_points(_ffi.ptr(points), F, P, _ffi.ptr(offsets), B, _ffi.ptr(db.points),
                                                _ffi.ptr(db.offsets), _ffi.ptr(db.boxes), N, _ffi.ptr(cand),
                                                _ffi.ptr(accept), S, _ffi.ptr(out), cap, _ffi.ptr(out_off),
                                                _ffi.ptr(ws), wsz, st), "rpc_object_sample_points")
        return out, out_off, gt_boxes, gt_labels, accept


class GpuObjectNoise:
    """ObjectNoise(num_try, translation_std, global_rot_range=[0, 0], rot_range) for a batch of frames."""

    def __init__(self, num_try: int = 100, translation_std=(1.0, 1.0, 0.5), rot_range=(-0.78539816, 0.78539816),
                 global_rot_range=(0.0, 0.0)):
        if any(float(v) != 0.0 for v in global_rot_range):
            raise NotImplementedError("ObjectNoise with a global_rot_range other than [0, 0]")
        if not 0 <= int(num_try) <= _ffi.GT_MAX_TRY:
            raise ValueError(f"num_try must be in 0..{_ffi.GT_MAX_TRY}")
        self.num_try = int(num_try)
        self.translation_std = [float(v) for v in translation_std]
        self.rot_range = [float(v) for v in rot_range]

    def sample(self, batch: int, max_gts: int, rng=np.random) -> Tuple[np.ndarray, np.ndarray]:
        """loc [B, M, T, 3] ~ N(0, std) then rot [B, M, T] ~ U(rot_range), frame after frame, as upstream's
        noise_per_object_v3_ draws them (float32, what the device reads)."""
        T = self.num_try
        loc = np.zeros((batch, max_gts, T, 3), np.float32)
        rot = np.zeros((batch, max_gts, T), np.float32)
        for b in range(batch):
            loc[b] = rng.normal(scale=self.translation_std, size=[max_gts, T, 3])
            rot[b] = rng.uniform(self.rot_range[0], self.rot_range[1], size=[max_gts, T])
        return loc, rot

    def __call__(self, points: torch.Tensor, offsets: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
                 noise: Optional[Tuple[np.ndarray, np.ndarray]] = None, rng=np.random):
        """points [P, F] / offsets [B+1] (cuda), gt_boxes [B, M, 7] / gt_labels [B, M] -> (points, gt_boxes,
        chosen [B, M] int32). Points (when a contiguous float32 tensor) and boxes are updated in place."""
        lib = _ffi.load()
        _need_cuda(points, "GpuObjectNoise")
        if gt_labels.dtype != torch.int64 or gt_boxes.dtype != torch.float32:
            raise TypeError("gt_boxes float32 [B, M, 7] and gt_labels int64 [B, M] expected")
        if not (gt_boxes.is_cuda and gt_boxes.is_contiguous() and gt_labels.is_cuda and gt_labels.is_contiguous()):
            raise RuntimeError("gt_boxes is updated in place: contiguous cuda tensors expected")
        points = points.float().contiguous()
        dev = points.device
        offsets = offsets.to(device=dev, dtype=torch.int32).contiguous()
        B, M = gt_labels.shape
        P, F = points.shape
        T = self.num_try
        if noise is None:
            noise = self.sample(B, M, rng)
        loc_h, rot_h = (np.ascontiguousarray(a, np.float32) for a in noise)
        if loc_h.shape != (B, M, T, 3) or rot_h.shape != (B, M, T):
            raise ValueError("noise tables must be [B, M, T, 3] and [B, M, T]")
        loc, rot = _upload(loc_h, dev), _upload(rot_h, dev)
        chosen = torch.empty((B, M), dtype=torch.int32, device=dev)
        st = _ffi.stream_of(points)
        _ffi.check(lib.rpc_object_noise_select(_ffi.ptr(gt_boxes), _ffi.ptr(gt_labels), B, M, _ffi.ptr(loc),
                                               _ffi.ptr(rot), T, _ffi.ptr(chosen), st), "rpc_object_noise_select")
        _ffi.check(lib.rpc_object_noise_apply(_ffi.ptr(points), F, P, _ffi.ptr(offsets), B, _ffi.ptr(gt_boxes),
                                              _ffi.ptr(gt_labels), M, _ffi.ptr(loc), _ffi.ptr(rot), T,
                                              _ffi.ptr(chosen), st), "rpc_object_noise_apply")
        return points, gt_boxes, chosen
