"""AdversarialCenterPoint — drop-in for models/detectors/adversarial_centerpoint.py:9-278 (§8(f3),
BASELINE config 4).

Same registry name, constructor (adversary_cfg, adversarial_loss_weight, regularization_weight,
**CenterPoint kwargs with the pts_ prefix), attributes (`adversary`, `_epoch`, `_current_l2_norm`)
and methods (`extract_pts_feat`, `loss`, `loss_by_feat_single`, `predict`, `set_epoch`).

extract_pts_feat (:43-115): from `_epoch >= 3` in training the raw voxels are perturbed before the
VFE; with HardSimpleVFE the valid-slot compaction (`sum != 0`, :77), the perturber, the scatter back
and the VFE are the fused VoxelPerturber.perturb_voxels sequence (no host synchronisation).
loss_by_feat_single (:203-257): detection losses clamped to [0, 100] and NaN/Inf-skipped, summed;
loss_adversarial = -min(w * epoch / 10, w) * total when total > 0 (the `.item() > 0` branch of :232
as a device-side select), loss_l2_regularization = regularization_weight * l2, and the logged
perturbation_l2_norm.

Documented fix (SURVEY.md finding 5): the reference stores the perturber's second output — its loss
DICT — as `_current_l2_norm` (:81) and then multiplies / isnan()s it (:247, :252), which raises once
`_epoch >= 3`; here `_current_l2_norm` is that dict's 'l2_norm' scalar, the value the code means.

`attack_eval()` is the attacked evaluation: inside the block the gate also opens in eval mode and the perturber
runs its eval forward (the recipe of evaluate_kitti_adversarial_attack.py, as AdversarialVoxelNet.attack_eval).
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict, List

import torch
from torch import Tensor

from robustpointclouds_amd.adversarial_loss import FusedLosses, center_combination, fused_center_tail
from robustpointclouds_amd.centerpoint import CenterPoint
from robustpointclouds_amd.registry import MODELS as _LOCAL_MODELS
from robustpointclouds_amd.voxelnet import HardSimpleVFE

from .. import builder

try:  # register into mmdet3d too when it is installed
    from mmdet3d.registry import MODELS as _MM_MODELS
except Exception:  # pragma: no cover - mmdet3d absent in this image
    _MM_MODELS = None


def _register(cls):
    _LOCAL_MODELS.register_module(module=cls)
    if _MM_MODELS is not None:
        _MM_MODELS.register_module(module=cls, force=True)
    return cls


@_register
class AdversarialCenterPoint(CenterPoint):
    def __init__(self, adversary_cfg: dict = None, adversarial_loss_weight: float = 1.0,
                 regularization_weight: float = 0.05, **kwargs):
        super().__init__(**kwargs)
        self.adversary = builder.build_adversary(adversary_cfg) if adversary_cfg is not None else None
        if self.adversary is not None:
            self.adversary._return_loss_dict = True
        self.adversarial_loss_weight = adversarial_loss_weight
        self.regularization_weight = regularization_weight
        self._current_l2_norm = None
        self._epoch = 0
        self._attack_eval = False

    def _gate(self):
        if getattr(self, "_attack_eval", False):
            return self.adversary is not None and self._epoch >= 3   # attacked evaluation: whatever `training` is
        return self.training and self._epoch >= 3                                      # :65

    @contextmanager
    def attack_eval(self):
        """Attacked evaluation, the contract of AdversarialVoxelNet.attack_eval(): inside the block the perturber
        runs although the detector is in eval mode (adversary present and `_epoch >= 3`). The reference has no
        attacked nuScenes evaluation of its own — its evaluate_nuscenes_adversarial.py runs the stock test loop
        in eval mode, where the gate `self.training and self._epoch >= 3` (:65) never opens — so this is the
        KITTI recipe (evaluate_kitti_adversarial_attack.py:23-62) applied to CenterPoint. Every submodule stays
        in eval mode, so the perturber takes its eval forward (running-statistics BatchNorm, eval bounds), which
        `self.adversary.training == False` already selects. No module's `training` changes; the previous
        `_attack_eval` is restored when the block exits, also when it raises."""
        prev = getattr(self, "_attack_eval", False)
        self._attack_eval = True
        try:
            yield self
        finally:
            self._attack_eval = prev

    def extract_pts_feat(self, voxel_dict, points=None, img_feats=None, batch_input_metas=None):
        if self.adversary is None:
            return super().extract_pts_feat(voxel_dict, points, img_feats, batch_input_metas)
        voxels, npts, coors = voxel_dict["voxels"], voxel_dict["num_points"], voxel_dict["coors"]
        self._sync_engines(voxels.device)
        if hasattr(self.pts_middle_encoder, "coors_ready"):
            self.pts_middle_encoder.coors_ready(coors)
        l2 = None
        if self._gate():
            if isinstance(self.pts_voxel_encoder, HardSimpleVFE):
                feats, loss_dict, _, _ = self.adversary.perturb_voxels(voxels, npts, self.pts_voxel_encoder.num_features)
            else:
                V, P, F = voxels.shape
                flat = voxels.view(-1, F)
                valid = flat.sum(dim=1) != 0                                           # :77
                out, loss_dict = self.adversary(flat[valid])
                flat2 = flat.clone()
                flat2[valid] = out
                feats = self.pts_voxel_encoder(flat2.view(V, P, F), npts, coors)
            l2 = loss_dict["l2_norm"]                                                  # finding 5 fix
        else:
            feats = self.pts_voxel_encoder(voxels, npts, coors)
        x = self.pts_middle_encoder(feats, coors, self._batch_size(voxel_dict))         # :114
        x = self.pts_backbone(x)
        if self.with_pts_neck:
            x = self.pts_neck(x)
        self._current_l2_norm = l2
        return x

    def loss(self, batch_inputs_dict: Dict[str, Tensor], batch_data_samples, **kwargs):
        losses = {}
        if batch_inputs_dict.get("points", None) is not None or "voxels" in batch_inputs_dict:
            vd = dict(batch_inputs_dict["voxels"])
            vd.setdefault("batch_size", batch_inputs_dict.get("batch_size"))
            res = self.loss_by_feat_single(vd, batch_data_samples, **kwargs)
            if isinstance(res, FusedLosses):   # keeps the fused tail's parse_losses total
                return res
            losses.update(res)
        return losses

    def loss_by_feat_single(self, voxel_dict, batch_data_samples, **kwargs):
        outs = self.pts_bbox_head(self.extract_pts_feat(voxel_dict))
        if isinstance(batch_data_samples, dict):
            gts = batch_data_samples
        else:
            gts = [s.gt_instances_3d for s in batch_data_samples]
        losses = self.pts_bbox_head.loss_by_feat(outs, gts)
        device = voxel_dict["voxels"].device
        zero = lambda: torch.zeros((), device=device, requires_grad=True)
        if self.training and self._current_l2_norm is not None:
            w = min(self.adversarial_loss_weight * (self._epoch / 10.0), self.adversarial_loss_weight)
            # the HIP tail (csrc/step_tail.hip) over the CenterHead's packed losses: the same values bit for
            # bit as the torch composition, in one launch each way instead of ~100 scalar kernels
            fused = fused_center_tail(losses, getattr(losses, "packed", None), self._current_l2_norm, w,
                                      self.regularization_weight)
            if fused is not None:
                return fused
            losses = center_combination(losses, self._current_l2_norm, w, self.regularization_weight, device)
        else:
            losses["loss_adversarial"] = zero()
            losses["loss_l2_regularization"] = zero()
        return losses

    @torch.no_grad()
    def predict(self, batch_inputs_dict, batch_data_samples=None, **kwargs) -> List[dict]:
        """Detections per frame — dict(bboxes_3d [n, 9], scores_3d, labels_3d) — from
        `pts_bbox_head.predict_by_feat` (CenterPoint box decoding + circle NMS on the HIP kernels of
        csrc/postprocess.hip) plus the perturbation norm like :262-273."""
        vd = dict(batch_inputs_dict["voxels"])
        vd.setdefault("batch_size", batch_inputs_dict.get("batch_size"))
        preds = self.pts_bbox_head(self.extract_pts_feat(vd))
        res = self.pts_bbox_head.predict_by_feat(preds)
        if self._current_l2_norm is not None:
            l2 = float(self._current_l2_norm)
            for r in res:
                r["perturbation_l2_norm"] = l2
        return res

    def set_epoch(self, epoch):
        self._epoch = epoch
