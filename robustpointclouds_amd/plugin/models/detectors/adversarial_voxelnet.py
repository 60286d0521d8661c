"""AdversarialVoxelNet — drop-in for models/detectors/adversarial_voxelnet.py:9-481.

Same registry name, constructor (adversary_cfg, adversarial_loss_weight,
regularization_weight, **voxelnet kwargs), attributes (`_epoch`, `_adversarial_disabled`,
`_current_l2_norm`), `extract_feat`, `loss` (same keys), `predict`, `perturber`,
`disable_/enable_adversarial_training`.

extract_feat (:55-151): when the gate is open (adversary set, training, not disabled,
_epoch >= 3, :77-78) and the voxel encoder is HardSimpleVFE, the valid-slot compaction,
the perturber, the gradient-connected masked scatter and the VFE run as ONE fused kernel
sequence (VoxelPerturber.perturb_voxels) with no host synchronisation; any other voxel
encoder takes the reference's explicit compaction path. loss (:153-427) is
robustpointclouds_amd.adversarial_loss.combine_adversarial_losses — the same values with the
`.item()` branches moved onto the device. Debug prints (:98-109, :193-196, :306-365) and the
every-100-iterations manual backward (:325-338) are not reproduced.

`attack_eval()` is the attacked evaluation of evaluate_kitti_adversarial_attack.py:23-62: inside the block the gate
also opens in eval mode, and the perturber runs its eval forward.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict, List, Optional

import torch
from torch import Tensor

from robustpointclouds_amd.adversarial_loss import combine_adversarial_losses
from robustpointclouds_amd.registry import MODELS as _LOCAL_MODELS
from robustpointclouds_amd.voxelnet import HardSimpleVFE, VoxelNet

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
class AdversarialVoxelNet(VoxelNet):
    def __init__(self, adversary_cfg: Optional[dict] = None, adversarial_loss_weight: float = 1.0,
                 regularization_weight: float = 0.05, **kwargs):
        super().__init__(**kwargs)
        self.adversary = builder.build_adversary(adversary_cfg) if adversary_cfg is not None else None
        if self.adversary is not None:
            self.adversary._return_loss_dict = True
        self.adversarial_loss_weight = adversarial_loss_weight   # stored, never read (as :47)
        self.regularization_weight = regularization_weight
        self._current_l2_norm = None
        self._current_loss_dict = None
        self._epoch = 0
        self._adv_iter = 0
        self._loss_debug_iter = 0
        self._adversarial_disabled = False
        self._attack_eval = False
        self._last_flags = None
        self._last_perturbed_voxels = None

    def _gate(self):
        if getattr(self, "_attack_eval", False):
            # attacked evaluation (attack_eval below): the gate as the reference's evaluator sees it after
            # forcing the detector's own `training` on and `_adversarial_disabled` off
            return self.adversary is not None and self._epoch >= 3
        return (self.adversary is not None and self.training and
                not getattr(self, "_adversarial_disabled", False) and self._epoch >= 3)

    @contextmanager
    def attack_eval(self):
        """Attacked evaluation — what evaluate_kitti_adversarial_attack.py:23-62 adds to the stock test loop:
        inside the block the perturber runs although the detector is in eval mode (adversary present and
        `_epoch >= 3`; `_adversarial_disabled` is ignored, :37-38). The reference forces only the detector's
        own `training` attribute, so every submodule — the perturber included — stays in eval mode: the
        perturber takes its eval forward (running-statistics BatchNorm, eval bounds,
        voxel_perturber.py:214-231, 339-344), which `self.adversary.training == False` already selects here.
        No module's `training` changes; the previous `_attack_eval` is restored when the block exits, also
        when it raises."""
        prev = getattr(self, "_attack_eval", False)
        self._attack_eval = True
        try:
            yield self
        finally:
            self._attack_eval = prev

    def extract_feat(self, batch_inputs_dict: dict):
        vd = batch_inputs_dict["voxels"]
        l2, loss_dict = None, None
        voxels, npts, coors = vd["voxels"], vd["num_points"], vd["coors"]
        self._sync_engines(voxels.device)
        if hasattr(self.middle_encoder, "coors_ready"):
            self.middle_encoder.coors_ready(coors)   # its rulebooks build concurrently with the perturber
        if self._gate() and isinstance(self.voxel_encoder, HardSimpleVFE):
            feats, loss_dict, pert, flags = self.adversary.perturb_voxels(voxels, npts,
                                                                          self.voxel_encoder.num_features)
            l2 = loss_dict["l2_norm"]
            self._last_flags = flags
            self._last_perturbed_voxels = pert
        elif self._gate():
            V, P, F = voxels.shape
            flat = voxels.view(-1, F)
            valid = flat.sum(dim=1) != 0                                         # :89
            pv = flat[valid]
            if pv.shape[0] > 0:
                out, loss_dict = self.adversary(pv)
                l2 = loss_dict["l2_norm"]
                flat2 = flat + torch.zeros_like(flat)                            # :113
                flat2[valid] = out
                voxels = flat2.view(V, P, F)
            else:
                l2 = torch.tensor(0.0, device=voxels.device)
                loss_dict = {k: torch.tensor(0.0, device=voxels.device)
                             for k in ("l2_norm", "intensity_loss", "bias_loss", "imbalance_loss")}
            feats = self.voxel_encoder(voxels, npts, coors)
        else:
            feats = self.voxel_encoder(voxels, npts, coors)
        B = batch_inputs_dict.get("batch_size") or int(coors[-1, 0].item()) + 1   # :140
        x = self.middle_encoder(feats, coors, B)
        x = self.backbone(x)
        if self.with_neck:
            x = self.neck(x)
        self._current_l2_norm = l2
        self._current_loss_dict = loss_dict
        return x

    def loss(self, batch_inputs_dict: Dict[str, Tensor], batch_data_samples) -> Dict[str, Tensor]:
        x = self.extract_feat(batch_inputs_dict)
        losses_pts = self.bbox_head.loss(x, batch_data_samples)
        device = x[0].device if isinstance(x, (list, tuple)) else x.device
        if self.adversary is None:
            return dict(losses_pts)
        return combine_adversarial_losses(losses_pts, self._current_l2_norm, self._current_loss_dict, self._epoch,
                                          self.regularization_weight, self.training, device)

    @torch.no_grad()
    def predict(self, batch_inputs_dict: Dict[str, Tensor], batch_data_samples=None, **kwargs) -> List[dict]:
        """Detections per frame — dict(bboxes_3d [n, 7], scores_3d, labels_3d) — from
        `bbox_head.predict_by_feat`: box decoding, per-class rotated NMS and the direction-bin correction of
        upstream Anchor3DHead, on the HIP kernels of csrc/postprocess.hip; plus the perturbation norm when the
        adversary ran."""
        x = self.extract_feat(batch_inputs_dict)
        out = self.bbox_head.predict_by_feat(*self.bbox_head(x))
        if self._current_l2_norm is not None:
            l2 = float(self._current_l2_norm)
            for res in out:
                res["perturbation_l2_norm"] = l2
        return out

    @property
    def perturber(self):
        return self.adversary

    def get_perturbation_data(self):
        if self._last_perturbed_voxels is None:
            return None
        return {"perturbed_features": self._last_perturbed_voxels, "l2_norm": self._current_l2_norm}

    def disable_adversarial_training(self):
        self._adversarial_disabled = True
        print("Adversarial training disabled due to instability")

    def enable_adversarial_training(self):
        self._adversarial_disabled = False
        print("Adversarial training re-enabled")
