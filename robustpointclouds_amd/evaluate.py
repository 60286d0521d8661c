"""Model-level evaluation: detection quality clean, under the perturber's attack, and the drop.

`evaluate` is the test loop of the reference's evaluate_kitti_adversarial_attack.py with the metric of its
`val_evaluator` (configs/_base_/kitti-3d-car.py: KittiMetric) replaced by kitti_eval.KittiAP: the model in
eval mode, `val_step` batch by batch — inside `model.attack_eval()` for the attacked run — and every batch's
detections and ground truth handed to the metric. No dataset loader: a batch is a pair (data, gts) with
`data` what `val_step` takes and `gts` the per-frame ground truth `KittiAP.update` takes.
"""
from __future__ import annotations

import contextlib

from .kitti_eval import KittiAP

__all__ = ["evaluate", "robustness_report"]


def evaluate(model, batches, metric, attacked: bool = False) -> dict:
    """Run `model` over `batches` ((data, gts) pairs) in eval mode and return `metric.compute()`. The metric is
    reset first. attacked: run inside `model.attack_eval()` (the eval-mode perturber in front of the detector);
    a model without `attack_eval` cannot be evaluated under attack and raises TypeError. The training flag of
    every module is put back afterwards, also when a batch raises."""
    if attacked and not hasattr(model, "attack_eval"):
        raise TypeError(f"{type(model).__name__} has no attack_eval(): it cannot be evaluated under attack")
    modes = [(m, m.training) for m in model.modules()]
    metric.reset()
    model.eval()
    try:
        with (model.attack_eval() if attacked else contextlib.nullcontext()):
            for data, gts in batches:
                metric.update(model.val_step(data), gts)
    finally:
        for m, training in modes:   # parents come first: a child's own mode is set after its parent's recursion
            m.train(training)
    return metric.compute()


def robustness_report(model, batches, class_names, min_overlaps=None, metric=None) -> dict:
    """{"clean": AP without the attack, "attacked": AP inside attack_eval(), "drop": clean - attacked per key}
    over the same batches (a list, or any iterable that can be walked twice). metric: an object with reset /
    update / compute (nuscenes_eval.NuScenesDetectionScore for AdversarialCenterPoint) to use in place of the
    KittiAP built from `class_names` and `min_overlaps`, which are then ignored. For a metric's error keys
    (mATE, ..._err) a negative drop means the error GREW under attack; a NaN value gives a NaN drop."""
    batches = batches if isinstance(batches, (list, tuple)) else list(batches)
    if metric is None:
        metric = KittiAP(class_names, min_overlaps)
    clean = evaluate(model, batches, metric, attacked=False)
    attacked = evaluate(model, batches, metric, attacked=True)
    return {"clean": clean, "attacked": attacked, "drop": {k: clean[k] - attacked[k] for k in clean}}
