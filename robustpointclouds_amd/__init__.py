from .evaluate import evaluate, robustness_report  # noqa: F401
from .gt_augment import GpuObjectNoise, GpuObjectSample, GtDatabase, points_in_boxes  # noqa: F401
