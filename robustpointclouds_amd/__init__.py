from .evaluate import evaluate, robustness_report  # noqa: F401
