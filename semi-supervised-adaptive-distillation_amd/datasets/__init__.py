"""Evaluators (the reference keeps its own under detectron/lib/datasets/)."""
from .detection_evaluator import DetectionEvaluator  # noqa: F401
