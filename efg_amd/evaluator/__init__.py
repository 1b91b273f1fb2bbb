"""`efg.evaluator` surface: dataset evaluators that stream over the loader (efg/evaluator/__init__.py)."""
from .evaluator import DatasetEvaluator, inference_on_dataset  # noqa: F401
from .nuscenes import NuScenesDetEvaluator, nuScenesDetEvaluator  # noqa: F401
from .waymo import WaymoDetEvaluator  # noqa: F401
from .waymo_track import WaymoTrackEvaluator  # noqa: F401

__all__ = ["DatasetEvaluator", "NuScenesDetEvaluator", "WaymoDetEvaluator", "WaymoTrackEvaluator", "inference_on_dataset",
           "nuScenesDetEvaluator"]
