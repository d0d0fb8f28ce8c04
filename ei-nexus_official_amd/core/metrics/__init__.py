from .matching_metrics import AbsolutePoseEstimation  # noqa: F401
