"""Ground-truth geometry of the matcher validation (reference core/geometry): gt_generation, wrappers."""
