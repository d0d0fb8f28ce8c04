#!/usr/bin/env python3
"""Fixture of the homography sampler and the point warps, generated from the reference (build container only):
    python tests/golden/gen_warp.py <reference checkout>   ->  tests/golden/warp.npz
Runs the reference's own core/geometry/homography.py (numpy and torch only): `sample_homography_corners` on
np.random.RandomState(seed) for the CASES below, and `warp_points` / `warp_points_torch` on seeded points.  Stores OUTPUTS only
(H, full, warped, how many tries the convexity loop took, the generator's next draw after the call) and the recipe of every case;
the test rebuilds the inputs from the recipe."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, sys.argv[1])
from core.geometry import homography as ref  # noqa: E402

# name, seed, shape (W, H), patch_shape, keywords
CASES = [
    ("mvsec_d0", 1, (346, 260), (346, 260), dict(difficulty=0.0)),
    ("mvsec_d03", 2, (346, 260), (346, 260), dict(difficulty=0.3)),
    ("mvsec_d07", 3, (346, 260), (346, 260), dict(difficulty=0.7)),
    ("mvsec_d1", 4, (346, 260), (346, 260), dict(difficulty=1.0)),
    ("mvsec_d1_b", 5, (346, 260), (346, 260), dict(difficulty=1.0)),
    ("mvsec_patch", 6, (346, 260), (256, 192), dict(difficulty=0.7)),
    ("mvsec_noangles", 7, (346, 260), (346, 260), dict(difficulty=0.7, n_angles=0)),
    ("mvsec_notrans", 8, (346, 260), (346, 260), dict(difficulty=0.7, translation=0.0)),
    ("ec_d03", 9, (240, 180), (240, 180), dict(difficulty=0.3)),
    ("ec_d07", 10, (240, 180), (240, 180), dict(difficulty=0.7, max_angle=45, n_angles=6)),
    ("ec_patch", 11, (240, 180), (128, 96), dict(difficulty=1.0, translation=0.2)),
    ("ec_convexity", 12, (240, 180), (240, 180), dict(difficulty=1.0, min_convexity=0.2)),
]


class CountingRng:
    """the RandomState, with the calls of the convexity loop counted (its draws are the only ones made with `size=`)"""

    def __init__(self, seed):
        self.rs, self.tries = np.random.RandomState(seed), 0

    def uniform(self, *a, **kw):
        self.tries += "size" in kw
        return self.rs.uniform(*a, **kw)

    def shuffle(self, x):
        return self.rs.shuffle(x)


out, meta = {}, {"numpy": np.__version__, "torch": torch.__version__, "cases": [], "points": []}
for name, seed, shape, patch, kw in CASES:
    rng = CountingRng(seed)
    H, full, warped, patch_out = ref.sample_homography_corners(shape, patch, rng=rng, **kw)
    assert H.shape == (3, 3) and H.dtype == np.float64 and H[2, 2] == 1.0 and tuple(patch_out) == tuple(patch)
    out[f"{name}.H"], out[f"{name}.full"], out[f"{name}.warped"] = H, np.asarray(full), warped
    out[f"{name}.next"] = np.array([rng.rs.uniform()])
    meta["cases"].append({"name": name, "seed": seed, "shape": list(shape), "patch_shape": list(patch), "kw": kw, "tries": rng.tries})
    print(f"{name}: {rng.tries} tries, H =\n{H}")
assert max(c["tries"] for c in meta["cases"]) >= 2, "no case runs the rejection loop twice: pick other seeds"

prng = np.random.RandomState(99)
pts = prng.uniform(0, 300, size=(7, 2))
Hs = np.stack([out["mvsec_d07.H"], out["ec_patch.H"], out["mvsec_d03.H"]])
for inverse in (True, False):
    tag = "inv" if inverse else "fwd"
    out[f"points.single.{tag}"] = ref.warp_points(pts, Hs[0], inverse=inverse)
    out[f"points.batched.{tag}"] = ref.warp_points(pts, Hs, inverse=inverse)
    tp = torch.from_numpy(np.stack([pts, pts[::-1].copy(), pts * 0.5]))
    out[f"points.torch.{tag}"] = ref.warp_points_torch(tp, torch.from_numpy(Hs), inverse=inverse).numpy()
    out[f"points.torch1.{tag}"] = ref.warp_points_torch(tp, torch.from_numpy(Hs[1]), inverse=inverse).numpy()
out["points.flat2mat"] = ref.flat2mat(np.arange(8.0)[None])
out["points.compute"] = ref.compute_homography(np.array([[0.0, 0], [0, 2], [3, 2], [3, 0]]), np.array([[1.0, 1], [0, 3], [4, 4], [5, 0]]), [1.0, 1.0])
meta["points"] = {"seed": 99, "n": 7, "hi": 300, "H": ["mvsec_d07", "ec_patch", "mvsec_d03"]}

out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
path = os.path.join(HERE, "warp.npz")
np.savez_compressed(path, **out)
print(f"wrote {path} ({os.path.getsize(path)} bytes)")
