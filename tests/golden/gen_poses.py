#!/usr/bin/env python3
"""Fixture of the pose tracks and the depth / image pairing, generated from the reference (build container only; needs scipy):
    python tests/golden/gen_poses.py <reference checkout>   ->  tests/golden/poses.npz
Runs the reference's own datasets/Interpolator.py::PoseInterpolator (scipy Slerp + three linear interp1d + np.linalg.inv), one
`interpolate` call per query as its datasets make them, on the seeded tracks of tests/poses_f64.py::TRACK_CASES and stores OUTPUTS
only, in float64 (the test rebuilds tracks and queries from the recipe).  Also stores what numpy's outer-difference argmin
(datasets/MVSEC.py:364-366) gives on tests/poses_f64.py::PAIRING_CASES.

The restatement (tests/poses_f64.py) is the contract of the kernels; this fixture shows that the reference agrees with it.  The
shorter arc between two knots is ambiguous at a half turn, so the generator refuses a track with a neighbouring pair within
0.1 rad of one."""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import poses_f64 as P  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_interpolator", os.path.join(sys.argv[1], "datasets", "Interpolator.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

import scipy  # noqa: E402

out, meta = {}, {"scipy": scipy.__version__, "numpy": np.__version__, "cases": []}
worst, total = 0.0, 0
for name, kw, quat in P.TRACK_CASES:
    stamps, t, R, quat_R, queries = P.track_case(name)
    assert quat_R == quat
    ang = P.neighbour_angles(P.matrix_from_quat(P.knots(R, quat_R)))
    assert (ang < np.pi - 0.1).all(), (name, ang.max())
    interp = ref.PoseInterpolator(stamps, t, R, quat_R=quat_R)
    with contextlib.redirect_stdout(io.StringIO()):  # (its range message: none of these queries is outside)
        poses = np.stack([interp.interpolate(np.float64(q)) for q in queries])
    assert poses.dtype == np.float64 and np.isfinite(poses).all()
    mine, bad = P.interpolate(stamps, t, P.knots(R, quat_R), queries)
    assert bad == 0
    scale = np.maximum(1.0, np.abs(poses[:, :3, 3]).max(1))
    diff = float((np.abs(mine - poses).max((1, 2)) / scale).max())
    worst, total = max(worst, diff), total + len(queries)
    out[f"{name}.poses"] = poses
    meta["cases"].append({"name": name, "queries": int(len(queries)), "max_neighbour_angle": float(ang.max()),
                          "min_neighbour_angle": float(ang.min()), "restatement_scaled_diff": diff})
    print(f"{name}: {len(queries)} queries, neighbour angles {ang.min():.3g} .. {ang.max():.3g} rad, restatement differs by {diff:.3g} (scaled)")

meta["pairing"] = []
for name, (stamps, queries) in P.PAIRING_CASES.items():
    idx = P.nearest_index_dense(stamps, queries)
    out[f"pairing.{name}"] = idx
    meta["pairing"].append(name)
    print(f"pairing {name}: {idx.tolist()}")

meta["restatement_worst_scaled_diff"] = worst
meta["queries"] = total
out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
path = os.path.join(HERE, "poses.npz")
np.savez_compressed(path, **out)
print(f"{path}: {os.path.getsize(path)} bytes, {total} queries, worst scaled float64 difference {worst:.3g}")
