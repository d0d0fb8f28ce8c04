#!/usr/bin/env python3
"""Fixture of core.geometry.depth and core.geometry.epipolar, generated from the reference (build container only):
    python tests/golden/gen_geometry.py   ->  tests/golden/geometry.npz
Runs /root/reference/core/geometry/depth.py::sample_fmap / ::sample_depth / ::project / ::dense_warp_consistency and
core/geometry/epipolar.py::sym_epipolar_distance_all / ::sym_epipolar_distance / ::relative_pose_error on the CPU (through
_ref_stubs) on the cases of tests/geometry_f64.py, pair by pair (the reference has no ragged batches), and stores OUTPUTS only, in
the reference's float32, plus the torch version and the public signatures of the modules: the tests rebuild the inputs from the
same recipes.

For the one epipolar case in general position it also stores the reference's own float32 noise (`floor`: max |float32 run -
float64 run| of the reference on the same inputs) and the bound formed from it as in gen_gt_matches.py: 2 x floor + 4 ulp of the
largest distance -- what a correct float32 implementation may differ from the float64 restatement by."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_stubs  # noqa: E402
import geometry_f64 as F  # noqa: E402

_ref_stubs.install()
sys.path.insert(0, "/root/reference")
from core.geometry import depth as ref_depth  # noqa: E402
from core.geometry import epipolar as ref_epi  # noqa: E402
from core.geometry import utils as ref_utils  # noqa: E402
from core.geometry.wrappers import Camera, Pose  # noqa: E402
from core.metrics import util as ref_mutil  # noqa: E402

torch.set_num_threads(1)
out = {}
meta = {"torch": torch.__version__}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def signatures(mod, names):
    sig = {}
    for n in names:
        fn = getattr(mod, n)
        try:
            sig[n] = str(inspect.signature(fn))
        except (TypeError, ValueError):  # a scripted function: its schema is not a Python signature
            sig[n] = None
    return sig


meta["signatures"] = {
    "depth": signatures(ref_depth, ["sample_fmap", "sample_depth", "sample_normals_from_depth", "project", "dense_warp_consistency"]),
    "epipolar": signatures(ref_epi, ["T_to_E", "T_to_F", "E_to_F", "F_to_E", "sym_epipolar_distance", "sym_epipolar_distance_all",
                                     "generalized_epi_dist", "decompose_essential_matrix", "angle_error_mat", "angle_error_vec",
                                     "relative_pose_error"]),
    "utils": signatures(ref_utils, ["to_homogeneous", "from_homogeneous", "batched_eye_like", "skew_symmetric", "transform_points", "is_inside",
                                    "so3exp_map", "get_image_coords"]),
    "metrics_util": signatures(ref_mutil, ["warp_points", "filter_points", "keep_true_points", "select_k_best_points"])}

# ---- the samplers
fm, pts = F.sample_case(3)
out["sample_fmap"] = ref_depth.sample_fmap(_t(pts), _t(fm)).numpy()
fm1, pts1 = F.sample_case(1)
d, v = ref_depth.sample_depth(_t(pts1), _t(fm1[:, 0]))
out["sample_depth.d"], out["sample_depth.valid"] = d.numpy(), v.numpy()

# ---- project on the occlusion scene, sampled depths, both directions, pair by pair
c = F.occlusion_scene(257)
for b in range(c.B):
    cam0, cam1 = Camera.from_calibration_matrix(_t(c.K0[b:b + 1])), Camera.from_calibration_matrix(_t(c.K1[b:b + 1]))
    T01, T10 = Pose.from_4x4mat(_t(c.T01[b:b + 1])), Pose.from_4x4mat(_t(c.T10[b:b + 1]))
    for side, (kp, own, other, ci, cj, T) in enumerate(((c.kp0[b], c.depth0[b], c.depth1[b], cam0, cam1, T01),
                                                        (c.kp1[b], c.depth1[b], c.depth0[b], cam1, cam0, T10))):
        kp, own, other = _t(kp)[None], _t(own)[None], _t(other)[None]
        d, valid = ref_depth.sample_depth(kp, own)
        for tag, ccth in (("none", None), ("eq", F.BOUND_EQ), ("above", F.BOUND_ABOVE)):
            uv, vis = ref_depth.project(kp, d, other, ci, cj, T, valid, ccth=ccth)
            out[f"project.{b}.{side}.{tag}.proj"], out[f"project.{b}.{side}.{tag}.visible"] = uv.numpy()[0], vis.numpy()[0]

# ---- dense_warp_consistency
for name in F.DENSE_SHAPES:
    dc = F.dense_case(name)
    for b in range(dc.B):
        ci, cj = Camera.from_calibration_matrix(_t(dc.K_i[b:b + 1])), Camera.from_calibration_matrix(_t(dc.K_j[b:b + 1]))
        T = Pose.from_4x4mat(_t(dc.T[b:b + 1]))
        for tag, ccth in (("none", None), ("eq", F.BOUND_EQ), ("above", F.BOUND_ABOVE)):
            warp, vis = ref_depth.dense_warp_consistency(_t(dc.depth_i[b:b + 1]), _t(dc.depth_j[b:b + 1]), T, ci, cj, ccth=ccth)
            out[f"dense.{name}.{b}.{tag}.warp"], out[f"dense.{name}.{b}.{tag}.visible"] = warp.numpy()[0], np.packbits(vis.numpy()[0])

# ---- the epipolar distances
for n, m in F.EPI_SHAPES:
    p0, p1, E = F.epipolar_case(n, m)
    keep = slice(0, 1) if n * m > 50000 else slice(None)  # the largest case: its first pair only (the file's size)
    out[f"epi_all.{n}x{m}"] = ref_epi.sym_epipolar_distance_all(_t(p0[keep]), _t(p1[keep]), _t(E[keep])).numpy()
p0, p1, E = F.epipolar_case(260, 260, cols=(2, 3))
for sq in (True, False):
    out[f"epi_pairs.{int(sq)}"] = ref_epi.sym_epipolar_distance(_t(p0), _t(p1), _t(E), squared=sq).numpy()
p0, p1, Fm = F.general_epipolar_case()
r32 = ref_epi.sym_epipolar_distance_all(_t(p0), _t(p1), _t(Fm)).numpy()
r64 = ref_epi.sym_epipolar_distance_all(_t(p0).double(), _t(p1).double(), _t(Fm).double()).numpy()
floor = float(np.abs(r32.astype(np.float64) - r64).max())
out["epi_general"] = r32
meta["epi_general"] = {"floor": floor, "bound": 2 * floor + 4 * float(np.spacing(np.float32(np.abs(r64).max()))), "max": float(np.abs(r64).max())}

# ---- relative_pose_error
T, estimates = F.pose_error_case()
out["pose_error"] = np.array([[float(x) for x in ref_epi.relative_pose_error(_t(T), _t(R), _t(t))] for R, t in estimates], np.float32)

out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
path = os.path.join(HERE, "geometry.npz")
np.savez_compressed(path, **out)
print(meta["epi_general"], os.path.getsize(path), "bytes")
assert os.path.getsize(path) < (1 << 20)
