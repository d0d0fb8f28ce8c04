#!/usr/bin/env python3
"""Fixture of the ground-truth matches and of matcher_metrics, generated from the reference (build container only):
    python tests/golden/gen_gt_matches.py   ->  tests/golden/gt_matches.npz
Runs /root/reference/core/geometry/gt_generation.py::gt_matches_from_pose_depth / ::gt_matches_from_homography and
core/modules/matchers/lightglue.py::matcher_metrics on the CPU (through _ref_stubs) on the integer-built scenes of
tests/gt_matches_ref.py, pair by pair (the reference has no ragged batches), and stores OUTPUTS only: the tests rebuild the inputs
from the same recipes.  Per pose case it also stores

  floors   the reference's own float32 noise: max |reference - float64 restatement| over proj_* (pixels), the sampled depths and
           epi_dist (pixels),
  margins  how far the reference's discrete decisions sit from their thresholds, in the units of the matching floor: `front`
           (|q.z - 1e-4| relative to |q.z| + 1, depth floor), `inside` on the four borders (pixels), sqrt(dist) against pos_th at
           every visible entry, sqrt(row / column min dist0 / dist1) against neg_th, the first-to-second arg-min gap of sqrt(dist) in
           every row / column whose minimum is below pos_th (only there can the arg-min reach an output: a positive needs
           dist < pos_th^2 at the mutual arg-min; bit-identical duplicate candidates are exempt, the lowest index decides them
           exactly), and epi_dist against neg_th,
  bounds   2 x floor + 4 ulp of the largest coordinate / depth: what a correct float32 implementation may differ from the reference by.

Seeds are searched until every margin is at least MARGIN x its floor, so the tests compare every discrete output exactly, with
no flip budget.  The full-size case (1024 x 1023: a million continuous entries of `reward`) cannot clear 16 floors at EVERY entry
of the dense matrix for any seed; there the O(N + M) decisions must clear them, and the few dense entries that do not are listed
(`reward_unsure`, flat indices) -- the reference itself is not reproducible at those."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_stubs  # noqa: E402
import gt_matches_ref as R  # noqa: E402

_ref_stubs.install()
sys.path.insert(0, "/root/reference")
from core.geometry import gt_generation as ref_gt  # noqa: E402
from core.geometry.epipolar import T_to_E, sym_epipolar_distance_all  # noqa: E402
from core.geometry.wrappers import Camera, Pose  # noqa: E402
from core.modules.matchers.lightglue import matcher_metrics as ref_matcher_metrics  # noqa: E402

MARGIN = 16.0
torch.set_num_threads(1)
out = {}
meta = {"torch": torch.__version__, "margin_factor": MARGIN, "cases": []}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def run_pose_pair(sc, b, ordering, pos_th, neg_th, pre=None):
    n, m = int(sc["n"][b]), int(sc["m"][b])
    kp0, kp1 = sc["kp0"][b:b + 1, :n], sc["kp1"][b:b + 1, :m]
    if ordering == "yx":
        kp0, kp1 = kp0[..., ::-1].copy(), kp1[..., ::-1].copy()
    cam0 = Camera.from_calibration_matrix(_t(sc["K0"][b:b + 1]))
    cam1 = Camera.from_calibration_matrix(_t(sc["K1"][b:b + 1]))
    T01, T10 = Pose.from_4x4mat(_t(sc["T01"][b:b + 1])), Pose.from_4x4mat(_t(sc["T10"][b:b + 1]))
    kw = {}
    if pre is not None:
        kw = {"depth_keypoints0": _t(pre[0])[None], "valid_depth_keypoints0": _t(pre[1])[None], "depth_keypoints1": _t(pre[2])[None],
              "valid_depth_keypoints1": _t(pre[3])[None]}
    r = ref_gt.gt_matches_from_pose_depth(_t(kp0), _t(kp1), cam0, cam1, _t(sc["depth0"][b:b + 1]), _t(sc["depth1"][b:b + 1]), T01, T10,
                                          pos_th=pos_th, neg_th=neg_th, ordering=ordering, **kw)
    if isinstance(r, tuple):
        return {"tuple": [x.numpy()[0] for x in r]}
    res = {k: v.numpy()[0] for k, v in r.items()}
    F = cam1.calibration_matrix().inverse().transpose(-1, -2) @ T_to_E(T01) @ cam0.calibration_matrix().inverse()
    res["epi"] = sym_epipolar_distance_all(_t(sc["kp0"][b:b + 1, :n]), _t(sc["kp1"][b:b + 1, :m]), F).numpy()[0]
    return res


def _gap(key, axis, limit):
    """first-to-second gap of every row (axis 1) / column (axis 0) whose minimum is below `limit`; inf where there is none"""
    if key.shape[axis] < 2:
        return np.inf
    s = np.sort(key, axis=axis)
    first, second = np.take(s, 0, axis), np.take(s, 1, axis)
    sel = first < limit
    return float((second - first)[sel].min()) if sel.any() else np.inf


def pose_margins(sc, b, res, pos_th, neg_th, pre=None):
    """floors, margins (each divided by its floor's unit: see the module docstring) and the unsure dense entries of one pair"""
    n, m = int(sc["n"][b]), int(sc["m"][b])
    e = R.project(sc, b, np.float64, depths=pre)
    kp0, kp1 = sc["kp0"][b, :n].astype(np.float64), sc["kp1"][b, :m].astype(np.float64)

    def err(a, x):
        a, x = np.asarray(a, np.float64), np.asarray(x, np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(x)), "NaN pattern of the reference differs from the float64 restatement"
        fin = ~np.isnan(a)
        return float(np.abs(a - x)[fin].max()) if fin.any() else 0.0
    assert np.array_equal(res["visible0"], e["visible0"]) and np.array_equal(res["visible1"], e["visible1"])
    floors = {"proj": max(err(res["proj_0to1"], e["proj01"]), err(res["proj_1to0"], e["proj10"]), 1e-7),
              "depth": max(err(res["depth_keypoints0"], e["d0"]), err(res["depth_keypoints1"], e["d1"]), 1e-8)}
    epi = R.epipolar_all(kp0, kp1, sc["K0"][b], sc["K1"][b], sc["T01"][b])
    floors["epi"] = max(err(res["epi"], epi), 1e-7)
    mg = {}
    front, inside = [], []
    for side, valid in ((e["side0"], e["valid0"]), (e["side1"], e["valid1"])):
        qz = side["qz"][valid]
        front.append(np.abs(qz - 1e-4) / (np.abs(qz) + 1))
        vf = valid & side["front"]
        u, v = side["proj"][vf, 0], side["proj"][vf, 1]
        inside.append(np.concatenate([np.abs(u), np.abs(u - side["wmax"]), np.abs(v), np.abs(v - side["hmax"])]))
    front, inside = np.concatenate(front), np.concatenate(inside)
    mg["front"] = (float(front.min()) if front.size else np.inf) / floors["depth"]
    mg["inside"] = (float(inside.min()) if inside.size else np.inf) / floors["proj"]
    # the distances in float64 from the float64 projections
    d0 = ((e["proj01"][:, None] - kp1[None]) ** 2).sum(-1)
    d1 = ((kp0[:, None] - e["proj10"][None]) ** 2).sum(-1)
    vis = e["visible0"][:, None] & e["visible1"][None]
    with np.errstate(invalid="ignore"):
        rd = np.sqrt(np.where(vis, np.fmax(d0, d1), np.inf))
        near0, near1 = np.sqrt(np.nanmin(np.where(np.isnan(d0), np.inf, d0), 1)), np.sqrt(np.nanmin(np.where(np.isnan(d1), np.inf, d1), 0))
    pos_m = np.abs(rd - pos_th)
    epi_m = np.abs(epi - neg_th)
    near = np.concatenate([near0[e["valid0"]], near1[e["valid1"]]])
    mg["neg"] = (float(np.abs(near - neg_th).min()) if near.size else np.inf) / floors["proj"]
    # arg-min gaps: exact duplicates (identical keypoint AND projection) are decided by the index, not by a float
    key = rd.copy()
    _, first1 = np.unique(np.concatenate([sc["kp1"][b, :m], res["proj_1to0"]], 1).view(np.uint32), axis=0, return_index=True)
    _, first0 = np.unique(np.concatenate([sc["kp0"][b, :n], res["proj_0to1"]], 1).view(np.uint32), axis=0, return_index=True)
    mg["argmin"] = min(_gap(key[:, np.sort(first1)], 1, pos_th), _gap(key[np.sort(first0)], 0, pos_th)) / floors["proj"]
    unsure = np.nonzero(((pos_m < MARGIN * floors["proj"]) | (epi_m < MARGIN * floors["epi"])).reshape(-1))[0]
    mg["reward_pos"] = float(pos_m.min()) / floors["proj"]
    mg["reward_epi"] = float(epi_m.min()) / floors["epi"]
    # the mutual positives themselves: dist at the reference's matches against pos_th (an O(N + M) decision)
    return floors, mg, unsure


def store_pair(tag, res, sc, b):
    for k in ("matches0", "matches1"):
        out[f"{tag}.{k}"] = res[k].astype(np.int16)
    out[f"{tag}.assignment"] = np.packbits(res["assignment"])
    out[f"{tag}.reward"] = res["reward"].astype(np.int8)
    assert np.array_equal(res["reward"], res["reward"].astype(np.int8))
    for k in ("depth_keypoints0", "depth_keypoints1", "proj_0to1", "proj_1to0"):
        out[f"{tag}.{k}"] = res[k].astype(np.float32)
    for k in ("visible0", "visible1"):
        out[f"{tag}.{k}"] = res[k]
    out[f"{tag}.dtypes"] = np.frombuffer(json.dumps({k: str(v.dtype) for k, v in res.items() if k != "epi"}).encode(), np.uint8)


def bounds(floors, sc):
    coord = float(max(np.abs(sc["kp0"]).max(), np.abs(sc["kp1"]).max(), 2 * sc["K0"][:, :2, 2].max(), 2 * sc["K1"][:, :2, 2].max()))
    depth = float(np.nanmax(np.abs(np.concatenate([sc["depth0"].reshape(-1), sc["depth1"].reshape(-1)]))))
    return {"proj": 2 * floors["proj"] + 4 * float(np.spacing(np.float32(coord))), "depth": 2 * floors["depth"] + 4 * float(np.spacing(np.float32(depth)))}


def pose_case(name, make, ordering, pos_th, neg_th, dense_margins=True, use_pre=False, first_seed=1, tries=200):
    for seed in range(first_seed, first_seed + tries):
        sc = make(seed)
        floors, margins, results, unsure_all, ok = {}, {}, [], [], True
        for b in range(len(sc["n"])):
            pre = None
            if use_pre:  # precomputed depths: the float64 restatement's samples rounded to float32 (the tests rebuild them)
                n, m = int(sc["n"][b]), int(sc["m"][b])
                d0, v0 = R.sample_depth(sc["kp0"][b, :n], sc["depth0"][b], np.float64)
                d1, v1 = R.sample_depth(sc["kp1"][b, :m], sc["depth1"][b], np.float64)
                pre = (d0.astype(np.float32), v0, d1.astype(np.float32), v1)
            res = run_pose_pair(sc, b, ordering, pos_th, neg_th, pre)
            results.append(res)
            if "tuple" in res:
                unsure_all.append(np.zeros(0, np.int64))
                continue
            f, mg, unsure = pose_margins(sc, b, res, pos_th, neg_th, pre)
            for k, v in f.items():
                floors[k] = max(floors.get(k, 0.0), v)
            for k, v in mg.items():
                margins[k] = min(margins.get(k, np.inf), v)
            unsure_all.append(unsure)
        need = ["front", "inside", "neg", "argmin"] + (["reward_pos", "reward_epi"] if dense_margins else [])
        ok = all(margins[k] >= MARGIN for k in need)
        # without the dense margins the mutual positives still have to clear pos_th: checked through the matches themselves
        if ok and not dense_margins:
            for b, res in enumerate(results):
                if "tuple" in res:
                    continue
                e = R.project(sc, b, np.float64)
                for i, j in enumerate(res["matches0"]):
                    if j >= 0 or res["assignment"][i].any():
                        jj = int(np.argmax(res["assignment"][i])) if res["assignment"][i].any() else j
                        d = max(((e["proj01"][i] - sc["kp1"][b, jj]) ** 2).sum(), ((sc["kp0"][b, i] - e["proj10"][jj]) ** 2).sum())
                        ok &= abs(np.sqrt(d) - pos_th) >= MARGIN * floors["proj"]
        print(name, "seed", seed, "floors", floors, "margins", {k: round(v, 1) for k, v in margins.items()}, "ok" if ok else "rejected")
        if ok:
            break
    else:
        raise SystemExit(f"{name}: no seed with every margin >= {MARGIN} floors")
    for b, res in enumerate(results):
        tag = f"{name}.{b}"
        if "tuple" in res:
            for k, v in zip(("assignment", "matches0", "matches1"), res["tuple"]):
                out[f"{tag}.tuple.{k}"] = v
            continue
        store_pair(tag, res, sc, b)
        out[f"{tag}.reward_unsure"] = unsure_all[b].astype(np.int64)
        assert dense_margins is False or unsure_all[b].size == 0
    meta["cases"].append({"name": name, "seed": seed, "ordering": ordering, "pos_th": pos_th, "neg_th": neg_th, "floors": floors,
                          "margins": {k: (v if np.isfinite(v) else 1e30) for k, v in margins.items()}, "bounds": bounds(floors, sc),
                          "B": len(sc["n"]), "dense_margins": dense_margins, "kind": "pose"})


def homography_case(name, B, n, m, pos_th, neg_th, first_seed=1, tries=200):
    for seed in range(first_seed, first_seed + tries):
        sc = R.homography_scene(seed, B, n, m)
        r = ref_gt.gt_matches_from_homography(_t(sc["kp0"]), _t(sc["kp1"]), _t(sc["H"]), pos_th=pos_th, neg_th=neg_th)
        res = {k: v.numpy() for k, v in r.items()}
        floor, mg = 1e-7, {"reward_pos": np.inf, "reward_neg": np.inf, "neg": np.inf, "argmin": np.inf}
        for b in range(B):
            p01 = R.warp(sc["kp0"][b], sc["H"][b], np.float64)
            p10 = R.warp(sc["kp1"][b], np.linalg.inv(sc["H"][b].astype(np.float64)), np.float64)
            floor = max(floor, float(np.abs(res["proj_0to1"][b] - p01).max()), float(np.abs(res["proj_1to0"][b] - p10).max()))
        for b in range(B):
            kp0, kp1 = sc["kp0"][b].astype(np.float64), sc["kp1"][b].astype(np.float64)
            p01 = R.warp(sc["kp0"][b], sc["H"][b], np.float64)
            p10 = R.warp(sc["kp1"][b], np.linalg.inv(sc["H"][b].astype(np.float64)), np.float64)
            d0, d1 = ((p01[:, None] - kp1[None]) ** 2).sum(-1), ((kp0[:, None] - p10[None]) ** 2).sum(-1)
            rd = np.sqrt(np.maximum(d0, d1))
            mg["reward_pos"] = min(mg["reward_pos"], float(np.abs(rd - pos_th).min()) / floor)
            mg["reward_neg"] = min(mg["reward_neg"], float(np.abs(rd - neg_th).min()) / floor)
            near = np.concatenate([np.sqrt(d0.min(1)), np.sqrt(d1.min(0))])
            mg["neg"] = min(mg["neg"], float(np.abs(near - neg_th).min()) / floor)
            _, first1 = np.unique(np.concatenate([sc["kp1"][b], res["proj_1to0"][b]], 1).view(np.uint32), axis=0, return_index=True)
            _, first0 = np.unique(np.concatenate([sc["kp0"][b], res["proj_0to1"][b]], 1).view(np.uint32), axis=0, return_index=True)
            mg["argmin"] = min(mg["argmin"], _gap(rd[:, np.sort(first1)], 1, pos_th) / floor, _gap(rd[np.sort(first0)], 0, pos_th) / floor)
        ok = all(v >= MARGIN for v in mg.values())
        print(name, "seed", seed, "floor", floor, "margins", {k: round(v, 1) for k, v in mg.items()}, "ok" if ok else "rejected")
        if ok:
            break
    else:
        raise SystemExit(f"{name}: no seed with every margin >= {MARGIN} floors")
    for k in ("matches0", "matches1"):
        out[f"{name}.{k}"] = res[k].astype(np.int16)
    out[f"{name}.assignment"] = np.packbits(res["assignment"])
    out[f"{name}.reward"] = res["reward"].astype(np.int8)
    for k in ("proj_0to1", "proj_1to0"):
        out[f"{name}.{k}"] = res[k]
    out[f"{name}.dtypes"] = np.frombuffer(json.dumps({k: str(v.dtype) for k, v in res.items()}).encode(), np.uint8)
    coord = float(max(np.abs(res["proj_0to1"]).max(), np.abs(res["proj_1to0"]).max()))
    meta["cases"].append({"name": name, "seed": seed, "B": B, "n": n, "m": m, "pos_th": pos_th, "neg_th": neg_th, "floors": {"proj": floor},
                          "margins": mg, "bounds": {"proj": 2 * floor + 4 * float(np.spacing(np.float32(coord)))}, "kind": "homography"})


def pr_cases_store():
    for name, (m, gt, sc) in R.pr_cases().items():
        r = ref_matcher_metrics({"matches0": _t(m), "matching_scores0": _t(sc)}, {"gt_matches0": _t(gt)})
        out[f"pr.{name}"] = np.stack([r[k].numpy() for k in ("match_recall", "match_precision", "accuracy", "average_precision")], 1)
        print("pr", name, out[f"pr.{name}"].tolist())


pose_case("a", R.scene_a, "yx", 3, 5)
pose_case("b", R.scene_b, "xy", 3, 5, use_pre=True)
homography_case("c", 2, 65, 130, 3, 6)
homography_case("c_neg_lt_pos", 2, 65, 130, 3, 2)
pose_case("d", R.scene_d, "yx", 3, 5, dense_margins=False)
pr_cases_store()
out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
path = os.path.join(HERE, "gt_matches.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
assert os.path.getsize(path) < (1 << 20)
