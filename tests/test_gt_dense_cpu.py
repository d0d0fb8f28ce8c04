"""Dense-grid ground-truth matches and pair covisibility, the part that needs no GPU: the exactness claim the GPU
companion (test_gt_dense_gpu.py) rests on, the situations its cases plant, the new symbols, select_pairs' bookkeeping on a fake
covisibility, and the dense restatement against the reference's fixture (tests/golden/gt_dense.npz)."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import gt_dense_f64 as D
from helpers import Golden, load_pkg

pkg = load_pkg()
F32 = np.float32


def _all(name):
    c = D.case(name)
    return [(c, b, e) for b, e in enumerate(D.expected(name))]


# ------------------------------------------------------------------------------------------------ (a) exactness
@pytest.mark.parametrize("name", D.CASES)
def test_fp32_evaluation_is_exact_for_every_gpu_case(name):
    """evaluated in float32 the dense restatement gives its float64 result bit for bit, on every case and every output the GPU test
    compares: that licenses array_equal there"""
    c = D.case(name)
    for a in (c.depth0, c.depth1, c.K0, c.K1, c.T01, c.T10):
        assert a.dtype == F32
    for b, (e64, e32) in enumerate(zip(D.expected(name), D.expected(name, F32))):
        for k in D.COMPARED:
            assert np.asarray(e32[k]).dtype in (F32, np.bool_, np.int64, np.int32), (name, b, k)
            assert np.array_equal(np.asarray(e64[k], np.float64), np.asarray(e32[k], np.float64), equal_nan=True), (name, b, k)
        for k in ("near0", "near1", "dmin0", "dmin1", "min0", "min1"):
            assert np.array_equal(np.asarray(e64["lab"][k], np.float64), np.asarray(e32["lab"][k], np.float64), equal_nan=True), (name, b, k)


# ------------------------------------------------------------------------------------------------ (b) planted situations
def _clipped(c, e, side):
    """per matched pixel of `side`: does its candidate box |x + 0.5 - p| <= pos_th + 1 reach beyond the other map (l, r, t, b)?"""
    p, m = (e["proj_0to1"], e["matches0"]) if side == 0 else (e["proj_1to0"], e["matches1"])
    H, W = c.size1 if side == 0 else c.size0
    r = c.pos_th + 1
    ok = m > -1
    return ok & (p[:, 0] - r < 0), ok & (p[:, 0] + r > W), ok & (p[:, 1] - r < 0), ok & (p[:, 1] + r > H)


def test_windows_are_clipped_at_every_border_and_at_a_corner():
    seen = np.zeros(5, bool)
    for name in D.CASES:
        for c, b, e in _all(name):
            for side in (0, 1):
                left, right, top, bottom = _clipped(c, e, side)
                seen[:4] |= [left.any(), right.any(), top.any(), bottom.any()]
                seen[4] |= ((left | right) & (top | bottom)).any()
    assert seen.all(), seen


def test_projections_on_and_beside_the_camera_border():
    c = D.case("borders")
    wmax = 2 * c.K1[0, 0, 2] - 1
    e0, e1, e2 = D.expected("borders")[:3]
    u0, u1, u2 = e0["proj_0to1"][:, 0], e1["proj_0to1"][:, 0], e2["proj_0to1"][:, 0]
    assert (e0["visible0"] & (u0 == 0)).any() and (e0["visible0"] & (u0 == wmax)).any()
    assert (e1["valid0"] & ~e1["visible0"] & (u1 == -0.25)).any() and not (e1["visible0"] & (u1 < 0)).any()
    assert (e2["valid0"] & ~e2["visible0"] & (u2 == wmax + 0.25)).any() and not (e2["visible0"] & (u2 > wmax)).any()


def test_projections_outside_the_image_by_more_and_by_less_than_neg_th():
    c, e = D.case("borders"), D.expected("borders")[3]
    u, near = e["proj_0to1"][:, 0], np.sqrt(e["lab"]["near0"])
    far = e["valid0"] & (u < -c.neg_th)
    close = e["valid0"] & (u < 0) & (near < c.neg_th)
    assert far.any() and (near[far] > c.neg_th).all() and (e["matches0"][far] == -1).all()
    assert close.any() and not e["visible0"][close].any() and (e["matches0"][close] == -2).all()


def test_two_pixels_across_a_depth_step_share_a_projection():
    """columns 5 (depth 1) and 6 (depth 2) of rows 2-4 land on one location: the lower raster index is matched, the other ignored"""
    c, e = D.case("step"), D.expected("step")[0]
    W = c.size0[1]
    for y in (2, 3, 4):
        i, j = y * W + 5, y * W + 6
        assert c.depth0[0, y, 5] == 1 and c.depth0[0, y, 6] == 2 and e["visible0"][i] and e["visible0"][j]
        assert np.array_equal(e["proj_0to1"][i], e["proj_0to1"][j])
        assert e["matches0"][i] > -1 and e["matches0"][j] == -2
        assert e["matches1"][e["matches0"][i]] == i
    # and exact ties between candidates decide matches all over the half-pixel pairs: the lowest raster index wins them
    lab = D.expected("borders")[0]["lab"]
    assert (lab["tied0"] & (lab["dmin0"] < 9)).sum() > 50 and (lab["tied1"] & (lab["dmin1"] < 9)).sum() > 50
    assert (lab["min0"][lab["tied0"]] < lab["last0"][lab["tied0"]]).all()


def test_dist_equal_to_pos_th_squared_is_no_positive():
    """candidates at dist == pos_th^2 exactly: earlier in raster order than the row's match (a smaller value), and as the minimum of
    a row, which then has no positive"""
    hit_before, hit_min = 0, 0
    for name in ("borders", "neg_lt_pos"):
        for c, b, e in _all(name):
            lab, pos_sq = e["lab"], c.pos_th ** 2
            if not lab["at_pos"]:
                continue
            full = D.label(e["kp0"], e["kp1"], e["proj_0to1"], e["proj_1to0"], e["visible0"], e["visible1"], e["valid0"], e["valid1"],
                           c.pos_th, c.neg_th, keep=True)
            at = full["dist"] == pos_sq
            first_at = np.where(at.any(1), at.argmax(1), at.shape[1])
            hit_before += int(((e["matches0"] > -1) & (first_at < e["matches0"])).sum())
            rows = lab["dmin0"] == pos_sq
            hit_min += int(rows.sum())
            assert (lab["pos0"][rows] == -1).all()
    assert hit_before > 0 and hit_min > 0, (hit_before, hit_min)


def test_a_row_that_is_positive_and_negative_is_unmatched():
    c, e = D.case("neg_lt_pos"), D.expected("neg_lt_pos")[0]
    assert c.neg_th < c.pos_th
    y, x = D.NEG_LT_POS_ROW
    i = y * c.size0[1] + x
    assert e["lab"]["pos0"][i] == y * c.size1[1] + 15 and e["visible0"][i]
    assert e["lab"]["near0"][i] == 9 > c.neg_th ** 2 and e["matches0"][i] == -1
    assert e["lab"]["dmin0"][i] == 9 < c.pos_th ** 2


def test_thresholds_holes_and_poses_the_cases_cover():
    assert D.case("step").pos_th == 2.5
    for name in D.CASES:
        c = D.case(name)
        if name == "behind":
            continue
        for d in (c.depth0, c.depth1):
            assert (d == 0).any() and (d < 0).any() and np.isnan(d).any(), name
    for c, b, e in _all("borders"):
        holes = ~(c.depth0[b].reshape(-1) > 0)
        assert holes.any() and not e["valid0"][holes].any() and e["valid0"][~holes].all()  # a pixel centre reads its own pixel
    # no visible pixel: 0 / 0
    c, e = D.case("behind"), D.expected("behind")[0]
    assert e["counts"].tolist() == [0, 0, 0, 0] and np.isnan(e["valid_ratio"]) and e["valid_ratio"].dtype == F32
    i = 5 * 16 + 8
    assert e["valid0"].sum() == 1 and e["valid0"][i] and not e["visible0"][i]  # behind the camera: valid, in no image
    assert np.array_equal(e["proj_0to1"][i], [8.5, 5.5]) and e["matches0"][i] == -2
    # identity pose on one hole-free map
    c, e = D.case("step"), D.expected("step")[1]
    assert np.array_equal(c.depth0[1], c.depth1[1]) and (c.depth0[1] > 0).all() and np.array_equal(c.T01[1], np.eye(4))
    n = e["counts"][0]
    assert n > 100 and e["counts"].tolist() == [n] * 4 and e["valid_ratio"] == 1
    assert np.array_equal(e["matches0"][e["visible0"]], np.nonzero(e["visible0"])[0])
    # rotations by 90 and 180 degrees, different sizes and intrinsics per side
    assert np.array_equal(D.case("rot90").T01[0, :3, :3], D.RZ[90]) and np.array_equal(D.case("borders").T01[4, :3, :3], D.RZ[180])
    for name, b in (("rot90", 0), ("rot90", 1), ("borders", 4), ("scale", 0)):
        assert D.expected(name)[b]["counts"][0] > 20, name
    c = D.case("scale")
    assert c.size0 != c.size1 and c.K0[0, 0, 0] != c.K1[0, 0, 0] and D.case("rot90").size0 != D.case("rot90").size1


# ------------------------------------------------------------------------------------------------ (c) symbols
def _params(B=2, F0=2, F1=2, H0=12, W0=16, H1=10, W1=14, pos_sq=9.0, neg_sq=25.0):
    L = import_module(pkg.__name__ + "._lib")
    p = L.GtDenseParams()
    p.struct_size = ctypes.sizeof(L.GtDenseParams)
    p.B, p.F0, p.F1, p.H0, p.W0, p.H1, p.W1, p.pos_sq, p.neg_sq = B, F0, F1, H0, W0, H1, W1, pos_sq, neg_sq
    return p


def test_symbols_and_workspace_size():
    lib = pkg.native.lib()
    assert lib.einx_abi_version() == 6
    assert hasattr(lib, "einx_gt_dense") and hasattr(lib, "einx_gt_dense_ws_bytes")
    M = import_module(pkg.__name__ + ".core.metrics._native_metrics")
    G = import_module(pkg.__name__ + ".core.geometry.gt_generation")
    P = import_module(pkg.__name__ + ".datasets.pairs")
    assert callable(M.gt_matches_dense) and callable(G.gt_matches_dense_grid)
    assert callable(P.grid_keypoints) and callable(P.covisibility) and callable(P.select_pairs)
    ws = lambda **kw: lib.einx_gt_dense_ws_bytes(ctypes.byref(_params(**kw)))  # noqa: E731
    assert ws() > 0
    assert ws(B=0) == 0 and ws(H0=0) == 0 and lib.einx_gt_dense_ws_bytes(None) == 0
    assert ws(pos_sq=0.0) == 0 and ws(pos_sq=float("inf")) == 0 and ws(pos_sq=float("nan")) == 0
    p = _params()
    p.struct_size -= 4
    assert lib.einx_gt_dense_ws_bytes(ctypes.byref(p)) == 0
    # linear in the pixels of both sides (14 bytes a pixel, regions rounded to 256 bytes), nothing like N x M
    n = 260 * 346
    full = ws(B=1, F0=1, F1=1, H0=260, W0=346, H1=260, W1=346)
    assert 2 * 14 * n <= full <= 2 * 14 * n + 16 * 256
    assert ws(B=4, F0=1, F1=1, H0=260, W0=346, H1=260, W1=346) <= 4 * full
    assert abs(ws(B=1, F0=1, F1=1, H0=520, W0=346, H1=260, W1=346) - 1.5 * full) <= 16 * 256
    assert ws(B=1, F0=7, F1=9, H0=260, W0=346, H1=260, W1=346) == full  # frames cost nothing


def test_grid_keypoints_is_check_indices_grid():
    P = import_module(pkg.__name__ + ".datasets.pairs")
    H, W = 5, 7
    ref = torch.tensor([[y + 0.5, x + 0.5] for y in range(H) for x in range(W)])
    g = P.grid_keypoints(H, W)
    assert g.dtype == torch.float32 and torch.equal(g, ref) and torch.equal(P.grid_keypoints(H, W, "xy"), ref.flip(-1))
    assert g[2 * W + 3].tolist() == [2.5, 3.5]


# ------------------------------------------------------------------------------------------------ (d) select_pairs' bookkeeping
RATIOS = {(0, 1): 0.4, (0, 2): 0.41, (0, 3): 0.8, (0, 4): 0.79, (1, 2): float("nan"), (2, 1): 0.5, (3, 0): 0.1, (4, 2): 0.6, (5, 1): 0.95,
          (1, 5): 0.45}


def _fake_covisibility(calls):
    def fake(depth0, depth1, K0, K1, T_0to1, T_1to0=None, pos_th=3, neg_th=5, idx0=None, idx1=None):
        calls.append(len(idx0))
        assert depth0 is depth1 and K0.shape == (len(idx0), 3, 3) and T_0to1.shape == (len(idx0), 4, 4) and T_1to0.shape == T_0to1.shape
        r = torch.tensor([RATIOS[(int(a), int(b))] for a, b in zip(idx0, idx1)], dtype=torch.float32)
        counts = torch.stack([idx0, idx1, idx0 + idx1, idx0 * idx1], 1).to(torch.int32)
        return {"counts": counts, "valid_ratio": r}
    return fake


def test_select_pairs_bookkeeping(monkeypatch):
    P = import_module(pkg.__name__ + ".datasets.pairs")
    depth = torch.ones(6, 4, 5)
    poses = np.stack([np.eye(4)] * 6)
    poses[:, 0, 3] = np.arange(6)
    K = np.array([[4, 0, 2.5], [0, 4, 2], [0, 0, 1.0]])
    indices = [(0, 1), (0, 2), (3, 3), (0, 3), (0, 4), (1, 2), (2, 1), (2, 2), (3, 0), (4, 2), (5, 1), (1, 5)]
    results = []
    for batch in (1, 3, 4, 64):
        calls = []
        monkeypatch.setattr(P, "covisibility", _fake_covisibility(calls))
        r = P.select_pairs(depth, K, poses, indices, batch=batch, device="cpu")
        cand = [p for p in indices if p[0] != p[1]]  # equal indices are skipped, as in the reference
        assert r["candidates"].tolist() == [list(p) for p in cand]
        assert calls == [min(batch, len(cand) - s) for s in range(0, len(cand), batch)]  # one covisibility call a batch
        # strict bounds (0.4 and 0.8 themselves are out), NaN dropped, input order kept
        assert r["pairs"].tolist() == [[0, 2], [0, 4], [2, 1], [4, 2], [1, 5]]
        assert r["kept"].tolist() == [0.4 < RATIOS[p] < 0.8 for p in cand]
        assert np.array_equal(r["valid_ratio"], np.array([RATIOS[p] for p in cand], F32), equal_nan=True) and r["valid_ratio"].dtype == F32
        assert r["counts"].dtype == np.int32 and r["counts"][:, 2].tolist() == [a + b for a, b in cand]
        results.append(r)
    for r in results[1:]:  # batching does not change the result
        for k in results[0]:
            assert np.array_equal(r[k], results[0][k], equal_nan=True), k
    r = P.select_pairs(depth, K, poses, indices, ratio_range=(0.05, 0.45), device="cpu")
    assert r["pairs"].tolist() == [[0, 1], [0, 2], [3, 0]]
    with pytest.raises(IndexError):
        P.select_pairs(depth, K, poses, [(0, 6)], device="cpu")


def test_relative_transforms_are_the_rigid_closed_form():
    P = import_module(pkg.__name__ + ".datasets.pairs")
    poses = np.stack([D._pose(D._rot(0.1 * k, -0.2 * k, 0.3 * k), [k, 2 * k, -k]) for k in range(4)])
    pairs = np.array([(0, 1), (3, 1), (2, 0)])
    T01, T10 = P.relative_transforms(poses, pairs)
    assert T01.dtype == F32 and T10.dtype == F32
    for (a, b), x, y in zip(pairs, T01, T10):
        assert np.allclose(x, poses[b] @ np.linalg.inv(poses[a]), atol=1e-6) and np.allclose(y, poses[a] @ np.linalg.inv(poses[b]), atol=1e-6)


# ------------------------------------------------------------------------------------------------ (e) the reference's fixture
def test_restatement_equals_the_reference_fixture():
    """the reference's own gt_matches_from_pose_depth on check_indices' meshgrid (tests/golden/gen_gt_dense.py): every discrete
    output, the counts and valid_ratio equal the float64 restatement's exactly; the continuous ones within float32 noise"""
    G = Golden("gt_dense")
    assert set(G.cases) == set(D.FIXTURE_SIZES)
    for name, m in G.cases.items():
        c = D.random_scene(m["seed"], 1, tuple(m["size0"]), tuple(m["size1"]))
        e = D.dense_pair(c.depth0[0], c.depth1[0], c.K0[0], c.K1[0], c.T01[0], c.T10[0], m["pos_th"], m["neg_th"])
        for k in D.DISCRETE:
            assert np.array_equal(G[f"{name}.{k}"], e[k]), (name, k)
        assert G[f"{name}.valid_ratio"].dtype == F32 and G[f"{name}.valid_ratio"] == e["valid_ratio"]
        assert m["dtypes"]["matches0"] == "int64" and m["dtypes"]["matching_scores0"] == "float32" and m["dtypes"]["visible0"] == "bool"
        for k in ("matching_scores0", "matching_scores1"):
            assert np.array_equal(G[f"{name}.{k}"], e[k])
        for k in ("proj_0to1", "proj_1to0", "depth_keypoints0", "depth_keypoints1"):
            np.testing.assert_allclose(G[f"{name}.{k}"], e[k], rtol=0, atol=1e-4, equal_nan=True)
        assert e["counts"][0] > 50  # a scene with matches, not an empty agreement
