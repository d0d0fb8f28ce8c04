"""GPU tests (-m gpu), component: core.geometry.depth / .epipolar on the device (csrc/geometry.hip) against the dense
restatement tests/geometry_f64.py on inputs that fp32 evaluates exactly (test_geometry_cpu.py asserts that, and what each case
plants).  Every comparison of a projection, a depth, a sample or a flag is array_equal; the epipolar distances, whose root and
quotients round, are held to a relative 2^-21 against float64 (geometry_f64.EPI_GATE) and, in general position, to the bound the
fixture recorded from the reference's own float32 noise."""
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import geometry_f64 as F
from gpu_support import DEV, _np, _t, pkg
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
G = F.G
M = import_module(pkg.__name__ + ".core.metrics._native_metrics")
depth = import_module(pkg.__name__ + ".core.geometry.depth")
epipolar = import_module(pkg.__name__ + ".core.geometry.epipolar")
wrappers = import_module(pkg.__name__ + ".core.geometry.wrappers")
pairs = import_module(pkg.__name__ + ".datasets.pairs")
LAYOUTS = (("yx", 3), ("xy", 2))
BOUNDS = (None, F.BOUND_EQ, F.BOUND_ABOVE)


def _i32(v):
    return torch.tensor([int(x) for x in v], dtype=torch.int32, device=DEV)


def _f(a):
    return _t(np.asarray(a, np.float32))


def _equal(got, exp, tag):
    got = _np(got)
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    assert np.array_equal(got.astype(exp.dtype), exp, equal_nan=True), tag
    return got


# ------------------------------------------------------------------------------------------------ sparse project
def _both_sides(c, ordering, cols, T10, pre, ccth, fill, cap):
    """both directions in one launch, as gt_matches_cc issues it"""
    kp0, kp1 = _t(G.pad_rows(c.kp0, cap, fill, ordering, cols)), _t(G.pad_rows(c.kp1, cap, fill, ordering, cols))
    n, m = _i32(c.n), _i32(c.m)
    K0, K1, T01 = _t(c.K0), _t(c.K1), _t(c.T01)
    T10 = None if T10 is None else _t(T10)
    kw0, kw1 = dict(depth=_t(c.depth0)), dict(depth=_t(c.depth1))
    if pre:
        kw0 = dict(d=_t(G.pad_values([p[0] for p in c.pre], cap, fill)), valid=_t(G.pad_flags([p[1] for p in c.pre], cap, True)))
        kw1 = dict(d=_t(G.pad_values([p[2] for p in c.pre], cap, fill)), valid=_t(G.pad_flags([p[3] for p in c.pre], cap, True)))
    s0 = M._geom_side(c.B, torch.device(DEV), kp0, n, K0, K1, T01, T10, depth_other=_t(c.depth1), **kw0)
    s1 = M._geom_side(c.B, torch.device(DEV), kp1, m, K1, K0, T10, T01, depth_other=_t(c.depth0), **kw1)
    M._geom_project_sides([s0, s1], ccth, ordering)
    return {"proj_0to1": s0["proj"], "proj_1to0": s1["proj"], "depth_keypoints0": s0["d_out"], "depth_keypoints1": s1["d_out"],
            "valid0": s0["valid_out"].bool(), "valid1": s1["valid_out"].bool(), "visible0": s0["visible"].bool(), "visible1": s1["visible"].bool()}


@pytest.mark.parametrize("n", F.PROJECT_N)
def test_project(n):
    """block edges (1, 255, 256, 257 keypoints of capacity n + 3), both orderings, 2 and 3 columns, T_1to0 given and inverted in the
    kernel, depth maps and given depths, no cycle check / the bound ON the hidden points' distance / one lattice step above it;
    rows past the counts are zeros whatever they hold"""
    c = F.occlusion_scene(n)
    cap = n + 3
    for ccth in BOUNDS:
        for given in (True, False):
            for pre in (False, True):
                exp = G.padded_expected(F.occlusion_expected(n, ccth, given, pre), cap, cap, G.STAGE_A_KEYS)
                first = None
                for (ordering, cols), fill in zip(LAYOUTS, (np.nan, 7.0)):
                    got = _both_sides(c, ordering, cols, c.T10 if given else None, pre, ccth, fill, cap)
                    out = {k: _equal(got[k], exp[k], (n, ccth, given, pre, ordering, k)) for k in G.STAGE_A_KEYS}
                    first = first or out
                    assert all(first[k].tobytes() == out[k].tobytes() for k in out)
    # the strict bound decides: some point is invisible AT the bound and visible a lattice step above it
    if n > 1:
        eq, above = (G.padded_expected(F.occlusion_expected(n, t, True, False), cap, cap, ("visible0", "visible1")) for t in BOUNDS[1:])
        assert all((above[k] & ~eq[k]).any() for k in eq)


def test_project_one_direction_and_the_drop_in():
    """geom_project (one direction per launch) and core.geometry.depth.project give the both-sides launch's bits; a sampler of the
    caller's goes through two launches with the same result"""
    n = 257
    c = F.occlusion_scene(n)
    cam0, cam1 = wrappers.Camera(_t(c.K0)), wrappers.Camera(_t(c.K1))
    T01 = wrappers.Pose.from_4x4mat(_t(c.T01))
    calls = []

    def my_sampler(pts, dm, scale=1.0):
        calls.append(scale)
        return depth.sample_depth(pts, dm)
    for ccth in BOUNDS:
        exp = G.padded_expected(F.occlusion_expected(n, ccth, True, True), n, n, G.STAGE_A_KEYS)
        kp0 = _t(G.pad_rows(c.kp0, n, 7.0, "xy", 2))
        d0, v0 = _t(G.pad_values([p[0] for p in c.pre], n, 2.0)), _t(G.pad_flags([p[1] for p in c.pre], n, True))
        r = M.geom_project(kp0, _t(c.K0), _t(c.K1), _t(c.T01), d=d0, valid=v0, depth_j=_t(c.depth1), count=_i32(c.n), cc_bound=ccth)
        _equal(r["proj"], exp["proj_0to1"], ccth)
        _equal(r["visible"], exp["visible0"], ccth)
        # the drop-in has no counts: compare each pair's own rows
        uv, vis = depth.project(kp0, d0, _t(c.depth1), cam0, cam1, T01, v0, ccth=ccth)
        uv2, vis2 = depth.project(kp0, d0, _t(c.depth1), cam0, cam1, T01, v0, ccth=ccth, sample_depth_fun=my_sampler, sample_depth_kwargs={"scale": 2.0})
        assert vis.dtype == torch.bool and uv.shape == (c.B, n, 2)
        for b in range(c.B):
            for u, v in ((uv, vis), (uv2, vis2)):
                _equal(u[b, :c.n[b]], exp["proj_0to1"][b, :c.n[b]], (ccth, b))
                _equal(v[b, :c.n[b]], exp["visible0"][b, :c.n[b]], (ccth, b))
    assert calls == [2.0, 2.0]  # not called without a bound
    uv, vis = depth.project(kp0, d0, None, cam0, cam1, T01, v0, ccth=F.BOUND_EQ)  # no depthj: no check, as in the reference
    _equal(vis[0, :c.n[0]], F.occlusion_expected(n, None, True, True)[0]["visible0"], "depthj None")


# ------------------------------------------------------------------------------------------------ dense warp
@pytest.mark.parametrize("name", list(F.DENSE_SHAPES))
def test_dense_warp(name):
    c = F.dense_case(name)
    (Hi, Wi), (Hj, Wj) = c.size_i, c.size_j
    cam_i, cam_j = wrappers.Camera(_t(c.K_i)), wrappers.Camera(_t(c.K_j))
    T = wrappers.Pose.from_4x4mat(_t(c.T))
    Tinv = np.stack([F.invert_pose(t) for t in c.T]).astype(np.float32)
    for ccth in BOUNDS:
        exp = [F.dense_warp(c.depth_i[b], c.depth_j[b], c.K_i[b], c.K_j[b], c.T[b], ccth) for b in range(c.B)]
        back = [F.dense_warp(c.depth_j[b], c.depth_i[b], c.K_j[b], c.K_i[b], Tinv[b], ccth) for b in range(c.B)]
        first = None
        for run in range(2):
            r = M.geom_dense_warp(_t(c.depth_i), _t(c.depth_j), _t(c.K_i), _t(c.K_j), _t(c.T), cc_bound=ccth)
            two = M.geom_dense_warp(_t(c.depth_i), _t(c.depth_j), _t(c.K_i), _t(c.K_j), _t(c.T), None, cc_bound=ccth, both=True)
            warp, vis, counts = _np(r["warp"]), _np(r["visible"]), _np(r["counts"])
            assert warp.shape == (c.B, Hi, Wi, 2) and vis.shape == (c.B, Hi, Wi) and vis.dtype == bool and counts.dtype == np.int32
            for b in range(c.B):
                valid = c.depth_i[b] > 0
                assert np.array_equal(warp[b][valid].astype(np.float64), exp[b][0][valid], equal_nan=True), (name, ccth, b)
                assert np.array_equal(np.isnan(warp[b]), np.isnan(exp[b][0])), (name, ccth, b)  # a NaN depth: a NaN warp
                assert np.array_equal(vis[b].reshape(-1), exp[b][1]), (name, ccth, b)
                assert tuple(counts[b]) == exp[b][2] == (int(valid.sum()), int(vis[b].sum())), (name, ccth, b)
                # the other direction on the same launch: the inverse taken in the kernel
                v1 = c.depth_j[b] > 0
                assert np.array_equal(_np(two["warp1"])[b][v1].astype(np.float64), back[b][0][v1], equal_nan=True), (name, ccth, b)
                assert np.array_equal(_np(two["visible1"])[b].reshape(-1), back[b][1]), (name, ccth, b)
                assert _np(two["counts"])[b].tolist() == [list(exp[b][2]), list(back[b][2])]
            assert torch.equal(two["warp"].view(torch.int32), r["warp"].view(torch.int32)) and torch.equal(two["visible"], r["visible"])
            bits = warp.tobytes() + vis.tobytes() + counts.tobytes()
            first = first or bits
            assert bits == first
        # the drop-in: the visibility takes depthj's shape
        kw = {} if ccth is None else {"ccth": ccth}
        w, v = depth.dense_warp_consistency(_t(c.depth_i), _t(c.depth_j), T, cam_i, cam_j, **kw)
        assert w.shape == (c.B, Hi, Wi, 2) and v.shape == (c.B, Hj, Wj) and v.dtype == torch.bool
        assert torch.equal(w.view(torch.int32), r["warp"].view(torch.int32)) and torch.equal(v.reshape(c.B, -1), r["visible"].reshape(c.B, -1))
        # overlap of both directions from the counts of one launch
        ov = _np(pairs.pair_overlap(_t(c.depth_i), _t(c.depth_j), _t(c.K_i), _t(c.K_j), _t(c.T), cc_th=ccth))
        want = np.array([[np.float32(e[2][1]) / np.float32(e[2][0]), np.float32(k[2][1]) / np.float32(k[2][0])] for e, k in zip(exp, back)])
        assert ov.dtype == np.float32 and np.array_equal(ov, want), (name, ccth)
    empty = _np(pairs.pair_overlap(torch.zeros(1, 4, 4, device=DEV), torch.ones(1, 4, 4, device=DEV), _t(c.K_i[:1]), _t(c.K_j[:1]), _t(c.T[:1])))
    assert np.isnan(empty[0, 0])  # 0 / 0


# ------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("C", [1, 3, 5])
def test_sample_fmap(C):
    fm, pts = F.sample_case(C)
    exp = np.stack([F.sample_fmap(pts[b], fm[b]) for b in range(2)])
    first = None
    for _ in range(2):
        got = _equal(depth.sample_fmap(_t(pts), _t(fm)), exp, C)
        first = first if first is not None else got
        assert got.tobytes() == first.tobytes()
    if C == 1:
        d, valid = depth.sample_depth(_t(pts), _t(fm[:, 0]))
        for b in range(2):
            e, ev = F.sample_depth(pts[b], fm[b, 0])
            _equal(d[b], e, b)
            _equal(valid[b], ev, b)


def test_sample_depth_equals_stage_a():
    """sample_depth gives the bits of einx_gt_project's depth_keypoints* and valid* on the same inputs (the sampler case of 8e:
    borders, corners, points outside, far / infinite / NaN coordinates, holes under one tap and under a weighted tap)"""
    c = G.sampler_case()
    cap0, cap1 = c.cap0, c.cap1
    kp0, kp1 = _t(G.pad_rows(c.kp0, cap0, 3.5, "xy", 2)), _t(G.pad_rows(c.kp1, cap1, 3.5, "xy", 2))
    a = M.gt_project(kp0, kp1, None, None, _t(c.depth0), _t(c.depth1), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10), ordering="xy")
    for kp, dm, side in ((kp0, c.depth0, 0), (kp1, c.depth1, 1)):
        d, valid = depth.sample_depth(kp, _t(dm))
        assert torch.equal(d.view(torch.int32), a[f"depth_keypoints{side}"].view(torch.int32)) and torch.equal(valid, a[f"valid{side}"])


# ------------------------------------------------------------------------------------------------ labels
LABEL_KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1", "pos0")


def test_gt_matches_cc():
    """gt_matches_cc = the cycle-checked stage A + the unchanged stage B: key by key what gt_label gives on the restatement's
    projections and flags; the visibility differs from gt_matches' (test_geometry_eval_gpu.py follows it into the labels); and on a scene without
    occluders and holes they are gt_matches'"""
    n = 257
    c = F.occlusion_scene(n)
    kp0, kp1 = _t(G.pad_rows(c.kp0, n, np.nan, "yx", 3)), _t(G.pad_rows(c.kp1, n, np.nan, "yx", 3))
    cnt_n, cnt_m = _i32(c.n), _i32(c.m)
    args = (_t(c.depth0), _t(c.depth1), _t(c.K0), _t(c.K1), _t(c.T01))
    plain = M.gt_matches(kp0, kp1, cnt_n, cnt_m, *args, pos_th=3, neg_th=5, ordering="yx")
    for ccth in BOUNDS:
        for T10 in (None, _t(c.T10)):
            e = G.padded_expected(F.occlusion_expected(n, ccth, T10 is not None, False), n, n, G.STAGE_A_KEYS)
            want = M.gt_label(kp0, kp1, cnt_n, cnt_m, _f(e["proj_0to1"]), _f(e["proj_1to0"]), _t(e["visible0"]), _t(e["visible1"]), _t(e["valid0"]),
                              _t(e["valid1"]), pos_th=3, neg_th=5, ordering="yx")
            got = M.gt_matches_cc(kp0, kp1, cnt_n, cnt_m, *args, T10, cc_th=ccth, pos_th=3, neg_th=5, ordering="yx")
            again = M.gt_matches_cc(kp0, kp1, cnt_n, cnt_m, *args, T10, cc_th=ccth, pos_th=3, neg_th=5, ordering="yx")
            assert set(got) == set(plain)
            for k in G.STAGE_A_KEYS:
                _equal(got[k], e[k], (ccth, k))
            for k in LABEL_KEYS:
                assert torch.equal(got[k], want[k]), (ccth, k)
            for k in got:
                assert _np(got[k]).tobytes() == _np(again[k]).tobytes(), (ccth, k)
            if ccth is None:
                for k in plain:
                    assert _np(got[k]).tobytes() == _np(plain[k]).tobytes(), k
            else:
                assert not torch.equal(got["visible0"], plain["visible0"]) and not torch.equal(got["visible1"], plain["visible1"])
    # no occluder, no hole: the plane at depth 2 in both views.  Everything gt_matches calls visible stays visible, except within
    # half a pixel of the other map's border: there the sampler's zero padding mixes a 0 into the depth (the reference's
    # grid_sample does the same), and the point comes back elsewhere
    flat0, flat1 = torch.full_like(args[0], F.FAR), torch.full_like(args[1], F.FAR)
    a = M.gt_matches(kp0, kp1, cnt_n, cnt_m, flat0, flat1, *args[2:], pos_th=3, neg_th=5, ordering="yx")
    b = M.gt_matches_cc(kp0, kp1, cnt_n, cnt_m, flat0, flat1, *args[2:], cc_th=1.0, pos_th=3, neg_th=5, ordering="yx")
    band = {k: ((a[p] < 0.5) | (a[p] > F.SIZE - 0.5)).any(-1) for k, p in (("visible0", "proj_0to1"), ("visible1", "proj_1to0"))}
    assert a["visible0"].any() and a["visible1"].any()
    for k in a:
        if k in band:
            assert torch.equal(b[k], a[k] & ~band[k]), k
        elif k in G.STAGE_A_KEYS or not (band["visible0"] & a["visible0"]).any() and not (band["visible1"] & a["visible1"]).any():
            assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k


# ------------------------------------------------------------------------------------------------ capture and replay
def test_graph_capture_and_replay():
    """every entry captured once on a side stream and replayed twice: the results of each replay are those of the eager calls"""
    c = F.occlusion_scene(257)
    dc = F.dense_case("33x45")
    fm, pts = F.sample_case(3)
    p0, p1, E = F.epipolar_case(257, 260)
    kp0, kp1 = _t(G.pad_rows(c.kp0, 257, np.nan, "yx", 3)), _t(G.pad_rows(c.kp1, 257, np.nan, "yx", 3))
    t = [_i32(c.n), _i32(c.m), _t(c.depth0), _t(c.depth1), _t(c.K0), _t(c.K1), _t(c.T01)]
    dt = [_t(dc.depth_i), _t(dc.depth_j), _t(dc.K_i), _t(dc.K_j), _t(dc.T)]
    st = [_t(pts), _t(fm)]
    et = [_t(p0), _t(p1), _t(E)]

    def run():
        a = M.gt_matches_cc(kp0, kp1, *t, cc_th=F.BOUND_EQ, ordering="yx")
        d = M.geom_dense_warp(*dt, cc_bound=F.BOUND_EQ, both=True)
        return {**{f"cc.{k}": v for k, v in a.items()}, **{f"dense.{k}": v for k, v in d.items()}, "sample": M.geom_sample(*st),
                "epi": M.epipolar_all(*et)}
    eager = {k: _np(v).tobytes() for k, v in run().items()}
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        for v in out.values():
            v.fill_(1) if v.dtype == torch.bool else v.fill_(85)
        graph.replay()
        torch.cuda.synchronize()
        for k, v in out.items():
            assert _np(v).tobytes() == eager[k], k


# ------------------------------------------------------------------------------------------------ epipolar distances
def _relative(got, exp):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(exp == 0, np.abs(got), np.abs(got - exp) / np.abs(exp))))


@pytest.mark.parametrize("n,m", F.EPI_SHAPES)
def test_epipolar_all(n, m):
    """exact inputs (dyadic F, lattice points): p1^T F p0 and the squared norms are exact, what rounds is a root and a quotient per
    term and the sum: gated at a relative 2^-21 against float64, twice the four roundings of 2^-24.
    Measured on an MI355X: see DESIGN.md 8t."""
    worst = 0.0
    for cols in ((2, 2), (3, 2), (2, 3), (3, 3)):
        p0, p1, E = F.epipolar_case(n, m, cols)
        exp = np.stack([F.epipolar_all(p0[b], p1[b], E[b]) for b in range(2)])
        first = None
        for _ in range(2):
            got = _np(epipolar.sym_epipolar_distance_all(_t(p0), _t(p1), _t(E)))
            first = first if first is not None else got
            assert got.tobytes() == first.tobytes()
        assert got.shape == (2, n, m) and got.dtype == np.float32 and np.isfinite(got).all()
        worst = max(worst, _relative(got.astype(np.float64), exp))
    print(f"epipolar_all {n}x{m}: worst relative deviation from float64 {worst:.3e} = {worst * 2 ** 24:.2f} x 2^-24 (gate {F.EPI_GATE:.3e})")
    assert worst <= F.EPI_GATE
    # leading dimensions, as the reference's einsum takes them: none, and two
    p0, p1, E = F.epipolar_case(n, m)
    base = _np(epipolar.sym_epipolar_distance_all(_t(p0), _t(p1), _t(E)))
    one = _np(epipolar.sym_epipolar_distance_all(_t(p0[0]), _t(p1[0]), _t(E[0])))
    two = _np(epipolar.sym_epipolar_distance_all(_t(p0)[None], _t(p1)[None], _t(E)[None]))
    assert one.shape == (n, m) and two.shape == (1, 2, n, m) and one.tobytes() == base[0].tobytes() and two.tobytes() == base.tobytes()


def test_epipolar_general_position_and_pairs():
    meta = json.loads(bytes(np.load(os.path.join(GOLDEN, "geometry.npz"))["meta"]).decode())["epi_general"]
    p0, p1, Fm = F.general_epipolar_case()
    exp = F.epipolar_all(p0[0], p1[0], Fm[0])
    got = _np(epipolar.sym_epipolar_distance_all(_t(p0), _t(p1), _t(Fm)))[0].astype(np.float64)
    err = float(np.abs(got - exp).max())
    print(f"epipolar_all, general position: max |kernel - float64| {err:.3e} px (the reference's own float32: {meta['floor']:.3e}, bound {meta['bound']:.3e})")
    assert err <= meta["bound"]
    # the paired distance is plain torch on the device: the same gate on the exact inputs
    p0, p1, E = F.epipolar_case(260, 260, cols=(2, 3))
    for sq in (True, False):
        got = _np(epipolar.sym_epipolar_distance(_t(p0), _t(p1), _t(E), squared=sq)).astype(np.float64)
        exp = np.stack([F.epipolar_pairs(p0[b], p1[b], E[b], sq) for b in range(2)])
        assert _relative(got, exp) <= F.EPI_GATE, sq
    cam = wrappers.Camera(_t(np.stack([F._kmat(32, 16, 16)] * 2).astype(np.float32)))
    T = wrappers.Pose.from_4x4mat(_t(np.stack([F._pose(F.RZ[90], F.T_XY)] * 2).astype(np.float32)))
    k0, k1 = _t(p0), _t(p1[..., :2].copy())
    d = epipolar.generalized_epi_dist(k0, k1, cam, cam, T, all=True, essential=False)
    assert d.shape == (2, 260, 260) and torch.isfinite(d).all()
    assert epipolar.generalized_epi_dist(k0, k1, cam, cam, T, all=False, essential=True).shape == (2, 260)
