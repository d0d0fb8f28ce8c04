"""CPU tests of the pair metrics under depth + motion: the host-side parts of einx_pair_metrics_pose (size query,
refusals, the evaluator's arguments) and the float64 restatement tests/pose_metrics_f64.py against itself in float32 -- the
condition under which tests/test_pose_metrics_gpu.py may compare with array_equal -- and against metrics_f64.Restated under the
homography a fronto-parallel plane induces."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

import metrics_f64 as MF
import pose_metrics_f64 as F
from helpers import load_pkg

pkg = load_pkg()
_lib = import_module(pkg.__name__ + "._lib")
NM = import_module(pkg.__name__ + ".core.metrics._native_metrics")


def _params(B=3, cap0=70, cap1=90, D=36, cols=3, sizes=(48, 64, 40, 56), n=(2, 2, 2), size=None):
    p = _lib.PoseMetricParams()
    p.struct_size = ctypes.sizeof(_lib.PoseMetricParams) if size is None else size
    p.B, p.cap0, p.cap1, p.D, p.cols = B, cap0, cap1, D, cols
    p.H0, p.W0, p.H1, p.W1 = sizes
    p.n_mma, p.n_vdd, p.n_epi = n
    return p


BAD = {"struct_size": dict(size=8), "struct_size_of_einx_metric_params": dict(size=ctypes.sizeof(_lib.MetricParams)),
       "five_mma": dict(n=(5, 2, 2)), "five_vdd": dict(n=(2, 5, 2)), "five_epi": dict(n=(2, 2, 5)), "negative_count_of_thresholds": dict(n=(2, -1, 2)),
       "cols_1": dict(cols=1), "cols_4": dict(cols=4), "B_0": dict(B=0), "cap0_0": dict(cap0=0), "cap1_negative": dict(cap1=-1), "D_0": dict(D=0),
       "H0_0": dict(sizes=(0, 64, 40, 56)), "W1_negative": dict(sizes=(48, 64, 40, -56))}


def test_workspace_query():
    L = pkg.native.lib()
    q = lambda p: L.einx_pair_metrics_pose_ws_bytes(ctypes.byref(p))  # noqa: E731
    small, full = q(_params()), q(_params(32, 1024, 1024, 256))
    assert small > 0 and small % 256 == 0 and full % 256 == 0
    assert 0 < full < 2 * 32 * (1024 + 1024) * 64  # no N x M region
    assert q(_params(n=(0, 0, 0))) > 0 and q(_params(n=(4, 4, 4))) > 0
    for name, kw in BAD.items():
        assert q(_params(**kw)) == 0, name
    assert L.einx_pair_metrics_pose_ws_bytes(None) == 0
    assert L.einx_abi_version() == 6  # additive symbols only


@pytest.mark.parametrize("name", list(BAD) + ["one_depth_pointer_0", "one_depth_pointer_1", "depth_size_0"])
def test_refusals(name):
    """every refusal returns EINX_ERR_ARG with a message before anything touches the device (the pointers are never read)"""
    L = pkg.native.lib()
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    p = _params(**BAD.get(name, {}))
    depth = [None, None]
    if name.startswith("one_depth_pointer"):
        depth[int(name[-1])] = ptr
        p.dH0 = p.dW0 = p.dH1 = p.dW1 = 8
    if name == "depth_size_0":
        depth = [ptr, ptr]
        p.dH0, p.dW0, p.dH1, p.dW1 = 8, 8, 0, 8
    rc = L.einx_pair_metrics_pose(ctypes.byref(p), *[ptr] * 9, *depth, *[ptr] * 3, None, ptr, ptr, None)
    assert rc != 0
    msg = L.einx_last_error().decode()
    assert msg.startswith("einx_pair_metrics_pose: ") and len(msg) > len("einx_pair_metrics_pose: "), msg


def test_column_names():
    assert NM.pose_metric_names((1, 3), (2,), (0.5,)) == ["MR", "DT_MMA@1", "DT_MMA@3", "DT_judged_ratio", "DT_Repeatability@2",
                                                         "DT_ValidDistance@2", "DT_Angle@2", "EPI@0.5"]
    assert NM.pose_metric_names((), (), ()) == ["MR", "DT_judged_ratio"]


def _cases():
    return [F.build_case(name) for name in F.CASE_NAMES] + [F.two_layer_case()]


def _same(a, b, what):
    assert np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True), what


@pytest.mark.parametrize("name", F.CASE_NAMES + ["two_layer", "two_layer_off"])
def test_fp32_evaluation_is_exact(name):
    """float32 and float64 evaluations of the restatement agree bit for bit on every decision and every value the GPU test
    compares: projections of the points that count, masks, counts, neighbours, squared distances, squared reprojection errors"""
    c = F.two_layer_case() if name.startswith("two_layer") else F.build_case(name)
    occ = 0.0 if name == "two_layer_off" else "case"
    for b in range(c.B):
        R64, R32 = c.restate(b, np.float64, occ=occ), c.restate(b, np.float32, occ=occ)
        tag = (name, b)
        assert R32.warped0.dtype == np.float32 and R64.warped0.dtype == np.float64
        for k in ("ok0", "ok1", "valid0", "valid1", "keep0", "keep1", "judged"):
            assert np.array_equal(getattr(R32, k), getattr(R64, k)), (tag, k)
        assert (R32.N1, R32.N2) == (R64.N1, R64.N2)
        _same(R32.warped0[R64.ok0], R64.warped0[R64.ok0], (tag, "warped0"))
        _same(R32.match_proj[R64.judged], R64.match_proj[R64.judged], (tag, "match projections"))
        _same(R32.mma_sq[R64.judged], R64.mma_sq[R64.judged], (tag, "mma_sq"))
        for s in (0, 1):
            assert np.array_equal(R32.near_j[s], R64.near_j[s]), (tag, s)
            _same(R32.near_sq[s], R64.near_sq[s], (tag, s, "near_sq"))
        _same(R32.row(c.thr, c.thr, c.epi), R64.row(c.thr, c.thr, c.epi), (tag, "row"))


def test_cases_reach_what_they_are_for():
    """the planted structure is there: thresholds met exactly, ties, projections exactly on the image's bounds and a quarter pixel
    either side, holes under keypoints / under one tap of four / under matched rows, every special pair"""
    at = ties = 0
    for name in ("ragged", "trip_edge", "past_1024"):
        c = F.build_case(name)
        for b, R in enumerate(c.pairs):
            if min(c.n[b], c.m[b]) < 30:
                continue
            assert c.info[b]["edges"], (name, b)
            for k, axis, bound, off in c.info[b]["edges"]:
                assert R.valid0[k] and R.warped0[k, axis] == bound + off, (name, b, k)
                lim = c.size1[1 - axis]
                assert R.keep0[k] == (0 <= bound + off < lim), (name, b, k, "the bound is the image's, half-open")
            at += sum(int((R.near_sq[s] == t * t).sum()) for s in (0, 1) for t in c.thr)
            ties += sum(R.ties)
            assert (~R.valid0).any() and (~R.valid1).any() and (~R.judged).any() and R.judged.any(), (name, b, "holes")
            assert 0 < R.N1 < c.n[b] and 0 < R.N2 < c.m[b]
            assert any(((R.mma_sq == t * t) & R.judged).any() for t in c.thr), (name, b, "a reprojection error exactly on a threshold")
    assert at >= 8 and ties >= 4, (at, ties)
    # a hole under one tap of four whose nearest pixel is good: the keypoint stays valid through the fallback
    c = F.build_case("past_1024")
    xy = c.k0[0, :c.n[0]][:, [1, 0]].astype(np.float64)
    _, valid, info = F.sample_depth(xy, c.depth0[0])
    assert (info["fallback"] & valid).any() and (info["fallback"] & ~valid).any()
    u = F.build_case("unjudged")
    assert not u.pairs[0].judged.any() and u.nm[0] > 0 and np.isnan(u.row(0)[1]) and u.row(0)[1 + len(u.thr)] == 0.0
    assert u.pairs[1].N1 == 0 and u.pairs[1].N2 > 0 and np.isnan(u.row(1)[2 + len(u.thr):2 + 4 * len(u.thr)]).all() and u.row(1)[0] > 0
    assert (u.pairs[2].epi == 0).all() and (u.row(2)[-len(u.epi):] == 1.0).all()
    L = F.two_layer_case()
    on, off = L.pairs[0], L.pairs_off[0]
    assert off.keep0.all() and off.keep1.all() and off.judged.all()
    assert np.array_equal(on.keep0, ~L.hidden0) and np.array_equal(on.keep1, ~L.hidden1) and np.array_equal(on.judged, ~L.hidden_matches)
    assert 8 <= L.hidden0.sum() < L.n[0] // 2 and 6 <= L.hidden1.sum() < L.m[0] // 2 and 5 <= L.hidden_matches.sum() < L.nm[0]


def test_epipolar_margins():
    """every planted epipolar distance is farther than 1e-6 from every EPI threshold (row() asserts it)"""
    for c in _cases():
        for b, R in enumerate(c.pairs):
            R.row(c.thr, c.thr, c.epi)
            for t in c.epi:
                assert not len(R.epi) or np.abs(R.epi - t).min() > F.EPI_MARGIN, (c.name, b, t)


@pytest.mark.parametrize("geom", ["shift", "rot90", "rot180"])
def test_plane_equals_the_induced_homography(geom):
    """on a fronto-parallel plane without holes and with in-plane motion the pose form IS the homography form under
    H = [[R, s + c1 - R c0], [0, 0, 1]]: the same MMA@t, Repeatability@t, ValidDistance@t and Angle@t as metrics_f64.Restated,
    for the keypoints that lie inside their own depth map (outside it there is no depth, which a homography does not know)"""
    thr = (1, 2.5, 3, 5)
    k0, k1, d0, d1, mk0, mk1, _, _, _ = F.make_pair(777, 120, 130, 60, 36, 3, True, geom)
    own = lambda k, size: (k[:, 1] >= 0.5) & (k[:, 1] <= size[1] - 0.5) & (k[:, 0] >= 0.5) & (k[:, 0] <= size[0] - 0.5)  # noqa: E731
    s0, s1 = own(k0, F.SIZE0), own(k1, F.SIZE1)
    k0, d0, k1, d1 = k0[s0], d0[s0], k1[s1], d1[s1]
    g = F.GEOMETRIES[geom]
    plane0, plane1 = np.full(F.SIZE0, F.PLANE, np.float32), np.full(F.SIZE1, F.PLANE, np.float32)
    P = F.RestatedPose(k0, k1, d0, d1, mk0, mk1, F.SIZE0, F.SIZE1, g.K0, g.K1, g.T01, None, plane0, plane1)
    Hm = MF.Restated(k0, k1, d0, d1, mk0, mk1, F.SIZE0, F.SIZE1, F.induced_homography(geom))
    assert P.judged.all() and 0 < P.N1 < len(k0) and 0 < P.N2 <= len(k1)
    assert np.array_equal(P.warped0, Hm.warped0) and np.array_equal(P.keep0, Hm.keep0) and np.array_equal(P.keep1, Hm.keep1)
    got, exp = P.row(thr, thr, ()), Hm.row(thr, thr)
    assert got[1 + len(thr)] == 1.0  # judged_ratio
    assert np.array_equal(np.delete(got, 1 + len(thr)), exp, equal_nan=True)
    assert 0 < exp[1] < exp[4] < 1


def test_evaluator_arguments():
    """host logic only: the constructor refuses before it looks at the model"""
    E = pkg.DifferentTimeEvaluator
    with pytest.raises(ValueError, match="occlusion_th needs reproj_thr"):
        E(None, 5, occlusion_th=1.0)
    with pytest.raises(ValueError, match="occlusion_th needs reproj_thr"):
        E(None, 5, epi_thr=(1, 3), occlusion_th=1.0)
    with pytest.raises(ValueError, match="reproj_thr takes 1 to 4"):
        E(None, 5, reproj_thr=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="epi_thr takes 1 to 4"):
        E(None, 5, epi_thr=())
    with pytest.raises(ValueError, match="both depth maps or neither"):
        NM.pair_metrics_pose.__wrapped__(*[None] * 11, None, None, None, depth0=object())
