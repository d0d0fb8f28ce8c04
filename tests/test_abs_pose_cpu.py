"""CPU tests of the absolute pose: what tests/test_abs_pose_gpu.py relies on is established here on the float64
restatement tests/abs_pose_f64.py alone -- the ground-truth bound, that swapped cameras would be noticed, the P3P certificate,
the summation-order floor of the refit, the boundary seeds -- together with the metric class, the evaluator's keys on fake rows
and the C entry's refusals.  Each measuring test prints its figures; the constants in tests/abs_pose_cases.py are those prints."""
import ctypes
import types
from importlib import import_module

import numpy as np
import pytest
import torch

import abs_pose_cases as C
import abs_pose_f64 as A
from helpers import load_pkg

pkg = load_pkg()
_lib = import_module(pkg.__name__ + "._lib")
NM = import_module(pkg.__name__ + ".core.metrics._native_metrics")
MM = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
H = import_module(pkg.__name__ + ".harness")
absolute_pose, AbsolutePoseEstimation = NM.absolute_pose, import_module(pkg.__name__ + ".core.metrics").AbsolutePoseEstimation

OK = [i for i in range(len(C.PAIRS)) if i not in C.STATUS]


def test_statuses():
    for i in range(len(C.PAIRS)):
        assert C.ref(i)["status"] == C.STATUS.get(i, "ok"), i
    assert C.ref(15)["nu"] == 4 and C.ref(15)["rows"][4] == 0.1 and C.ref(14)["rows"][4] == 0.0
    assert np.isnan(C.ref(0)["rows"][4])  # no match: the usable ratio is 0 / 0
    for i in range(len(C.LIFT_PAIRS)):
        r = C.lift_ref(i)
        assert r["status"] == ("few" if C.LIFT_PAIRS[i] == "all_holes" else "ok")
        if r["status"] == "ok":
            assert 0.6 < r["rows"][4] < 0.95  # ~20 % holes make more than 20 % of the bilinear samples fall back or fail


def test_ground_truth_bound():
    """(a) R_err and t_err of the restatement on the cases with n >= 50, <= 50 % outliers, <= 0.5 px noise and exact depth"""
    worst = {"R_err": (0.0, None), "t_err": (0.0, None)}
    idx = [i for i in OK if C.gt_case(i)]
    assert len(idx) >= 6
    for i in idx:
        rows = C.ref(i)["rows"]
        for k, v in (("R_err", rows[0]), ("t_err", rows[1])):
            if v > worst[k][0]:
                worst[k] = (v, i)
    print("ground-truth worst", worst, "bound", C.GT_BOUND)
    for k in worst:
        assert worst[k][0] <= C.GT_BOUND[k], (k, worst[k])
        assert worst[k][0] <= 1.05 * C.GT_WORST[k], "GT_WORST is not what the restatement gives any more"


def test_swapped_cameras_are_noticed():
    """(b) with K0 and K1 swapped the restatement is far off on each ground-truth case"""
    for i in OK:
        if not C.gt_case(i):
            continue
        s = dict(C.pair(i))
        s["K0"], s["K1"] = s["K1"], s["K0"]
        r = C.run(s, **C.KW)
        off = r["status"] != "ok" or r["rows"][0] > 20 * C.GT_BOUND["R_err"] or r["rows"][1] > 20 * C.GT_BOUND["t_err"]
        print(i, r["status"], r["rows"][:2])
        assert off, i


def test_p3p_certificate():
    """(c) every pose of the 24 problems reprojects its three points; the true pose is among them"""
    X, f, R, t = C.p3p_problems()
    worst, counts = (0.0, None), []
    for k in range(len(X)):
        sols = A.p3p(X[k], f[k])
        assert 1 <= len(sols) <= 4
        counts.append(len(sols))
        for Rs, ts in sols:
            assert np.all((X[k] @ Rs.T + ts)[:, 2] > 0)
            res = C.p3p_residual(X[k], f[k], Rs, ts)
            if res > worst[0]:
                worst = (res, k)
        assert min(C.pose_distance(Rs, ts, R[k], t[k]) for Rs, ts in sols) < 1e-8, k
    print("P3P_WORST", worst, "solution counts", counts)
    assert worst[0] <= C.P3P_WORST <= 1.5 * worst[0] + 1e-15
    assert 10 * C.P3P_WORST < C.P3P_CEILING
    assert max(counts) == 4 and min(counts) == 1  # the problems cover one to four poses


def test_p3p_guards():
    X, f, _, _ = C.p3p_problems(2)
    line = np.stack([X[0][0], X[0][0] + (X[0][1] - X[0][0]) * 0.5, X[0][1]])
    assert A.p3p(line, f[0]) == []
    assert A.p3p(np.repeat(X[0][:1], 3, 0), f[0]) == []
    assert A.p3p(X[0], np.stack([f[0][0], f[0][0], f[0][2]])) == []


def test_frames_and_kabsch_agree():
    X, f, R, t = C.p3p_problems()
    for k in range(len(X)):
        Q = X[k] @ R[k].T + t[k]
        R1, t1 = A.frames_pose(X[k], Q)
        R2, t2 = A.kabsch_pose(X[k], Q)
        assert C.pose_distance(R1, t1, R[k], t[k]) < 1e-12 and C.pose_distance(R2, t2, R[k], t[k]) < 1e-12


def test_summation_order_floor():
    """(d) the refit with its LM sums taken over the reversed inlier list, and the restatement's distance from the true pose on
    the noise-free, outlier-free cases"""
    floor, clean = (0.0, None), (0.0, None)
    for i in OK:
        r = C.ref(i)
        rr = C.run(C.pair(i), reverse=True, **C.KW)
        assert rr["it"] == r["it"] and np.array_equal(rr["mask"], r["mask"])
        d = C.pose_distance(rr["R"], rr["t"], r["R"], r["t"])
        if d > floor[0]:
            floor = (d, i)
        if C.clean_case(i):
            T = C.pair(i)["T"]
            d = C.pose_distance(r["R"], r["t"], T[:3, :3], T[:3, 3])
            if d > clean[0]:
                clean = (d, i)
    print("REFIT_FLOOR", floor, "CLEAN_WORST", clean)
    assert floor[0] <= C.REFIT_FLOOR <= 1.5 * floor[0]
    assert clean[0] <= C.CLEAN_WORST <= 1.5 * clean[0]


def test_refit_improves_the_ransac_model():
    for i in OK:
        r, s = C.ref(i), C.pair(i)
        if r["nu"] < 6:
            continue
        idx, X = A.lift(s["kp0"][:, 1::-1], s["K0"], d0=s["d0"], valid0=s["valid0"])
        px = s["kp1"][idx][:, 1::-1].astype(np.float64)
        inl = r["mask"][idx]
        K1 = s["K1"].astype(np.float64)
        S0 = A._normal(r["R0"], r["t0"], X[inl], px[inl], K1)[2]
        S1 = A._normal(r["R"], r["t"], X[inl], px[inl], K1)[2]
        assert S1 <= S0, i


def test_boundary_seeds():
    assert sorted(C.BOUNDARY_SEEDS) == sorted(C.BOUNDARY_ITERS)
    for it, seed in C.BOUNDARY_SEEDS.items():
        r = C.boundary_ref(seed)
        assert r["status"] == "ok" and r["it"][0] == it, (it, seed, r.get("it"))


def test_draws_do_not_depend_on_anything_but_nu_iteration_seed():
    assert A.draw3(5, 7, 40) == A.draw3(5, 7, 40) and len(set(A.draw3(5, 7, 4))) == 3
    assert A.draw3(5, 7, 40) != A.draw3(6, 7, 40) or A.draw3(5, 8, 40) != A.draw3(5, 7, 40)


# ------------------------------------------------------------------ (e) the metric class and the evaluator's keys
ROWS = np.array([[1.0, 0.05, 2.0, 0.8, 1.0], [7.0, 0.05, 3.0, 0.5, 0.5], [4.0, 0.3, np.nan, 0.6, 0.75], [np.inf, np.inf, np.inf, 0.0, np.nan]])
THR = ((5, 0.1), (10, 0.5))
KEYS = ["APE_R_errs", "APE_t_errs", "APE_t_angles", "APE_inliers", "APE_usable", "APE@5deg_0.1_ratio", "APE@10deg_0.5_ratio"]


def test_metric_class_on_rows():
    m = AbsolutePoseEstimation("APE", THR)
    assert m.thresholds == ((5.0, 0.1), (10.0, 0.5)) and m.ransac_thresh == 8.0 and m.ransac_conf == 0.99 and m.ordering == "yx"
    out = AbsolutePoseEstimation.summary(ROWS, m.thresholds, "APE")
    assert list(out) == KEYS
    assert out["APE_R_errs"] == 4.0 and out["APE_t_errs"] == pytest.approx(0.4 / 3) and out["APE_t_angles"] == 2.5
    assert out["APE_inliers"] == pytest.approx(1.9 / 4) and out["APE_usable"] == 0.75
    assert out["APE@5deg_0.1_ratio"] == 0.25 and out["APE@10deg_0.5_ratio"] == 0.75  # the pair without a pose counts 0
    m.rows = list(ROWS)
    assert m.compute() == out
    assert all(np.isnan(v) for k, v in AbsolutePoseEstimation("X", ()).compute().items()) and H.ape_summary(ROWS, m.thresholds) == out
    with pytest.raises(AssertionError):
        AbsolutePoseEstimation("APE", THR, ordering="zz")
    assert NM.ABS_POSE_STATUS == {-1: "few", -2: "none"}


def test_evaluator_keys_on_fake_rows():
    mnn = types.SimpleNamespace(matcher=import_module(pkg.__name__ + ".core.modules.Matchers").Matcher(pkg.default_config("SP_MNN"), None, device="cpu"))
    ev = pkg.DifferentTimeEvaluator(mnn, 5, abs_pose_thresh=THR)
    metric = torch.from_numpy(np.arange(2 * len(ev.names), dtype=np.float64).reshape(2, -1) / 8.0)
    ev._metric_mean.add(metric)
    before = ev.result()
    assert list(before) == list(ev.names)  # no batch carried pose and depth: no new key
    ev._abs_pose_rows.append(torch.from_numpy(ROWS[:2]))
    ev._abs_pose_rows.append(torch.from_numpy(ROWS[2:]))
    res = ev.result()
    assert list(res) == list(ev.names) + KEYS
    assert {k: res[k] for k in KEYS} == AbsolutePoseEstimation.summary(ROWS, ev.abs_pose_thresh, "APE")
    assert (ev.abs_pose_ransac_thresh, ev.abs_pose_conf) == (8.0, 0.99)
    # the default evaluator has no such key whatever it holds, and its other keys are the same
    ev0 = pkg.DifferentTimeEvaluator(mnn, 5)
    assert ev0.abs_pose_thresh is None
    ev0._metric_mean.add(metric)
    ev0._abs_pose_rows.append(torch.from_numpy(ROWS))
    assert ev0.result() == before


# ------------------------------------------------------------------ (f) refusals
def _params(B=2, cap=64, cols=3, H_=40, W_=48, max_iters=100, size=None):
    p = _lib.AbsPoseParams()
    p.struct_size = ctypes.sizeof(_lib.AbsPoseParams) if size is None else size
    p.B, p.cap, p.cols, p.kp_yx, p.H, p.W, p.max_iters, p.refine = B, cap, cols, 1, H_, W_, max_iters, 1
    p.thresh, p.conf, p.seed = 8.0, 0.99, 1
    return p


BAD = {"struct_size_0": dict(size=0), "struct_size_short": dict(size=8), "cols_1": dict(cols=1), "cols_4": dict(cols=4), "B_0": dict(B=0),
       "cap_0": dict(cap=0), "max_iters_0": dict(max_iters=0), "max_iters_65536": dict(max_iters=65536)}


def test_workspace_query():
    L = pkg.native.lib()
    q = lambda p: L.einx_absolute_pose_ws_bytes(ctypes.byref(p))  # noqa: E731
    small, full = q(_params()), q(_params(32, 1024))
    assert small > 0 and small % 256 == 0 and full % 256 == 0
    assert full < 32 * (1024 * 64 + 100 * 4 * 12 * 8 * 2)  # points and models only
    for name, kw in BAD.items():
        assert q(_params(**kw)) == 0, name
    assert L.einx_absolute_pose_ws_bytes(None) == 0
    assert L.einx_abi_version() == 6  # additive symbols only


@pytest.mark.parametrize("name", list(BAD) + ["both_depth_forms", "no_depth", "d_without_valid", "depth_size_0"])
def test_refusals(name):
    """every refusal returns an error with a message before anything touches the device (the pointers are never read)"""
    L = pkg.native.lib()
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    p = _params(**BAD.get(name, {}))
    depth = {"both_depth_forms": [ptr, ptr, ptr], "no_depth": [None, None, None], "d_without_valid": [None, ptr, None]}.get(name, [ptr, None, None])
    if name == "depth_size_0":
        p.H = 0
    rc = L.einx_absolute_pose(ctypes.byref(p), ptr, ptr, ptr, *depth, ptr, ptr, None, ptr, ptr, ptr, ptr, ptr, None, None)
    assert rc != 0
    msg = L.einx_last_error().decode()
    assert msg.startswith("einx_absolute_pose: ") and len(msg) > len("einx_absolute_pose: "), msg


def test_python_refusals():
    mk = torch.zeros((1, 8, 3))
    n, K = torch.zeros(1, dtype=torch.int32), torch.eye(3)[None]
    d, v, dm = torch.ones((1, 8)), torch.ones((1, 8), dtype=torch.uint8), torch.ones((1, 4, 4))
    for kw in (dict(depth0=dm, d0=d, valid0=v), dict(), dict(d0=d), dict(depth0=dm, valid0=v)):
        with pytest.raises(ValueError, match="either as a map"):
            absolute_pose(mk, mk, n, K, K, **kw)
    with pytest.raises(ValueError, match="2 or 3 columns"):
        absolute_pose(mk[..., :1], mk[..., :1], n, K, K, depth0=dm)
