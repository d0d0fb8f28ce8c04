"""CPU tests of the relative-pose refinement: what tests/test_pose_refine_gpu.py relies on is established here on
the float64 restatement tests/pose_refine_f64.py alone -- the analytic Jacobian, the summation-order floor, the distance from the
truth on clean data, the margins that make the device's selections comparable, the improvement on noisy data -- together with
the C entry's and the Python layer's refusals.  Each measuring test prints its figures; the constants in
tests/pose_refine_cases.py are those prints."""
import ctypes
import inspect
import types
from importlib import import_module

import numpy as np
import pytest
import torch

import pose_f64 as P
import pose_refine_cases as C
import pose_refine_f64 as RF
from helpers import load_pkg

pkg = load_pkg()
_lib = import_module(pkg.__name__ + "._lib")
NM = import_module(pkg.__name__ + ".core.metrics._native_metrics")
MM = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
H = import_module(pkg.__name__ + ".harness")


def _points(name):
    s = C.scene(name)
    return P.normalize(s["kp0"][:, 1::-1], s["K0"]), P.normalize(s["kp1"][:, 1::-1], s["K1"])


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["n64_clean", "n64_cams", "forward", "ransac_255"])
def test_jacobian_against_central_differences(name):
    """the analytic Jacobian over (w, a, b) against central differences of the residuals through apply_step"""
    x1, x2 = _points(name)
    R, t, _, _ = C.initial(name)
    r0, J = RF.jacobian(R, t, x1, x2)
    assert np.allclose(r0, RF.residuals(R, t, x1, x2), rtol=0, atol=1e-15)
    h, worst = 1e-6, 0.0
    for k in range(5):
        d = np.zeros(5)
        d[k] = h
        num = (RF.residuals(*RF.apply_step(R, t, d), x1, x2) - RF.residuals(*RF.apply_step(R, t, -d), x1, x2)) / (2 * h)
        worst = max(worst, float(np.abs(num - J[:, k]).max() / max(1.0, np.abs(J[:, k]).max())))
    print("jacobian", name, worst)
    assert worst < 1e-8  # central differences at h = 1e-6: h^2 truncation and 1e-16 / h rounding


def test_step_stays_on_the_manifold():
    R, t, _, _ = C.initial("n64_cams")
    Rn, tn = RF.apply_step(R, t, np.array([0.01, -0.02, 0.03, 0.05, -0.04]))
    assert np.abs(Rn @ Rn.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.norm(tn) - 1) < 1e-15
    b1, b2 = RF.basis(np.array([0.5, 0.5, np.sqrt(0.5)]))  # a tie of |t_0| and |t_1|: the first one
    assert b1[0] == 0.0 and abs(b1 @ b2) < 1e-16
    assert np.array_equal(RF.rot_step(np.zeros(3), R), R)


def test_summation_order_floor_and_clean_worst():
    """REFINE_FLOOR: the largest change of an entry of R or t with the sums taken in reverse, over the cases and the campaign;
    CLEAN_WORST: the restatement's own distance from the true pose on the noise-free, outlier-free cases"""
    floor, clean = (0.0, None), (0.0, None)
    for name in C.CASES:
        r, rr = C.ref(name), C.run(name, reverse=True)
        assert rr["info"][:2] == r["info"][:2] and rr["info"][3] == r["info"][3] and np.array_equal(rr["mask"], r["mask"]), name
        d = C.pose_distance(rr["R"], rr["t"], r["R"], r["t"])
        if d > floor[0]:
            floor = (d, name)
        if C.clean_case(name):
            assert r["info"][0] == 1, name
            d = C.pose_distance(r["R"], r["t"], *C.truth(name))
            if d > clean[0]:
                clean = (d, name)
    flips = 0
    for seed in C.FLOOR_CAMPAIGN:  # the accept flip at convergence: see REFINE_FLOOR
        d, acc, acc_rev = C.campaign_floor(seed)
        flips += acc != acc_rev
        if d > floor[0]:
            floor = (d, seed)
    print("REFINE_FLOOR", floor, "pairs of the campaign whose accepted-step count flipped", flips, "CLEAN_WORST", clean)
    assert floor[0] <= C.REFINE_FLOOR <= 1.5 * floor[0]
    assert clean[0] <= C.CLEAN_WORST <= 1.5 * clean[0]


@pytest.mark.parametrize("name", list(C.CASES))
def test_preconditions_of_the_gpu_comparison(name):
    """at every selection point (c_in, each S_r, c_ref, the final mask) no match has a float64 Sampson value within a relative
    1e-6 of the threshold, and no cheirality quantity lies within 1e-9 of zero: the device cannot select differently"""
    trace = []
    C.run(name, trace=trace)
    assert trace[0][1] == "c_in" and trace[-1][1] in ("c_ref", "mask")
    for kind, tag, val, aux in trace:
        if kind == "sampson":
            with np.errstate(invalid="ignore"):
                rel = np.abs(val - aux) / aux
            assert not np.any(rel <= 1e-6), (name, tag, float(np.nanmin(rel)))
        else:
            assert len(val) == 0 or float(np.abs(val).min()) > 1e-9, (name, tag)


def test_special_cases_are_what_they_are_named():
    assert C.ref("n5")["info"] == (0, 0, 0, 0) and C.ref("n5")["c_in"] < 6
    assert C.ref("few_inliers")["info"] == (0, 0, 0, 0) and C.ref("few_inliers")["c_in"] < 6
    r = C.ref("rejected")
    assert r["info"][0] == 0 and r["info"][2] > 0 and r["c_ref"] < r["c_in"]  # steps were accepted, the keep rule said no
    R, t, mask, _ = C.initial("rejected")
    assert np.array_equal(r["R"], R) and np.array_equal(r["t"], t) and np.array_equal(r["mask"], mask)
    neg = C.run(C.NEGATIVE, status=-2)
    assert neg["info"] == (-1, 0, 0, 0) and not neg["R"].any() and neg["rows"] == (np.inf, np.inf, np.inf, 0.0)
    assert C.ref("rounds4")["info"][1] == 4 and C.ref("rounds1")["info"][1] == 1
    assert np.isnan(C.run("n64_clean", with_T=False)["rows"][:3]).all()
    for name in C.DEGENERATE:
        r = C.ref(name)
        assert np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all(), name
    not_kept = {n for n in C.CASES if C.ref(n)["info"][0] == 0}
    print("NOT_KEPT", sorted(not_kept), "of", len(C.CASES))
    assert not_kept == C.NOT_KEPT and all(C.ref(n)["info"][0] == 1 for n in C.CASES if n not in not_kept)
    for name in C.CASES:  # the keep rule: the mask of a kept refinement is no smaller than the input pose's inlier set can make it
        r = C.ref(name)
        assert r["info"][0] == 0 or r["c_ref"] >= r["c_in"], name


def test_refinement_improves_the_noisy_cases():
    names = [n for n in C.CASES if C.noisy_case(n)]
    assert len(names) >= 10
    before = np.array([C.pose_err_before(n) for n in names])
    after = np.array([C.ref(n)["rows"][2] for n in names])
    print("pose_err before", before.round(3), "after", after.round(3), "means", before.mean(), after.mean())
    assert after.mean() < before.mean()
    for n in names:
        r = C.ref(n)
        assert r["cost"][1] <= r["cost"][0], n


# ------------------------------------------------------------------ the C entry's refusals
def _params(B=2, cap=64, cols=3, kp_yx=1, k_f64=0, rounds=2, lm_iters=10, thresh=1.0, size=None):
    p = _lib.PoseRefineParams()
    p.struct_size = ctypes.sizeof(_lib.PoseRefineParams) if size is None else size
    p.B, p.cap, p.cols, p.kp_yx, p.k_f64, p.rounds, p.lm_iters, p.thresh = B, cap, cols, kp_yx, k_f64, rounds, lm_iters, thresh
    return p


BAD = {"struct_size_0": dict(size=0), "struct_size_short": dict(size=8), "B_0": dict(B=0), "cap_0": dict(cap=0), "cols_1": dict(cols=1),
       "cols_4": dict(cols=4), "kp_yx_2": dict(kp_yx=2), "k_f64_2": dict(k_f64=2), "rounds_0": dict(rounds=0), "rounds_5": dict(rounds=5),
       "lm_iters_0": dict(lm_iters=0), "lm_iters_51": dict(lm_iters=51), "thresh_0": dict(thresh=0.0), "thresh_nan": dict(thresh=float("nan")),
       "thresh_inf": dict(thresh=float("inf"))}
POINTERS = ("mk0", "mk1", "nmatch", "K0", "K1", "R_in", "t_in", "mask_in", "status_in", "T_0to1", "ws", "R_out", "t_out", "mask_out", "rows_out",
            "info_out", "cost_out", "stream")
OPTIONAL = ("T_0to1", "rows_out", "cost_out", "stream")


def test_struct_and_signatures():
    assert [f[0] for f in _lib.PoseRefineParams._fields_] == ["struct_size", "B", "cap", "cols", "kp_yx", "k_f64", "rounds", "lm_iters", "thresh"]
    assert ctypes.sizeof(_lib.PoseRefineParams) == 48
    res, args = _lib.SIGNATURES["einx_relative_pose_refine"]
    assert res is ctypes.c_int and len(args) == 1 + len(POINTERS)
    assert _lib.SIGNATURES["einx_relative_pose_refine_ws_bytes"][0] is ctypes.c_size_t
    # the estimator's own struct and entry are as they were
    assert [f[0] for f in _lib.PoseParams._fields_] == ["struct_size", "B", "cap", "cols", "kp_yx", "k_f64", "max_iters", "thresh", "conf", "seed"]
    assert len(_lib.SIGNATURES["einx_relative_pose"][1]) == 14


def test_workspace_query():
    L = pkg.native.lib()
    q = lambda p: L.einx_relative_pose_refine_ws_bytes(ctypes.byref(p))  # noqa: E731
    small, full = q(_params()), q(_params(32, 1024))
    assert small > 0 and small % 256 == 0 and full % 256 == 0
    assert 32 * 1024 * 33 <= full < 32 * 1024 * 34 + 3 * 256  # the normalised points and one flag per match
    assert q(_params(rounds=4, lm_iters=50)) == small  # no term in the options
    for name, kw in BAD.items():
        assert q(_params(**kw)) == 0, name
    assert L.einx_relative_pose_refine_ws_bytes(None) == 0
    assert L.einx_abi_version() == 6  # additive symbols only


@pytest.mark.parametrize("name", list(BAD) + ["null_" + n for n in POINTERS if n not in OPTIONAL])
def test_refusals(name):
    """every refusal returns an error with a message before anything touches the device (the pointers are never read)"""
    L = pkg.native.lib()
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    p = _params(**BAD.get(name, {}))
    args = [None if name == "null_" + n or n in OPTIONAL else ptr for n in POINTERS]
    rc = L.einx_relative_pose_refine(ctypes.byref(p), *args)
    assert rc != 0
    msg = L.einx_last_error().decode()
    assert msg.startswith("einx_relative_pose_refine: ") and len(msg) > len("einx_relative_pose_refine: "), msg
    if name.startswith("null_"):
        assert "null pointer" in msg


# ------------------------------------------------------------------ the Python layer
def test_python_refusals():
    mk = torch.zeros((1, 8, 3))
    n, K = torch.zeros(1, dtype=torch.int32), torch.eye(3)[None]
    R, t, mask = torch.eye(3, dtype=torch.float64)[None], torch.zeros((1, 3), dtype=torch.float64), torch.zeros((1, 8), dtype=torch.bool)
    mr = types.SimpleNamespace(mk0=mk, mk1=mk, nmatch=n)
    for kw, word in ((dict(rounds=0), "rounds"), (dict(rounds=5), "rounds"), (dict(lm_iters=0), "lm_iters"), (dict(lm_iters=51), "lm_iters"),
                     (dict(rounds=1.5), "rounds")):
        with pytest.raises(ValueError, match=word):
            NM.refine_relative_pose(mk, mk, n, K, K, R, t, mask, n, **kw)
    for fn, head in ((NM.relative_pose, (mk, mk, n, K, K)), (NM.batch_relative_pose, (mr, K, K))):
        for kw, word in ((dict(refine=True, refine_rounds=0), "refine_rounds"), (dict(refine=True, refine_rounds=5), "refine_rounds"),
                         (dict(refine=True, refine_iters=0), "refine_iters"), (dict(refine=True, refine_iters=51), "refine_iters"),
                         (dict(refine_rounds=3), "refine=True"), (dict(refine_iters=5), "refine=True")):
            with pytest.raises(ValueError, match=word):
                fn(*head, **kw)
    mnn = types.SimpleNamespace(matcher=import_module(pkg.__name__ + ".core.modules.Matchers").Matcher(pkg.default_config("SP_MNN"), None, device="cpu"))
    with pytest.raises(ValueError, match="pose_refine"):
        pkg.DifferentTimeEvaluator(mnn, 5, pose_refine=2)


def test_signatures_keep_todays_parameters():
    today = [("mk0", inspect.Parameter.empty), ("mk1", inspect.Parameter.empty), ("nmatch", inspect.Parameter.empty), ("K0", inspect.Parameter.empty),
             ("K1", inspect.Parameter.empty), ("T_0to1", None), ("thresh", 1.0), ("conf", 0.999), ("ordering", "yx"), ("max_iters", 1000),
             ("seed", NM.POSE_SEED)]
    new = [("refine", False), ("refine_rounds", 2), ("refine_iters", 10)]
    got = [(k, v.default) for k, v in inspect.signature(NM.relative_pose).parameters.items()]
    assert got == today + new
    got = [(k, v.default) for k, v in inspect.signature(NM.batch_relative_pose).parameters.items()]
    assert got == [("mr", inspect.Parameter.empty)] + today[3:9] + new
    got = [(k, v.default) for k, v in inspect.signature(NM.refine_relative_pose).parameters.items()]
    assert got == today[:5] + [(k, inspect.Parameter.empty) for k in ("R", "t", "mask", "status")] + [("T_0to1", None), ("thresh", 1.0),
                                                                                                     ("ordering", "yx"), ("rounds", 2), ("lm_iters", 10)]
    sig = inspect.signature(MM.RelativePoseEstimation.__init__).parameters
    assert list(sig)[-1] == "refine" and sig["refine"].default is False
    assert MM.RelativePoseEstimation("RPE", (5, 10, 20)).refine is False and MM.RelativePoseEstimation("RPE", (5,), refine=True).refine is True
    sig = inspect.signature(pkg.DifferentTimeEvaluator.__init__).parameters
    assert list(sig)[-1] == "pose_refine" and sig["pose_refine"].default is False


def test_evaluator_keys_on_fake_rows():
    mnn = types.SimpleNamespace(matcher=import_module(pkg.__name__ + ".core.modules.Matchers").Matcher(pkg.default_config("SP_MNN"), None, device="cpu"))
    rows = torch.tensor([[1.0, 2.0, 2.0, 0.5], [7.0, 3.0, 7.0, 0.4], [np.inf, np.inf, np.inf, 0.0], [0.5, 0.2, 0.5, 0.9]], dtype=torch.float64)
    kept = torch.tensor([[1.0], [0.0], [-1.0], [1.0]], dtype=torch.float64)
    res = {}
    for flag in (False, True):
        ev = pkg.DifferentTimeEvaluator(mnn, 5, pose_refine=flag)
        ev._metric_mean.add(torch.from_numpy(np.arange(2 * len(ev.names), dtype=np.float64).reshape(2, -1) / 8.0))
        ev._pose_rows.append(rows)
        ev._pose_kept.append(kept[:2])
        ev._pose_kept.append(kept[2:])
        res[flag] = ev.result()
    assert "RPE_refined_ratio" not in res[False]
    assert list(res[True]) == list(res[False]) + ["RPE_refined_ratio"] and res[True]["RPE_refined_ratio"] == pytest.approx(2 / 3)
    assert {k: res[True][k] for k in res[False]} == res[False]
    assert np.isnan(H.refined_summary(torch.tensor([[-1.0]]))["RPE_refined_ratio"])
