"""Relative pose without a GPU: the float64 restatement of DESIGN.md 8b (tests/pose_f64.py) against ground truth, and the host
side of the reference's RelativePoseEstimation (constructor, relative_pose_error, compute_all_auc)."""
import math

import numpy as np
import pytest

import pose_f64 as P
from helpers import load_pkg

pkg = load_pkg()
from importlib import import_module  # noqa: E402

_mm = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
_harness = import_module(pkg.__name__ + ".harness")


def test_relative_pose_estimation_constructs_like_the_reference():
    rpe = _mm.RelativePoseEstimation("RPE", pose_thresh=[5, 10, 20])
    assert rpe.metric_name == "RPE" and rpe.pose_thresh == [5, 10, 20]
    assert rpe.ransac_thresh == 1.0 and rpe.ransac_conf == 0.999 and rpe.ordering == "yx" and rpe.error_list == []
    assert rpe.to_device.type in ("cuda", "cpu")
    with pytest.raises(AssertionError):
        _mm.RelativePoseEstimation("RPE", [5], ordering="zz")
    with pytest.raises(NotImplementedError, match="OpenCV"):
        _mm.HomographyEstimation("HE")


def test_generator_is_pinned():
    assert [P.splitmix64(i) for i in range(3)] == [0xE220A8397B1DCDAF, 0x910A2DEC89025CC1, 0x975835DE1C9756CE]
    assert P.draw(P.DEFAULT_SEED, 0, 300) == P.draw(P.DEFAULT_SEED, 0, 300)
    d = P.draw(P.DEFAULT_SEED, 7, 6)
    assert len(set(d)) == 5 and all(0 <= v < 6 for v in d)
    assert P.draw(P.DEFAULT_SEED, 3, 1000) != P.draw(P.DEFAULT_SEED, 4, 1000)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_threshold_rule_is_the_reference_expression(dt):
    rng = np.random.default_rng(3)
    for _ in range(200):
        K0 = np.diag([rng.uniform(150, 400), rng.uniform(150, 400), 1.0]).astype(dt)
        K1 = np.diag([rng.uniform(150, 400), rng.uniform(150, 400), 1.0]).astype(dt)
        thresh = float(rng.choice([1.0, 0.5, 2.0]))
        ref = thresh / np.mean([K0[0, 0], K1[1, 1], K0[0, 0], K1[1, 1]])  # matching_metrics.py:417
        assert P.ransac_threshold(thresh, K0, K1) == float(ref)


def _exact_five(rng):
    R = P.rotation(rng.normal(size=3), rng.uniform(1, 15))
    t = rng.normal(size=3)
    X = np.stack([rng.uniform(-2, 2, 5), rng.uniform(-1.5, 1.5, 5), rng.uniform(2, 10, 5)], 1)
    X1 = X @ R.T + t
    return X[:, :2] / X[:, 2:], X1[:, :2] / X1[:, 2:], P.skew(t) @ R


def test_five_point_contains_the_true_essential_matrix():
    rng = np.random.default_rng(11)
    for _ in range(30):
        x1, x2, Et = _exact_five(rng)
        Es = P.solve5(x1, x2)
        assert 1 <= len(Es) <= 10
        Et = Et / np.linalg.norm(Et)
        assert min(min(np.abs(E / np.linalg.norm(E) - Et).max(), np.abs(E / np.linalg.norm(E) + Et).max()) for E in Es) < 1e-8
        zs = [E[2, 1] for E in Es]
        assert zs == sorted(zs)
        for E in Es:
            En = E / np.linalg.norm(E)
            assert abs(np.linalg.det(En)) < 1e-8
            assert np.abs(2 * En @ En.T @ En - np.trace(En @ En.T) * En).max() < 1e-8


def test_degenerate_samples_yield_no_model():
    p = np.full((5, 2), 0.1)
    assert P.solve5(p, p) == []
    line = np.stack([np.linspace(-0.5, 0.5, 5), np.linspace(-0.2, 0.3, 5)], 1)
    assert P.solve5(line, line[::-1] * 0.9) == []


def test_restatement_recovers_ground_truth_noise_free():
    """float64 correspondences and a tight threshold (with the default ~1 px one, a model from an ill-conditioned sample can
    already hold every point and end the scan): the pose error is at arccos's conditioning (about 1e-6 degrees)"""
    rng = np.random.default_rng(21)
    for _ in range(4):
        R = P.rotation(rng.normal(size=3), rng.uniform(1, 15))
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        X = np.stack([rng.uniform(-3, 3, 80), rng.uniform(-2, 2, 80), rng.uniform(2, 10, 80)], 1)
        X1 = X @ R.T + t
        x1, x2 = X[:, :2] / X[:, 2:], X1[:, :2] / X1[:, 2:]
        Es, mask, chosen = P.ransac(x1, x2, 1e-7)
        assert mask.all()
        cnt, Rh, th, ok = P.recover_pose(Es[0], x1, x2, mask)
        assert cnt == 80
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        r_err, t_err, pose_err = P.pose_errors(T, Rh, th)
        assert pose_err < 1e-5, (r_err, t_err)


def test_restatement_noise_free_float32_keypoints():
    """noise-free scenes through float32 keypoints and the default ~1 px threshold (what the GPU test feeds the kernels); the
    forward-driving motion puts the true solution far out in the (x, y, z, 1) parametrisation"""
    rng = np.random.default_rng(51)
    for t_dir in (None, None, P.FORWARD, P.FORWARD):
        kp0, kp1, K0, K1, T = P.scene(rng, 300, t_dir=t_dir, max_deg=3.0 if t_dir else 15.0)
        r = P.relative_pose(kp0, kp1, K0, K1)
        assert r["status"] == "ok" and r["mask"].all()
        assert P.pose_errors(T, r["R"], r["t"])[2] < P.GT_BOUNDS["noise_free"]


def test_restatement_forward_motion_with_noise_and_outliers():
    rng = np.random.default_rng(41)
    for _ in range(2):
        kp0, kp1, K0, K1, T = P.scene(rng, 200, noise=0.5, outliers=0.3, t_dir=P.FORWARD, max_deg=3.0)
        r = P.relative_pose(kp0, kp1, K0, K1)
        assert r["status"] == "ok"
        assert P.pose_errors(T, r["R"], r["t"])[2] < P.GT_BOUNDS["outliers_30"]


@pytest.mark.parametrize("outliers,bound", [(0.3, P.GT_BOUNDS["outliers_30"]), (0.6, P.GT_BOUNDS["outliers_60"])])
def test_restatement_with_noise_and_outliers(outliers, bound):
    """0.5 px noise on MVSEC-like float32 keypoints; the bounds hold the worst of these fixed seeds with margin"""
    rng = np.random.default_rng(31)
    errs = []
    for _ in range(2):
        kp0, kp1, K0, K1, T = P.scene(rng, 200, noise=0.5, outliers=outliers)
        r = P.relative_pose(kp0, kp1, K0, K1)
        assert r["status"] == "ok"
        errs.append(P.pose_errors(T, r["R"], r["t"])[2])
        assert 0.2 < r["mask"].mean() <= 1.0 - outliers + 0.05
    assert max(errs) < bound, errs


def test_relative_pose_error_cases():
    rpe = _mm.RelativePoseEstimation("RPE", pose_thresh=[5, 10, 20])
    T = np.eye(4)
    T[:3, 3] = [1.0, 0.0, 0.0]
    R = P.rotation([0, 0, 1], 3.0)
    t_err, R_err = rpe.relative_pose_error(T, R, np.array([1.0, 0.0, 0.0]))
    assert abs(R_err - 3.0) < 1e-9 and t_err == 0.0
    t_err, _ = rpe.relative_pose_error(T, R, np.array([-1.0, 0.0, 0.0]))  # min(e, 180 - e)
    assert t_err == 0.0
    T0 = np.eye(4)  # zero t_gt: NaN t_err, update_one then takes R_err as the pose error
    with np.errstate(invalid="ignore", divide="ignore"):
        t_err, R_err = rpe.relative_pose_error(T0, R, np.array([1.0, 0.0, 0.0]))
    assert np.isnan(t_err) and abs(R_err - 3.0) < 1e-9
    Ti = np.eye(4)
    Ti[:3, 3] = [np.inf, 0.0, 0.0]  # non-finite t_gt: t_err = 0
    with np.errstate(invalid="ignore"):
        t_err, _ = rpe.relative_pose_error(Ti, R, np.array([1.0, 0.0, 0.0]))
    assert t_err == 0.0
    rpe.error_list = [0.5, 3.0, np.inf, 12.0, np.nan]
    assert rpe.compute_all_auc() == _mm.compute_auc([0.5, 3.0, np.inf, 12.0, np.nan], [5, 10, 20])


def test_rpe_summary_matches_the_reference_loop():
    """harness.rpe_summary = test_events-image_different_time.py:326-334 over update_one's per-pair dicts"""
    rows = np.array([[1.0, 2.0, 2.0, 0.8], [np.inf, np.inf, np.inf, 0.0], [3.0, np.nan, 3.0, 0.5], [7.0, 30.0, 30.0, 0.4]])
    out = _harness.rpe_summary(rows, (5, 10, 20))
    assert out["RPE_R_errs"] == np.mean([1.0, 3.0, 7.0]) and out["RPE_t_errs"] == np.mean([2.0, 30.0])
    assert out["RPE_inliers"] == np.mean(rows[:, 3])
    assert out["RPE@5_ratio"] == np.mean([1.0, 0.0, 1.0, 0.0]) and out["RPE@20_ratio"] == 0.5
    auc = _mm.compute_auc(list(rows[:, 2]), [5, 10, 20])
    for t in (5, 10, 20):
        assert out[f"RPE@{t}_auc"] == auc[str(t)]
    assert math.isfinite(out["RPE@10_auc"])
