"""The float64 restatement of the homography contract (tests/homography_f64.py) on its own, and the host API of
HomographyEstimation -- no GPU."""
from importlib import import_module

import numpy as np
import pytest
import torch

import homography_f64 as Hm
import pose_f64 as P
from helpers import load_pkg

pkg = load_pkg()
_mm = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
_harness = import_module(pkg.__name__ + ".harness")


def test_homography_estimation_constructs_like_the_reference():
    he = _mm.HomographyEstimation("HE", [3, 5, 10])
    assert he.metric_name == "HE" and he.correctness_thresh == [3, 5, 10] and he.ordering == "yx" and he.error_list == []
    assert he.to_device.type in ("cuda", "cpu")
    assert _mm.HomographyEstimation("HE", correctness_thresh=(3, 5), ordering="xy").ordering == "xy"
    with pytest.raises(AssertionError):
        _mm.HomographyEstimation("HE", [3], ordering="zz")
    with pytest.raises(AssertionError):
        _mm.HomographyEstimation("HE", 3)
    # the malformed call (a TypeError in the reference): the message names what is missing and what the estimator is
    with pytest.raises(NotImplementedError, match="correctness_thresh.*DESIGN.md 8c.*not OpenCV"):
        _mm.HomographyEstimation("HE")
    assert not hasattr(_mm, "_NeedsOpenCV")


def test_compute_all_auc_on_a_hand_list():
    he = _mm.HomographyEstimation("HE", [3, 5, 10])
    he.error_list = [1.0, 2.0, np.inf, 4.0]
    auc = he.compute_all_auc()
    # finite errors 1, 2, 4, recall 1/3, 2/3, 1: trapezoids up to each threshold, divided by it
    want3 = (0.5 * 1 * (1 / 3) + 0.5 * 1 * (1 / 3 + 2 / 3) + 1 * (2 / 3)) / 3
    want5 = (0.5 * 1 * (1 / 3) + 0.5 * 1 * (1 / 3 + 2 / 3) + 0.5 * 2 * (2 / 3 + 1) + 1 * 1) / 5
    assert set(auc) == {"3", "5", "10"}
    assert abs(auc["3"] - want3) < 1e-12 and abs(auc["5"] - want5) < 1e-12
    assert auc == _mm.compute_auc(he.error_list, [3, 5, 10])


def test_generator_is_the_one_of_8b():
    assert [Hm.splitmix64(i) for i in range(3)] == [0xE220A8397B1DCDAF, 0x910A2DEC89025CC1, 0x975835DE1C9756CE]
    # attempt 0 uses 8b's keys: the first four of its five draws
    for it, n in ((0, 300), (7, 6), (3, 1000)):
        assert Hm.draw(Hm.DEFAULT_SEED, it, 0, n) == P.draw(P.DEFAULT_SEED, it, n)[:4]
    d = Hm.draw(Hm.DEFAULT_SEED, 7, 3, 5)
    assert len(set(d)) == 4 and all(0 <= v < 5 for v in d)
    assert Hm.draw(Hm.DEFAULT_SEED, 3, 0, 1000) != Hm.draw(Hm.DEFAULT_SEED, 3, 1, 1000)
    assert Hm.draw(Hm.DEFAULT_SEED, 3, 0, 1000) != Hm.draw(Hm.DEFAULT_SEED, 4, 0, 1000)


def test_update_iters_cases():
    assert Hm.update_iters(0.995, 0.0, 2000) == 0          # no outlier: denom underflows, the scan stops
    assert Hm.update_iters(0.995, 1.0, 2000) == 2000       # no inlier: log(1) = 0, the bound stays
    assert Hm.update_iters(0.995, 0.3, 2000) == int(np.floor(np.log(0.005) / np.log(1 - 0.7 ** 4) + 0.5)) == 19
    assert Hm.update_iters(0.995, 0.6, 2000) == 204
    assert Hm.update_iters(0.995, 0.9, 100) == 100         # more than the bound: the bound stays
    assert Hm.update_iters(2.0, 0.5, 2000) == 2000 and Hm.update_iters(-1.0, 0.5, 2000) == 0  # conf clamped to [0, 1]
    assert Hm.update_iters(0.999, 0.3, 1000, model_points=5) == P.update_iters(0.999, 0.3, 1000)


def test_check_subset():
    sq = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], float)
    assert Hm.check_subset(sq, sq + 3.0)
    assert not Hm.check_subset(sq, sq * [-1.0, 1.0])                      # a reflection: every orientation flips
    assert not Hm.check_subset(sq, sq[[0, 1, 3, 2]])                      # two points swapped: some flip
    assert not Hm.check_subset(np.array([[0, 0], [5, 5], [10, 10], [0, 10]], float), sq)  # three collinear points
    assert not Hm.check_subset(sq, np.repeat(sq[:1], 4, 0))


def test_noise_free_homography_is_recovered():
    rng = np.random.default_rng(5)
    for n in (4, 5, 50, 300):
        Ht = Hm.random_homography(rng)
        M = np.stack([rng.uniform(0, 345, n), rng.uniform(0, 259, n)], 1)
        m = Hm.warp(Ht, M)
        H = Hm.dlt(M, m)
        assert np.linalg.norm(H - Ht) / np.linalg.norm(Ht) < 1e-9, n
        H2 = Hm.polish(H, M, m)
        assert np.linalg.norm(H2 - Ht) / np.linalg.norm(Ht) < 1e-9, n
    # and through the whole estimator, to float32 storage's accuracy, with every point an inlier
    k0, k1, Ht = Hm.scene(rng, 200)
    r = Hm.homography(k0, k1)
    assert r["status"] == "ok" and r["it"] == 0 and r["mask"].all()
    assert np.linalg.norm(r["H"] - Ht) / np.linalg.norm(Ht) < 1e-5


def test_polish_repairs_a_perturbed_fit():
    rng = np.random.default_rng(6)
    Ht = Hm.random_homography(rng)
    M = np.stack([rng.uniform(0, 345, 100), rng.uniform(0, 259, 100)], 1)
    m = Hm.warp(Ht, M)
    H0 = Ht * (1 + 1e-3 * rng.normal(size=(3, 3)))
    H0 = H0 / H0[2, 2]
    assert np.linalg.norm(Hm.polish(H0, M, m) - Ht) / np.linalg.norm(Ht) < 1e-9


def test_degenerate_inputs():
    rng = np.random.default_rng(7)
    k0, k1, _ = Hm.scene(rng, 40)
    assert Hm.homography(k0[:3], k1[:3])["status"] == "few"
    assert Hm.homography(k0[:0], k1[:0])["status"] == "few"
    four = Hm.homography(k0[:4], k1[:4])
    assert four["status"] == "ok" and four["it"] == 0 and four["mask"].all()
    same = np.repeat(k0[:1], 4, 0)
    assert Hm.homography(same, same)["status"] == "noH"
    xy = Hm.homography(k0[:, 1::-1], k1[:, 1::-1], ordering="xy")  # two columns, the other ordering: the same answer
    yx = Hm.homography(k0, k1)
    assert xy["it"] == yx["it"] and np.array_equal(xy["H"], yx["H"]) and np.array_equal(xy["mask"], yx["mask"])


def test_batch_of_the_kernel_tests_holds_for_the_restatement_alone():
    """statuses, the ground-truth bound and the distance of every error from every threshold, without any pinned pair"""
    pairs = Hm.batch()
    assert sorted({len(p[0]) for p in pairs[:16]}) == [4, 5, 8, 50, 300, 1024]
    for b, (k0, k1, Ht) in enumerate(pairs):
        r = Hm.homography(k0, k1)
        row = Hm.rows(r, Ht.astype(np.float32), Hm.IMG_SHAPE)
        if b in Hm.BATCH_FAIL:
            assert r["status"] == Hm.BATCH_FAIL[b] and row == [0.0, 0.0, 0.0, np.inf, 0.0]
            continue
        assert r["status"] == "ok" and r["it"] < 2000
        assert all(abs(row[3] - t) > 0.1 for t in (3, 5, 10)), (b, row)
        if b in Hm.BATCH_GT:
            assert row[3] < Hm.GT_BOUND, (b, row)


def test_corner_rows_are_the_reference_expression():
    """update_one's torch expression (matching_metrics.py:265-297), evaluated on the CPU on the same H.  torch.mm leaves the
    order and the fusing of its three-term sums to the BLAS library, so the float32 corner coordinates (below 512 px: one ulp is
    2^-14 = 6.1e-5 px) can differ from the explicit left-to-right sums of 8c by a few roundings each; the mean distance is held to
    8 ulp(512) = 4.9e-4 px, and the ratios are equal (no error of these seeds lies that close to a threshold)."""
    tol = 8 * 2.0 ** -14
    rng = np.random.default_rng(9)
    for _ in range(50):
        Ht = Hm.random_homography(rng)
        Hp = Ht * (1 + 1e-3 * rng.normal(size=(3, 3)))
        img_shape = (260, 346)
        true_h, pred_h = torch.from_numpy(Ht).float(), torch.from_numpy(Hp).float()
        corners = torch.tensor([[0, 0, 1], [img_shape[1] - 1, 0, 1], [0, img_shape[0] - 1, 1], [img_shape[1] - 1, img_shape[0] - 1, 1]],
                               dtype=torch.float32)
        real = torch.mm(corners, torch.transpose(true_h, 0, 1))
        real = real[:, :2] / real[:, 2:]
        warped = torch.mm(corners, torch.transpose(pred_h, 0, 1))
        warped = warped[:, :2] / warped[:, 2:]
        mean_dist = torch.mean(torch.linalg.norm(real - warped, dim=1))
        correct = mean_dist <= torch.tensor([3, 5, 10], dtype=torch.float32)
        ratios, err = Hm.corner_rows(Ht, Hp, img_shape)
        assert err.dtype == np.float32
        assert abs(float(err) - float(mean_dist)) <= tol, (float(err), float(mean_dist))
        assert all(abs(float(err) - t) > tol for t in (3, 5, 10))
        assert ratios == correct.float().tolist()


def test_he_summary_forms_the_scripts_means():
    rows = np.array([[1, 1, 1, 0.5, 0.8], [0, 1, 1, 4.0, 0.5], [0, 0, 0, np.inf, 0.0]])
    out = _harness.he_summary(torch.from_numpy(rows), (3, 5, 10))
    assert list(out) == ["HE@3_ratio", "HE@5_ratio", "HE@10_ratio", "HE_errors", "HE_inliers", "HE@3_auc", "HE@5_auc", "HE@10_auc"]
    assert out["HE@3_ratio"] == 1 / 3 and out["HE_errors"] == 2.25 and abs(out["HE_inliers"] - 1.3 / 3) < 1e-15
    auc = _mm.compute_auc([0.5, 4.0, np.inf], [3, 5, 10])
    assert [out[f"HE@{t}_auc"] for t in (3, 5, 10)] == [auc[str(t)] for t in (3, 5, 10)]
    assert _harness.gather_pose_rows is _harness.gather_rows
