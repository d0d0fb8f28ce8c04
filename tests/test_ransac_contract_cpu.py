"""What the RANSAC contract tests on the device (test_pose_contract_gpu.py, test_homography_contract_gpu.py) rely on, established
on the float64 restatements alone (tests/pose_f64.py, tests/homography_f64.py) over the fixed inputs of tests/ransac_cases.py:
every case is decisive, the K0 != K1 cases can see a swap of the two cameras, the round-boundary seeds give their iterations,
and the bound of the pose certificate.

ransac_cases.CERT_WORST is the largest |x2' E' x1| of the restatement's own (R, t) over the five drawn matches of every pose
input (printed by test_certificate_bound); the gate of the device's certificate is 10 x that, under the ceiling of 1e-6
(another iteration's sample gives 3e-3 and swapped cameras 4e-2 on a noisy case)."""
import numpy as np
import pytest

import homography_f64 as Hm
import pose_f64 as P
import ransac_cases as C

CERT_WORST, CERT_GATE, CERT_CEILING = C.CERT_WORST, C.CERT_GATE, C.CERT_CEILING
HE_THR, HE_ERR_GATE = C.HE_THR, C.HE_ERR_GATE


def _pose_err(pair, r):
    return P.pose_errors(pair[4], r["R"], r["t"])[2] if r["status"] == "ok" else np.inf


def _no_point_on_the_threshold(pair, kw, r):
    """test_pose_gpu.py's rule asks that no float64 Sampson error lies within 1e-6 (relative) of thr^2; 1e-4 here, which also
    covers the certificate's mask: E' rebuilt from (R, t) is within 1e-12 of the model the kernel scored (CERT_GATE), which moves
    a squared error of about thr^2 by far less than 1e-4 of it"""
    x1, x2 = C.pose_points(pair)
    thr2 = P.ransac_threshold(kw.get("thresh", 1.0), pair[2], pair[3]) ** 2
    _, e64 = P.sampson_f32(r["E"], x1, x2)
    return not np.any(np.abs(e64 - thr2) <= 1e-4 * thr2)


@pytest.mark.parametrize("i", range(len(C.POSE_CASES)))
def test_pose_case_is_decisive(i):
    pair, kw, r = C.pose_ref(i)
    assert r["status"] == C.POSE_STATUS.get(i, "ok")
    if r["status"] != "ok":
        return
    assert r["it"][0] < kw.get("max_iters", 1000)
    assert _no_point_on_the_threshold(pair, kw, r)


@pytest.mark.parametrize("i", range(len(C.POSE_CASES)))
def test_pose_case_sees_swapped_cameras(i):
    """K0 != K1 in every case: the pose meets the ground-truth bound of its outlier level, and the restatement with the two
    matrices swapped is off by more than 10 degrees (or finds no pose)"""
    pair, kw, r = C.pose_ref(i)
    a0, a1, K0, K1, T = pair
    assert K0.dtype == K1.dtype == C.POSE_CASES[i][4]
    assert all(K0[j, k] != K1[j, k] for j, k in ((0, 0), (1, 1), (0, 2), (1, 2))) and K0[0, 0] != K0[1, 1] and K1[0, 0] != K1[1, 1]
    bound = P.GT_BOUNDS[C.POSE_OUTLIER_BOUND[C.POSE_CASES[i][3]]]
    assert _pose_err(pair, r) < bound, _pose_err(pair, r)
    swapped = P.relative_pose(a0, a1, K1, K0, **kw)
    assert _pose_err(pair, swapped) > 10.0, _pose_err(pair, swapped)


def test_certificate_bound():
    """the certificate's residual on the restatement's own (R, t), over every input the device's certificate is asked of: the
    cases, the tiled pairs and the round-boundary pairs"""
    inputs = [(f"case {i}",) + C.pose_ref(i) for i in range(len(C.POSE_CASES))]
    inputs += [(f"tile {k}", p, C.TILE_KW, P.relative_pose(*p[:4], **C.TILE_KW)) for k, p in enumerate(C.tile_pairs("pose"))]
    for scene_seed, it, seed in C.BOUNDARY_SEEDS["pose"]:
        pair, r = C.boundary_ref("pose", scene_seed, seed)
        inputs.append((f"boundary {it}", pair, dict(C.BOUNDARY_KW, seed=seed), r))
    worst = 0.0
    for tag, pair, kw, r in inputs:
        if r["status"] != "ok" or len(pair[0]) <= 5:
            continue
        res = C.sample_residual(pair, r["R"], r["t"], r["it"][0], kw.get("seed", P.DEFAULT_SEED))
        print(f"pose {tag}: it {r['it']} certificate residual {res:.3e}")
        worst = max(worst, res)
    print(f"measured: worst certificate residual of the restatement {worst:.3e}; device gate {CERT_GATE:.3e}")
    assert worst <= CERT_WORST
    assert CERT_GATE == 10 * CERT_WORST and CERT_GATE <= CERT_CEILING
    # the certificate is sharp on a noisy case: the same pose against the next iteration's sample, or with the cameras swapped
    pair, kw, r = C.pose_ref(8)
    other = C.sample_residual(pair, r["R"], r["t"], r["it"][0] + 1)
    swapped = C.sample_residual(pair[:2] + (pair[3], pair[2], pair[4]), r["R"], r["t"], r["it"][0])
    print(f"case 8: next iteration's sample {other:.3e}, swapped cameras {swapped:.3e}")
    assert other > 1e3 * CERT_GATE and swapped > 1e3 * CERT_GATE


@pytest.mark.parametrize("i", range(len(C.HOMOGRAPHY_CASES)))
def test_homography_case_is_decisive(i):
    pair, kw, r = C.homography_ref(i)
    assert r["status"] == C.HOMOGRAPHY_STATUS.get(i, "ok")
    if r["status"] != "ok":
        return
    assert r["it"] < kw.get("max_iters", 2000)
    err = Hm.rows(r, pair[2].astype(np.float32), Hm.IMG_SHAPE, HE_THR)[3]
    assert all(abs(err - t) > HE_ERR_GATE for t in HE_THR)


def test_cases_cover_the_issue():
    kws = [c[5] for c in C.POSE_CASES]
    assert {kw.get("max_iters", 1000) for kw in kws} == {1, 33, 65, 300, 1000} and sum(kw.get("max_iters", 1000) > 300 for kw in kws) == 1
    assert {kw["thresh"] for kw in kws if "thresh" in kw} == {0.25, 2.0} and {kw["conf"] for kw in kws if "conf" in kw} == {0.5, 0.99}
    assert any(kw.get("seed", P.DEFAULT_SEED) != P.DEFAULT_SEED for kw in kws)
    assert {c[1] for c in C.POSE_CASES} >= {5, 6, 60, 257, 513} and {c[4] for c in C.POSE_CASES} == {np.float32, np.float64}
    kws = [c[4] for c in C.HOMOGRAPHY_CASES]
    assert {kw.get("max_iters") for kw in kws} == {1, 33, 65, 300}
    assert {kw["thresh"] for kw in kws if "thresh" in kw} == {1.0, 6.0} and {kw["conf"] for kw in kws if "conf" in kw} == {0.5}
    assert any("seed" in kw for kw in kws) and {c[1] for c in C.HOMOGRAPHY_CASES} >= {4, 5, 257, 513}
    # the max_iters = 33 result must equal the max_iters = 300 one whenever the chosen iteration is below 33: the cases do choose one
    assert C.pose_ref(11)[2]["it"][0] < 33 and C.homography_ref(5)[2]["it"] < 33
    # slots either side of a 64-lane block hold different pairs, one of them "few" and one a failure
    for b in (63, 64, 127, 128):
        assert b % len(C.TILE_SPEC) != (b + 1) % len(C.TILE_SPEC)
    assert C.TILE_SPEC[64 % len(C.TILE_SPEC)] == "few" and C.TILE_SPEC[128 % len(C.TILE_SPEC)] == "same"
    assert all(s in ("few", "same") or s[0] <= C.TILE_CAP for s in C.TILE_SPEC)


@pytest.mark.parametrize("kind", ["pose", "homography"])
def test_tile_pairs_statuses(kind):
    for k, p in enumerate(C.tile_pairs(kind)):
        r = P.relative_pose(*p[:4], **C.TILE_KW) if kind == "pose" else Hm.homography(p[0], p[1], **C.TILE_KW)
        want = {"few": "few", "same": "noE" if kind == "pose" else "noH"}.get(C.TILE_SPEC[k], "ok")
        assert r["status"] == want, (k, r["status"])
        if kind == "pose" and want == "ok":
            assert _no_point_on_the_threshold(p, C.TILE_KW, r), k


@pytest.mark.parametrize("kind", ["pose", "homography"])
def test_boundary_seeds_give_their_iterations(kind):
    """verified, not searched (ransac_cases.search_boundary_seeds found them)"""
    entries = C.BOUNDARY_SEEDS[kind]
    assert sorted(it for _, it, _ in entries) == sorted(C.BOUNDARY_ITERS)
    for scene_seed, it, seed in entries:
        assert C.chosen_iteration(kind, scene_seed, seed) == it, (scene_seed, it, seed)
        if kind == "pose":
            pair, r = C.boundary_ref(kind, scene_seed, seed)
            assert _no_point_on_the_threshold(pair, C.BOUNDARY_KW, r), (scene_seed, it, seed)


def test_search_finds_the_first_homography_seed():
    """the search function on a range short enough to be cheap: the first boundary seed it meets is the committed one"""
    scene_seed, it, seed = C.BOUNDARY_SEEDS["homography"][0]
    assert C.search_boundary_seeds("homography", scene_seed, wanted=(it,), seeds=range(1, seed + 1)) == {it: seed}
