"""The float64 restatement of the MNN matcher (tests/mnn_f64.py) against the C oracle and the reference's fixtures, and the
exactness claim its GPU companion (test_mnn_f64_gpu.py) rests on.  No GPU."""
import json
import os

import numpy as np
import pytest

import mnn_f64 as F
from helpers import GOLDEN, Golden, mnn_inputs, r2_mnn_inputs

MNN = Golden("mnn")
_Z = np.load(os.path.join(GOLDEN, "r2.npz"))
MNNS = {c["name"]: c for c in json.loads(bytes(_Z["meta"]).decode())["mnn_cases"]}
TIED = ("alleq", "dup", "zero", "ratio_dup")
EPS32 = float(np.finfo(np.float32).eps)


def _assert_equals_oracle(oracle, tag, d0, d1):
    """matches, scores and similarity equal; log_assignment within the fp32 evaluation's own error, which is printed"""
    n, m = d0.shape[0], d1.shape[0]
    R = F.Restated(d0, d1)
    exp = oracle.mnn(d0, d1, want_la=True, want_sim=True)
    assert np.array_equal(exp["similarity"].astype(np.float64), R.sim), tag
    m0, m1, s0, s1 = R.matches()
    assert np.array_equal(m0, exp["matches0"]) and np.array_equal(m1, exp["matches1"]), tag
    assert np.array_equal(s0, exp["matching_scores0"]) and np.array_equal(s1, exp["matching_scores1"]), tag
    la = R.log_assignment()
    err = float(np.abs(exp["log_assignment"].astype(np.float64) - la).max())
    # a plain fp32 evaluation of x - max - log(sum exp): a handful of roundings at |la|'s magnitude plus the relative error of the
    # fp32 sum of up to 2049 exps in (0, 1] (error <= terms x eps/2 relative, the log turns it into an absolute error)
    bound = 8 * EPS32 * max(1.0, float(np.abs(la).max())) + 2 * max(n, m) * EPS32
    print(f"{tag}: oracle log_assignment vs float64 {err:.3e} (bound {bound:.3e}, max |la| {np.abs(la).max():.3f})")
    assert err <= bound, tag
    for ratio, dist in F.THRESHOLDS:
        if ratio and (n < 2 or m < 2):
            continue  # the oracle raises like torch.topk(2); the kernels skip the ratio test there (checked below)
        e = oracle.mnn_thresh(d0, d1, ratio, dist)
        t0, t1, ts0, ts1 = R.matches(ratio, dist)
        assert np.array_equal(t0, e["matches0"]) and np.array_equal(t1, e["matches1"]), (tag, ratio, dist)
        assert np.array_equal(ts0, e["matching_scores0"]) and np.array_equal(ts1, e["matching_scores1"]), (tag, ratio, dist)


@pytest.mark.parametrize("family", F.FAMILIES)
@pytest.mark.parametrize("D", [4, 36, 64, 260])
def test_restatement_equals_oracle_on_exact_inputs(oracle, family, D):
    for n, m in ((1, 1), (5, 1), (129, 257), (1025, 2049)):
        d0, d1, _ = F.make_pair(family, 17 * D + n, n, m, D)
        _assert_equals_oracle(oracle, f"{family} D={D} {n}x{m}", d0, d1)


def test_single_candidate_skips_the_ratio_test():
    """thresh_match: with one candidate there is no second neighbour and the ratio test does not apply (the distance test does)"""
    d0, d1, _ = F.make_pair("unit", 3, 5, 1, 36)
    d1[0] = d0[2]
    R = F.Restated(d0, d1)
    assert np.isnan(R.sec0).all() and not np.isnan(R.sec1).any()
    m0, m1, _, _ = R.matches(ratio=0.5)
    assert m0[2] == 0 and m1[0] == 2 and (np.delete(m0, 2) == -1).all()
    d0[:] = d0[2]
    d1[0] = -d0[2]  # every similarity -1: d = 4
    assert (F.Restated(d0, d1).matches(dist=1.0)[0] == -1).all()


@pytest.mark.parametrize("name", list(MNN.cases))
def test_restatement_equals_reference_fixtures(name):
    c = MNN.cases[name]
    d0, d1, k0, k1 = mnn_inputs(c)
    R = F.Restated(d0, d1)
    m0, m1, s0, s1 = R.matches()
    assert np.array_equal(m0, MNN[f"{name}.matches0"][0]) and np.array_equal(m1, MNN[f"{name}.matches1"][0])
    assert np.array_equal(s0, MNN[f"{name}.mscores0"][0]) and np.array_equal(s1, MNN[f"{name}.mscores1"][0])
    mk0, mk1 = F.matched_kpts(k0, k1, m0, 3)
    assert np.array_equal(mk0, MNN[f"{name}.matched_kpts0"]) and np.array_equal(mk1, MNN[f"{name}.matched_kpts1"])
    la = R.log_assignment()
    if f"{name}.la" in MNN:
        np.testing.assert_allclose(la, MNN[f"{name}.la"][0], atol=2e-5, rtol=0)
    else:
        np.testing.assert_allclose(la[::37, ::41], MNN[f"{name}.la_probe"], atol=2e-5, rtol=0)


@pytest.mark.parametrize("name", [n for n in MNNS if n not in TIED])
def test_restatement_equals_reference_threshold_fixtures(name):
    c = MNNS[name]
    d0, d1, k0, k1 = r2_mnn_inputs(c)
    m0, m1, _, _ = F.Restated(d0, d1).matches(c.get("ratio"), c.get("dist"))
    assert np.array_equal(m0, _Z[f"{name}.matches0"][0]) and np.array_equal(m1, _Z[f"{name}.matches1"][0])
    mk0, mk1 = F.matched_kpts(k0, k1, m0, 3)
    assert np.array_equal(mk0, _Z[f"{name}.matched_kpts0"]) and np.array_equal(mk1, _Z[f"{name}.matched_kpts1"])


def test_families_are_what_they_claim():
    for D in (4, 32, 36, 64, 260):
        u = F.exact_unit(D, 50, D).astype(np.float64)
        s = 16 if D >= 16 else 4
        assert ((u != 0).sum(1) == s).all() and np.array_equal(np.abs(u[u != 0]), np.full((50 * s,), 1 / np.sqrt(s)))
        assert np.array_equal((u * u).sum(1), np.ones(50))
        sim = u @ u.T
        assert np.array_equal(sim * 16, np.round(sim * 16)) and np.abs(sim).max() <= 1
        d = F.exact_dense(D, 50, D).astype(np.float64)
        assert np.array_equal(d * 8, np.round(d * 8)) and np.abs(d).max() <= 1


def test_fp32_similarity_is_exact_for_every_gpu_case():
    """the claim test_mnn_f64_gpu.py relies on: on its inputs the fp32 similarity IS the float64 one, whatever the summation order
    (numpy's blocked fp32 matmul here, the matrix cores' k-ordered chain there)"""
    lists = F.exactness_lists()
    assert len(lists) >= 2 * len(F.CASES)
    for tag, d0, d1 in lists:
        assert d0.dtype == np.float32 and d1.dtype == np.float32
        assert not np.isnan(d0).any() and not np.isnan(d1).any(), tag
        sim64 = d0.astype(np.float64) @ d1.astype(np.float64).T
        assert np.array_equal((d0 @ d1.T).astype(np.float64), sim64), tag
        # every partial sum is exact too: |sim| and the sum of |products| stay far below 2^24 units of the common denominator
        assert np.array_equal(sim64 * 64, np.round(sim64 * 64)), tag
        assert (np.abs(d0.astype(np.float64)) @ np.abs(d1.astype(np.float64)).T).max(initial=0) * 64 < 2 ** 24, tag


def test_gpu_cases_hold_what_the_gpu_test_needs():
    """planted matches on both sides of index 1024, exact ties, and both threshold equalities decided by `<=`"""
    for name in ("beyond_1024", "beyond_1024_t"):
        for fam in F.FAMILIES:
            c = F.build_case(name, fam)
            for ratio, dist in ((None, None), (0.75, 1.0)):
                hit = np.nonzero(c.pairs[0].matches(ratio, dist)[0] > -1)[0]
                assert (hit >= 1024).any() and (hit < 1024).any(), (name, fam, ratio, dist)
    d0, d1, _, _, info = F.matcher_pair()
    for ratio, dist in ((None, None), (0.5, None), (0.75, 1.0)):
        hit = np.nonzero(F.Restated(d0, d1).matches(ratio, dist)[0] > -1)[0]
        assert (hit >= 1024).any() and (hit < 1024).any(), ("matcher_pair", ratio, dist)
    assert info["ratio_eq"][0] >= 1024
    cc = F.compact_case()
    nm = np.array([(R.matches()[0] > -1).sum() for R in cc.pairs])
    assert cc.B > 256 and nm[256:].sum() > 0 and (nm == 0).any() and (nm > 1).any()
    seen_ratio = seen_dist = 0
    for name in F.CASES:
        c = F.build_case(name, "unit")
        for b, R in enumerate(c.pairs):
            info = c.info[b]
            for kind, a, bb in info["dups"]:
                d = c.d0[b] if kind == "side0" else c.d1[b]
                assert np.array_equal(d[a], d[bb])
            if info["ratio_eq"] is None:
                continue
            (i, j), (p, q) = info["ratio_eq"], info["dist_eq"]
            # row i / column j: d0 == 0.5^2 * d2 exactly; the match stands only because the comparison is `<=`
            assert R.best0[i] == j and R.best1[j] == i
            assert 2 * (1 - R.top0[i]) == 0.25 * (2 * (1 - R.sec0[i])) and 2 * (1 - R.top1[j]) == 0.25 * (2 * (1 - R.sec1[j]))
            assert R.matches(ratio=0.5)[0][i] == j and R.matches(ratio=0.5)[1][j] == i
            # row p / column q: d0 == 1.0^2 exactly
            assert R.best0[p] == q and R.best1[q] == p and 2 * (1 - R.top0[p]) == 1.0 and 2 * (1 - R.top1[q]) == 1.0
            assert R.matches(dist=1.0)[0][p] == q and R.matches(ratio=0.75, dist=1.0)[0][p] == q
            assert R.matches(ratio=0.5)[0][p] == -1  # a decision the other way on the same row
            seen_ratio += 1
            seen_dist += 1
    assert seen_ratio >= 4 and seen_dist >= 4
