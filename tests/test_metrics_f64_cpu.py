"""The float64 restatement of the pair metrics (tests/metrics_f64.py) against the C oracle and the reference's fixtures, and the
exactness and coverage claims its GPU companion (test_metrics_f64_gpu.py) rests on.  No GPU."""
import math

import numpy as np
import pytest

import metrics_f64 as F
from helpers import Golden, metric_case, metric_inputs

METRICS = Golden("metrics")
EPS32 = float(np.finfo(np.float32).eps)
F32 = np.float32


def _pairs():
    """(tag, case, b) of every pair the GPU test feeds the kernels through pair_metrics"""
    for name, fam in F.CASE_IDS:
        c = F.build_case(name, fam)
        for b in range(c.B):
            yield f"{name}.{fam}.{b}", c, b


def _class_case():
    """the metric classes' pair in the shape of a one-pair case"""
    k0, k1, d0, d1, mk0, mk1, H, info = F.class_pair()
    c = F.Case()
    c.name, c.family, c.B, c.kp_yx, c.size0, c.size1, c.mma, c.vdd = "class_pair", "unit", 1, True, F.SIZE0, F.SIZE1, F.THRESHOLDS, F.THRESHOLDS
    c.k0, c.k1, c.d0, c.d1, c.mk0, c.mk1, c.hom = k0[None], k1[None], d0[None], d1[None], mk0[None], mk1[None], H[None]
    c.n, c.m, c.nm, c.info = [len(k0)], [len(k1)], [len(mk0)], [info]
    c.pairs = [F.Restated(k0, k1, d0, d1, mk0, mk1, c.size0, c.size1, H, True)]
    return c


def _all_pairs():
    yield from _pairs()
    yield "class_pair", _class_case(), 0


@pytest.mark.parametrize("name,family", F.CASE_IDS)
def test_restatement_equals_oracle_on_exact_inputs(oracle, name, family):
    """MR, MMA, repeatability and ValidDistance equal oracle.pair_metrics (NaN at the same places); the angle, the one entry that
    goes through acos, within the plain fp32 evaluation's own error, which is measured per record and per output row and printed:
    fp32 rounds the quotient (eps32 / 2 relative; |q| <= 15/16 in the unit family and far less in the dense one, so the angle moves
    by a few eps32 radians), acos and the conversion add a few ulps of at most 180 -- 8 eps32 180 degrees covers all of it."""
    c = F.build_case(name, family)
    nv = len(c.vdd)
    exact = [i for i in range(1 + len(c.mma) + 3 * nv) if i < 1 + len(c.mma) or (i - 1 - len(c.mma)) % 3 != 2]
    angle = [3 + len(c.mma) + 3 * k for k in range(nv)]
    e_row = e_rec = 0.0
    for b in range(c.B):
        exp = oracle.pair_metrics(*c.pair_inputs(b), c.size0, c.size1, None if c.hom is None else c.hom[b], mma_thr=c.mma, vdd_thr=c.vdd,
                                  kp_yx=c.kp_yx)
        row = c.row(b)
        assert np.array_equal(row[exact], exp[exact], equal_nan=True), (name, family, b, row, exp)
        assert np.array_equal(np.isnan(row[angle]), np.isnan(exp[angle])), (name, family, b)
        e_row = max(e_row, float(np.nanmax(np.abs(row[angle] - exp[angle]), initial=0.0)))
        e_rec = max(e_rec, F.oracle_angle_error(oracle, c, b))
    print(f"angle {name}.{family} (D={c.D}): oracle vs float64 per record {e_rec:.3e}, per output row {e_row:.3e}")
    assert e_rec <= 8 * EPS32 * 180 and e_row <= 8 * EPS32 * 180


@pytest.mark.parametrize("name", list(METRICS.cases))
def test_restatement_equals_reference_fixtures(name):
    """the reference's own numbers; these inputs are not exact, so the tolerances are test_metric_classes_vs_reference's"""
    c = METRICS.cases[name]
    mc = metric_case(c)
    got = F.Restated(*metric_inputs(c), mc["size0"], mc["size1"], c["hom"], kp_yx=not mc["xy"]).row(mc["thr"], mc["thr"])
    exp = METRICS[f"{name}.values"]
    assert got.shape == exp.shape
    i = mc["idx"]
    np.testing.assert_allclose(got[i["counts"]], exp[i["counts"]], atol=1e-7, rtol=1e-6)
    np.testing.assert_allclose(got[i["dist"]], exp[i["dist"]], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(got[i["angle"]], exp[i["angle"]], atol=2e-3, rtol=1e-5)


def test_restatement_conventions():
    """(0, 0, 0) when a side keeps nothing, NaN distance / angle when nothing is within t, no Repeatability entry (NaN) when
    neither side keeps a point, MMA 0 without matches"""
    z = np.zeros((0, 3), F32)
    k = np.array([[1.0, 1.0, 0.5], [200.0, 200.0, 0.5]], F32)
    d = F.exact_unit(1, 2, 32)
    far = np.array([[30.0, 30.0, 0.5]], F32)
    R = F.Restated(k, far, d, d[:1], z, z, (40, 56), (40, 56))
    assert (R.N1, R.N2) == (1, 1) and np.array_equal(R.keep0, [True, False])
    row = R.row((3,), (1,))
    assert row[0] == 0 and row[1] == 0 and row[2] == 0 and np.isnan(row[3]) and np.isnan(row[4])
    out = F.Restated(k[1:], far, d[:1], d[:1], z, z, (40, 56), (40, 56))
    assert np.array_equal(out.row((), (1,)), [0, 0, 0, 0]) and np.isinf(out.near_d[1]).all()
    none = F.Restated(k[1:], k[1:], d[:1], d[:1], z, z, (40, 56), (40, 56))
    assert np.isnan(none.row((), (1,), rep_nan_if_empty=True)[1]) and none.row((), (1,))[1] == 0
    assert F.Restated(k, far, d, d[:1], k[:1], far, (40, 56), (40, 56)).row((3,), ())[0] == 1 / (1 + 1e-8)


def test_homographies_invert_exactly():
    """all entries dyadic, determinant +- a power of two, bottom row (0, 0, c): the float64 inverse the restatement takes IS the
    adjugate over the determinant, and so is the fp32 cofactor inverse"""
    homs = {tuple(c.hom[b].reshape(-1).tolist()) for _, c, b in _all_pairs() if c.hom is not None}
    homs |= {tuple(F.homography(k).reshape(-1).tolist()) for k in F.HOM_KINDS}
    assert len(homs) >= 70
    assert tuple(F.homography("c2").reshape(-1).tolist()) == (2, 0, 4, 0, 2, -6, 0, 0, 2)
    dets = set()
    for h in homs:
        H = np.array(h, np.float64).reshape(3, 3)
        inv, det = F.adjugate_inverse(H)
        assert math.frexp(abs(det))[0] == 0.5 and H[2, 0] == 0 and H[2, 1] == 0 and H[2, 2] in (1, 2)
        assert np.array_equal(H * 4, np.round(H * 4))
        assert np.array_equal(np.linalg.inv(H), inv), H
        inv32, _ = F.adjugate_inverse(H.astype(F32))
        assert inv32.dtype == F32 and np.array_equal(inv32.astype(np.float64), inv)
        assert np.array_equal(inv @ H, np.eye(3))
        dets.add(det)
    assert {1.0, -1.0, 4.0, 0.25, 8.0} <= dets


def _warp32(h, x, y):
    """the warp, one fp32 operation after the other"""
    a = h[0, 0] * x + h[0, 1] * y + h[0, 2]
    b = h[1, 0] * x + h[1, 1] * y + h[1, 2]
    w = h[2, 0] * x + h[2, 1] * y + h[2, 2]
    assert a.dtype == F32 and w.dtype == F32
    return a / w, b / w


def test_fp32_evaluation_is_exact_for_every_gpu_case():
    """the claim test_metrics_f64_gpu.py relies on: on its inputs plain fp32 arithmetic gives the float64 warp, visibility,
    squared distances and descriptor sums bit for bit; fp32 square roots keep apart what float64 keeps apart; every threshold
    decision falls the same way; and the double-precision sum of the selected fp32 distances does not depend on its order"""
    seen = 0
    for tag, c, b in _all_pairs():
        R = c.pairs[b]
        k0, k1, d0, d1, mk0, mk1 = (c.k0[b, :c.n[b]], c.k1[b, :c.m[b]], c.d0[b, :c.n[b]], c.d1[b, :c.m[b]], c.mk0[b, :c.nm[b]],
                                    c.mk1[b, :c.nm[b]])
        for a in (k0, k1, d0, d1, mk0, mk1):
            assert a.dtype == F32 and not np.isnan(a).any(), tag
        assert np.array_equal(k0[:, :2] * 2, np.round(k0[:, :2] * 2)) and np.array_equal(k1[:, :2] * 2, np.round(k1[:, :2] * 2)), tag
        xi, yi = (1, 0) if c.kp_yx else (0, 1)
        h = np.eye(3, dtype=F32) if c.hom is None else c.hom[b]
        assert h.dtype == F32 and np.array_equal(h.astype(np.float64), R.H), tag
        hi, _ = F.adjugate_inverse(h)
        # the warp of image 0 and both visibility tests
        wx, wy = _warp32(h, k0[:, xi], k0[:, yi])
        assert np.array_equal(np.stack([wx, wy], 1).astype(np.float64), R.warped0), tag
        assert np.array_equal((wx >= 0) & (wx < F32(c.size1[1])) & (wy >= 0) & (wy < F32(c.size1[0])), R.keep0), tag
        ix, iy = _warp32(hi, k1[:, xi], k1[:, yi])
        back = F.warp(k1[:, [xi, yi]].astype(np.float64).T, R.Hinv)
        assert np.array_equal(np.stack([ix, iy]).astype(np.float64), back), tag
        assert np.array_equal((ix >= 0) & (ix < F32(c.size0[1])) & (iy >= 0) & (iy < F32(c.size0[0])), R.keep1), tag
        # squared distances over the kept points, their fp32 square roots, the threshold decisions
        ax, ay = wx[R.keep0], wy[R.keep0]
        bx, by = k1[R.keep1, xi], k1[R.keep1, yi]
        dx, dy = ax[:, None] - bx[None, :], ay[:, None] - by[None, :]
        sq32 = dx * dx + dy * dy
        assert sq32.dtype == F32 and np.array_equal(sq32.astype(np.float64), R.norm_sq), tag
        root32 = np.sqrt(sq32)
        for axis in (0, 1):
            order = np.argsort(R.norm_sq, axis=axis, kind="stable")
            s, q = np.take_along_axis(R.norm_sq, order, axis), np.take_along_axis(root32, order, axis)
            assert ((np.diff(s, axis=axis) > 0) == (np.diff(q, axis=axis) > 0)).all(), (tag, "an fp32 tie float64 does not see")
        for t in F.THRESHOLDS:
            assert np.array_equal(root32 <= F32(t), R.norm <= t), (tag, t)
        # matches
        mx, my = _warp32(h, mk0[:, xi], mk0[:, yi])
        ex, ey = mx - mk1[:, xi], my - mk1[:, yi]
        m32 = np.sqrt(ex * ex + ey * ey)
        assert m32.dtype == F32 and np.array_equal(m32, R.mma_d.astype(F32)), tag
        for t in F.THRESHOLDS:
            assert np.array_equal(m32 <= F32(t), R.mma_d <= t), (tag, t)
        # descriptor sums of every record
        for s, (idx, v1, v2) in enumerate(F.record_pairs(c, b)):
            if not len(idx):
                continue
            seen += len(idx)
            w1, w2 = v1.astype(np.float64), v2.astype(np.float64)
            df = v1 - v2
            sums32 = [(df * df).sum(1), (v1 * v2).sum(1), (v1 * v1).sum(1), (v2 * v2).sum(1)]
            sums64 = [((w1 - w2) ** 2).sum(1), (w1 * w2).sum(1), (w1 * w1).sum(1), (w2 * w2).sum(1)]
            for a32, a64 in zip(sums32, sums64):
                assert a32.dtype == F32 and np.array_equal(a32.astype(np.float64), a64), tag
            assert np.array_equal(sums64[0], R.desc_sq[s][idx]), tag
            # every partial sum too, in any order: all terms are multiples of 1/64 and their magnitudes sum to less than 2^24 / 64
            for terms in ((w1 - w2) ** 2, w1 * w2, w1 * w1, w2 * w2):
                assert np.array_equal(terms * 64, np.round(terms * 64)) and np.abs(terms).sum(1).max() * 64 < 2 ** 24, tag
            q = sums32[1] / (np.sqrt(sums32[2]) * np.sqrt(sums32[3]))
            assert q.dtype == F32 and (np.abs(q) <= 1).all(), (tag, "the quotient rounds above 1: NaN angle")
            if c.family == "unit":
                assert np.array_equal(sums64[2], np.ones(len(idx))) and np.array_equal(sums64[1] * 16, np.round(sums64[1] * 16)), tag
        # ValidDistance: the double-precision sum of the selected fp32 distances is exact, whatever its order
        for t in F.THRESHOLDS:
            s0, s1 = R.selected(t)
            v = np.concatenate([R.desc_d[0][s0], R.desc_d[1][s1]]).astype(F32).astype(np.float64)
            if len(v):
                fwd, rev = np.cumsum(v)[-1], np.cumsum(v[::-1])[-1]
                assert fwd == rev == v.sum() == math.fsum(v), (tag, t)
    assert seen > 3000


def test_gpu_cases_hold_what_the_gpu_test_needs():
    """the inputs really contain what the cases claim"""
    patterns = {0: set(), 1: set()}
    for tag, c, b in _all_pairs():
        R, info = c.pairs[b], c.info[b]
        mine, theirs = (c.d0[b], c.d1[b]), (c.d1[b], c.d0[b])
        for side, own, first, second, pattern in info["ties"]:
            o = 1 - side
            keep = (R.keep0, R.keep1)
            assert keep[side][own] and keep[o][first] and keep[o][second] and first < second, tag
            P = (R.warped0, c.k1[b, :c.m[b]][:, [1, 0] if c.kp_yx else [0, 1]].astype(np.float64))
            da, db = ((P[side][own] - P[o][first]) ** 2).sum(), ((P[side][own] - P[o][second]) ** 2).sum()
            assert da == db == R.near_sq[side][own] and R.near_j[side][own] == first, (tag, "a planted tie is not the tied minimum")
            sq = lambda j: ((mine[side][own].astype(np.float64) - theirs[side][j]) ** 2).sum()  # noqa: E731
            assert sq(first) != sq(second), (tag, "a wrong choice would not show in the distance record")
            assert second - first == {"slots": 64, "trips": 256, "lanes": 1, "cross": 63}[pattern]
            if pattern == "cross":
                assert first % 64 > second % 64  # the lower lane holds the larger index
            patterns[side].add(pattern)
        for key, table in (("at", F.AT), ("above", F.ABOVE)):
            for side, own, cand, t in info[key]:
                assert R.near_d[side][own] == math.hypot(*table[t]) and R.near_sq[side][own] == sum(v * v for v in table[t]), tag
                assert (R.near_d[side][own] == t) == (key == "at") and R.near_d[side][own] >= t
        for i, j in info["corr"]:
            assert R.near_d[0][i] == 0 and R.near_d[1][j] == 0 and np.array_equal(R.warped0[i], c.k1[b, j][[1, 0] if c.kp_yx else [0, 1]]), tag
            if c.family == "unit":
                assert np.array_equal(c.d0[b, i], c.d1[b, j]) and R.angle[0][i] == 0 and R.desc_d[0][i] == 0, tag
            else:
                assert not np.array_equal(c.d0[b, i], c.d1[b, j]), tag
    assert patterns[0] == patterns[1] == set(F.TIE_PATTERNS)
    nxt = {t: math.hypot(*F.ABOVE[t]) for t in F.THRESHOLDS}
    for t in F.THRESHOLDS:  # nothing on the lattice of halves lies between t and the distance planted just above it
        q = {a * a + b * b for a in range(30) for b in range(30)}
        assert min(v for v in q if v > 4 * t * t) == round(4 * nxt[t] ** 2)
    for name, fam in F.CASE_IDS:
        c = F.build_case(name, fam)
        big = max(c.n) >= 60
        # for every threshold the case uses, some record sits exactly on it and some on the next lattice distance beyond it
        d = np.concatenate([R.near_d[s] for R in c.pairs for s in (0, 1)])
        for t in c.vdd:
            assert (d == t).any() and (d == nxt[t]).any(), (name, fam, t)
        md = np.concatenate([R.mma_d for R in c.pairs])
        if sum(c.nm) >= 100:
            for t in c.mma:
                assert (md == t).any() and (md == nxt[t]).any(), (name, fam, t)
        if big:  # warped coordinates exactly 0, W and H (and W - 1/2) in both directions; sizes that matter
            w = np.concatenate([R.warped0 for R in c.pairs])
            assert (w[:, 0] == 0).any() and (w[:, 0] == c.size1[1]).any() and (w[:, 1] == c.size1[0]).any() and (w[:, 1] == 0).any(), (name, fam)
            xy = [1, 0] if c.kp_yx else [0, 1]
            back = np.concatenate([F.warp(c.k1[b, :c.m[b]][:, xy].astype(np.float64).T, c.pairs[b].Hinv).T for b in range(c.B)])
            assert (back[:, 0] == 0).any() and (back[:, 0] == c.size0[1]).any() and (back[:, 1] == c.size0[0]).any(), (name, fam)
            assert (w[:, 0] == c.size1[1] - 0.5).any() or (back[:, 0] == c.size0[1] - 0.5).any(), (name, fam)
            for b in range(c.B):  # a share outside on every side, before and after the warp
                if c.n[b] >= 60 and c.m[b] >= 60:
                    R = c.pairs[b]
                    assert 0.02 * c.n[b] < R.N1 < 0.98 * c.n[b] and 0.02 * c.m[b] < R.N2 < 0.98 * c.m[b], (name, fam, b)
                    wb = R.warped0
                    assert (wb[:, 0] < 0).any() and (wb[:, 1] < 0).any() and (wb[:, 0] > c.size1[1]).any() and (wb[:, 1] > c.size1[0]).any()
                    bb = F.warp(c.k1[b, :c.m[b]][:, xy].astype(np.float64).T, R.Hinv).T
                    assert (bb[:, 0] < 0).any() and (bb[:, 1] < 0).any() and (bb[:, 0] > c.size0[1]).any() and (bb[:, 1] > c.size0[0]).any()
            swapped = [F.Restated(*c.pair_inputs(b), c.size1, c.size0, None if c.hom is None else c.hom[b], c.kp_yx) for b in range(c.B)]
            assert any(not np.array_equal(S.keep0, R.keep0) or not np.array_equal(S.keep1, R.keep1) for S, R in zip(swapped, c.pairs)), name
    # the trips of the candidate loop
    c = F.build_case("three_trips", "unit")
    j1, j0 = c.pairs[0].near_j[1], c.pairs[0].near_j[0]
    assert (j1 >= 512).any() and ((j1 >= 0) & (j1 < 256)).any() and ((j1 >= 256) & (j1 < 512)).any() and (j0 >= 256).any()
    for fam in F.FAMILIES:
        c = F.build_case("trip_edge", fam)
        assert (c.pairs[0].near_j[0] == 256).any(), "the one candidate of the second trip is nobody's nearest"
        c = F.build_case("matches_beyond_256", fam)
        late = c.pairs[0].mma_d[256:]
        assert c.nm[0] > 256 >= c.n[0] and all((late == t).any() and (late == nxt[t]).any() for t in c.mma)
        c = F.build_case("many_pairs", fam)
        assert c.B > 64 and len({tuple(h.reshape(-1)) for h in c.hom}) == c.B
        assert (0, 0) in zip(c.n, c.m) and 0 in c.nm and max(c.n) == c.cap0 and len({(n, m) for n, m in zip(c.n, c.m)}) > 20
        c = F.build_case("clamp", fam)
        assert all(a >= t for a, t in zip(c.n_arg + c.m_arg + c.nm_arg, c.n + c.m + c.nm))
        assert max(c.n_arg) > c.cap0 and max(c.m_arg) > c.cap1 and max(c.nm_arg) > c.cap0
        assert all(t == min(a, cap) for a, t, cap in zip(c.n_arg + c.m_arg + c.nm_arg, c.n + c.m + c.nm, [c.cap0] * 2 + [c.cap1] * 2 + [c.cap0] * 2))
    sets = [F.SETTINGS[n] for n in F.CASES]
    assert {len(s["mma"]) for s in sets} == {0, 1, 3, 4} and {len(s["vdd"]) for s in sets} == {0, 1, 2, 4}
    assert {s["kp_yx"] for s in sets} == {True, False} and {s["cols"] for s in sets} == {2, 3}
    assert {t for s in sets for t in s["mma"] + s["vdd"]} == set(F.THRESHOLDS)
    assert F.SETTINGS["d4"]["homs"] is None and F.build_case("d4", "unit").hom is None  # the null pointer
    assert any(np.array_equal(h, np.eye(3)) for n, f in F.CASE_IDS if F.build_case(n, f).hom is not None for h in F.build_case(n, f).hom)
