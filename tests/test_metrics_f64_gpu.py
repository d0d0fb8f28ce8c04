"""GPU tests (-m gpu), component: metrics, against the float64 restatement tests/metrics_f64.py on inputs on which fp32 is exact
(test_metrics_f64_cpu.py::test_fp32_evaluation_is_exact_for_every_gpu_case).  MR, MMA@t, Repeatability@t, ValidDistance@t, the
warp, the visibility masks, every counter, every nearest distance and every descriptor distance are compared with array_equal;
only the angle has a bound, derived in the test from the plain fp32 evaluation's own error.  The cases (metrics_f64.CASES) are
the smallest shapes that reach

  lane_tail           partial slots of metric_nearest_kernel's clamped-address tail (65 / 130 candidates), a single candidate, an
                      empty side
  trip_edge           exactly one full trip of 256 candidates against a second trip of one candidate
  three_trips         a third trip on one side, a second on the other, different capacities
  d4 / d257 / d260 / d600   the channel loop: the shortest, a one-channel and a four-channel tail after a full trip, a third trip
  matches_beyond_256  the second block of metric_mma_kernel's grid; matched rows share image 0's capacity
  clamp               count tensors that say more than the capacities
  many_pairs          70 pairs with ragged counts and a homography each: per-pair counters and `hom[b * 9 + i]`

with exact distance ties on every level of the arg-min, distances exactly on a threshold and on the next lattice distance
beyond it, warped coordinates exactly 0 / W / H, two image sizes, both row conventions, 2- and 3-column matched rows and 0 to 4
thresholds per metric.  Rows past a pair's count hold NaN; every call runs twice and must repeat bit for bit."""
from importlib import import_module

import numpy as np
import pytest
import torch

import metrics_f64 as F
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu
N = pkg.native
NM = import_module(pkg.__name__ + ".core.metrics._native_metrics")
EPS32 = float(np.finfo(np.float32).eps)
ICNT = 16


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _twice(fn):
    """run `fn` (-> dict of numpy arrays) twice; the two results must be bit-equal; returns the first"""
    a, b = fn(), fn()
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{k} differs from run to run"
    return a


def _call(c):
    """-> a function that runs einx_pair_metrics on the case's padded batch"""
    k0, k1, d0, d1, mk0, mk1 = (_t(a) for a in (c.k0, c.k1, c.d0, c.d1, c.mk0, c.mk1))
    n, m, nm = _i32(c.n_arg), _i32(c.m_arg), _i32(c.nm_arg)
    hom = None if c.hom is None else _t(c.hom)
    return lambda: NM.pair_metrics(k0, d0, n, k1, d1, m, mk0, mk1, nm, c.size0, c.size1, homography=hom, mma_thr=c.mma, vdd_thr=c.vdd,
                                   ordering="yx" if c.kp_yx else "xy")


_E_ORC = {}


def _record_bound(oracle, c, b):
    """(e_orc, bound) of one pair's angle records: e_orc is the C oracle's own fp32 error against float64 on the same records (the
    plain fp32 evaluation of the same formula on exactly representable dot, n1, n2), never taken from the kernel; the bound is
    max(4 e_orc, 8 eps32 180): the factor 4 leaves room for another order of the same roundings, the second term keeps the bound
    from collapsing where the oracle happens to be exact (angles of exactly 0, 60, 90 degrees)."""
    key = (c.name, c.family, b)
    if key not in _E_ORC:
        _E_ORC[key] = F.oracle_angle_error(oracle, c, b)
    return _E_ORC[key], max(4 * _E_ORC[key], 8 * EPS32 * 180)


def _assert_row(R, got, exp, mma, vdd, rec_bound, tag):
    """one output row: everything but Angle@t equal (NaN at the same places); Angle@t within the per-record bound plus
    c 2^-52 max|angle| for the double-precision sum of c records (each of the c - 1 additions errs by at most 2^-53 of a partial sum
    no larger than c max|angle|).  Returns the largest angle error."""
    assert got.shape == exp.shape == (1 + len(mma) + 3 * len(vdd),), tag
    worst = 0.0
    for i in range(len(exp)):
        k = i - 1 - len(mma)
        if k < 0 or k % 3 != 2:
            assert np.array_equal(got[i], exp[i], equal_nan=True), (tag, i, got, exp)
            continue
        assert np.isnan(got[i]) == np.isnan(exp[i]), (tag, i, got, exp)
        if np.isnan(exp[i]):
            continue  # both sides keep points, none within t: 0 / 0
        if R.N1 == 0 or R.N2 == 0:
            assert got[i] == 0.0 and exp[i] == 0.0, (tag, i, got, exp)
            continue
        s0, s1 = R.selected(vdd[k // 3])
        ang = np.concatenate([R.angle[0][s0], R.angle[1][s1]])
        err = abs(got[i] - exp[i])
        worst = max(worst, err)
        assert err <= rec_bound + len(ang) * 2.0 ** -52 * np.abs(ang).max(), (tag, i, got[i], exp[i], rec_bound)
    return worst


@pytest.mark.parametrize("name,family", F.CASE_IDS)
def test_output_rows(oracle, name, family):
    """einx_pair_metrics' [B, 1 + n_mma + 3 n_vdd] rows against the restatement"""
    c = F.build_case(name, family)
    rows = _twice(lambda f=_call(c): {"rows": _np(f())})["rows"]
    assert rows.dtype == np.float64 and rows.shape == (c.B, 1 + len(c.mma) + 3 * len(c.vdd))
    worst = bound = 0.0
    for b in range(c.B):
        _, rb = _record_bound(oracle, c, b)
        worst = max(worst, _assert_row(c.pairs[b], rows[b], c.row(b), c.mma, c.vdd, rb, (name, family, b)))
        bound = max(bound, rb)
    print(f"Angle@t {name}.{family}: kernel {worst:.3e}, per-record bound {bound:.3e}")


def _carve(ws, B, cap0, cap1):
    """metrics.hip::carve: tw0 | p1 | keep0 | keep1 | icnt [B][16] | near0 [B,cap0,3] | near1 [B,cap1,3] | 256 bytes of slack, each
    region rounded up to 256 bytes"""
    up = lambda v: (v + 255) & ~255  # noqa: E731
    off, out = 0, {}
    for key, count, dt, shape in (("tw0", B * cap0 * 2, np.float32, (B, cap0, 2)), ("p1", B * cap1 * 2, np.float32, (B, cap1, 2)),
                                  ("keep0", B * cap0, np.uint8, (B, cap0)), ("keep1", B * cap1, np.uint8, (B, cap1)),
                                  ("icnt", B * ICNT, np.int32, (B, ICNT)), ("near0", B * cap0 * 3, np.float32, (B, cap0, 3)),
                                  ("near1", B * cap1 * 3, np.float32, (B, cap1, 3))):
        nbytes = count * np.dtype(dt).itemsize
        out[key] = ws[off:off + nbytes].view(dt).reshape(shape)
        off += up(nbytes)
    assert off + 256 == len(ws)
    return out


@pytest.mark.parametrize("name,family", F.CASE_IDS)
def test_per_keypoint_records(oracle, monkeypatch, name, family):
    """what the kernels leave in the workspace below the counts: the warp, both visibility masks, the counters, and per kept
    keypoint the nearest distance (the fp32 square root of the exact squared distance; +inf where the keypoint is filtered out or
    the other side keeps nothing), the descriptor distance of the pair -- a wrong neighbour among equidistant candidates shows
    here exactly -- and its angle within max(4 e_orc, 8 eps32 180) of float64"""
    c = F.build_case(name, family)
    made = []
    real = N._workspace

    def keep(nbytes, device):
        made.append(real(nbytes, device))
        return made[-1]

    monkeypatch.setattr(N, "_workspace", keep)
    _call(c)()
    assert len(made) == 1
    w = _carve(_np(made[0]), c.B, c.cap0, c.cap1)
    xy = [1, 0] if c.kp_yx else [0, 1]
    e_orc = e_gpu = bound = 0.0
    for b, R in enumerate(c.pairs):
        n, m = c.n[b], c.m[b]
        tag = (name, family, b)
        assert np.array_equal(w["tw0"][b, :n].astype(np.float64), R.warped0), tag
        assert np.array_equal(w["p1"][b, :m], c.k1[b, :m][:, xy]), tag
        assert np.array_equal(w["keep0"][b, :n], R.keep0.astype(np.uint8)) and np.array_equal(w["keep1"][b, :m], R.keep1.astype(np.uint8)), tag
        exp = np.zeros((ICNT,), np.int32)
        exp[0], exp[1] = R.N1, R.N2
        for k, t in enumerate(c.mma):
            exp[10 + k] = (R.mma_d <= t).sum()
        assert np.array_equal(w["icnt"][b], exp), (tag, w["icnt"][b], exp)
        if not c.vdd:
            continue  # the neighbour kernels do not run
        eo, rb = _record_bound(oracle, c, b)
        e_orc, bound = max(e_orc, eo), max(bound, rb)
        for s, near, cnt in ((0, w["near0"][b], n), (1, w["near1"][b], m)):
            with np.errstate(invalid="ignore"):
                d = np.where(R.near_j[s] >= 0, np.float32(np.sqrt(R.near_sq[s])), np.float32(np.inf)).astype(np.float32)
            assert np.array_equal(near[:cnt, 0], d), (tag, s, "nearest distance")
            has = np.isfinite(near[:cnt, 0])
            assert np.array_equal(has, R.near_j[s] >= 0), (tag, s)
            assert np.array_equal(near[:cnt, 1][has], np.float32(np.sqrt(R.desc_sq[s][has]))), (tag, s, "descriptor distance: which neighbour")
            if has.any():
                err = float(np.abs(near[:cnt, 2][has].astype(np.float64) - R.angle[s][has]).max())
                e_gpu = max(e_gpu, err)
                assert err <= rb, (tag, s, err, rb)
        for side, own, first, second, pattern in c.info[b]["ties"]:  # the first of two equidistant candidates, by its descriptor
            near = (w["near0"], w["near1"])[side][b, own]
            v = (c.d0[b, own], c.d1[b, first]) if side == 0 else (c.d0[b, first], c.d1[b, own])
            assert near[1] == np.float32(np.sqrt(((v[0].astype(np.float64) - v[1]) ** 2).sum())), (tag, side, own, first, second, pattern)
    print(f"angle records {name}.{family} (D={c.D}): oracle {e_orc:.3e}, kernel {e_gpu:.3e}, bound {bound:.3e}")


def test_metric_classes_beyond_256_keypoints(oracle):
    """the reference-named classes on one exact pair of 300 x 270 keypoints and 280 matches: both row conventions, 2- and 3-column
    rows, and Repeatability's batch with a pair that keeps nothing on either side"""
    mm = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
    km = import_module(pkg.__name__ + ".core.metrics.keypoints_metrics")
    k0, k1, d0, d1, mk0, mk1, H, _ = F.class_pair()
    assert len(k0) > 256 and len(k1) > 256 and len(mk0) > 256
    R = F.Restated(k0, k1, d0, d1, mk0, mk1, F.SIZE0, F.SIZE1, H, kp_yx=True)
    c = F.Case()
    c.name, c.family, c.pairs, c.d0, c.d1 = "class_pair", "unit", [R], d0[None], d1[None]
    e_orc, rb = _record_bound(oracle, c, 0)
    Ht = _t(H)
    thr = list(F.THRESHOLDS)
    flip = lambda a: np.ascontiguousarray(a[:, [1, 0]])  # noqa: E731
    arr = lambda d, keys: {k: np.array(d[k], np.float64) for k in keys}  # noqa: E731

    # ValidDescriptorsDistance: its "xy" takes (y, x) rows (keypoints_metrics.py:193-198)
    names = [f"VDD_{p}@{t}" for t in thr for p in ("Repeatability", "ValidDistance", "Angle")]
    exp = R.row((), thr)
    worst = 0.0
    for ordering, a, b in (("xy", k0, k1), ("yx", flip(k0), flip(k1)), ("xy", k0[:, :2], k1[:, :2])):
        vdd = km.ValidDescriptorsDistance("VDD", thr, ordering=ordering)
        got = _twice(lambda: arr(vdd.update_one(_t(a), _t(b), _t(d0), _t(d1), F.SIZE0, F.SIZE1, Ht), names))
        row = np.array([exp[0]] + [got[k] for k in names])
        worst = max(worst, _assert_row(R, row, exp, (), thr, rb, ("VDD", ordering, a.shape)))
    print(f"Angle@t class_pair: oracle per record {e_orc:.3e}, kernel per row {worst:.3e}, per-record bound {rb:.3e}")

    # Repeatability: its "yx" takes (y, x) rows; 2-column points
    for t in thr:
        e = R.row((), (t,), rep_nan_if_empty=True)[1]
        for ordering, a, b in (("yx", k0[:, :2], k1[:, :2]), ("xy", flip(k0), flip(k1))):
            rep = km.Repeatability("REP", distance_thresh=t, ordering=ordering)
            got = _twice(lambda: arr(rep.update_one(_t(a), _t(b), F.SIZE0, F.SIZE1, Ht), ["REP"]))
            assert got["REP"] == e, (t, ordering)
    k0b, k1b, d0b, d1b, mk0b, mk1b, Hb, _ = F.class_pair(280, 300, 10, 64)
    Rb = F.Restated(k0b, k1b, d0b, d1b, mk0b, mk1b, F.SIZE0, F.SIZE1, Hb, kp_yx=True)
    gone = k0[:5, :2] + np.float32(1000)
    none = F.Restated(gone, gone, d0[:5], d0[:5], mk0[:0], mk0[:0], F.SIZE0, F.SIZE1, H, kp_yx=True)
    assert none.N1 + none.N2 == 0 and np.isnan(none.row((), (3,), rep_nan_if_empty=True)[1])
    rep = km.Repeatability("REP", distance_thresh=3, ordering="yx")
    assert rep.update_one(_t(gone), _t(gone), F.SIZE0, F.SIZE1, Ht) == {}
    got = _twice(lambda: arr(rep.update_batch([_t(k0[:, :2]), _t(gone), _t(k0b[:, :2])], [_t(k1[:, :2]), _t(gone), _t(k1b[:, :2])], F.SIZE0,
                                              F.SIZE1, [Ht, Ht, _t(Hb)]), ["REP"]))
    ea, eb = (np.float32(r.row((), (3,), rep_nan_if_empty=True)[1]) for r in (R, Rb))
    assert ea != eb and got["REP"] == float((ea + eb) / np.float32(2))  # torch.tensor([a, b]).mean() in fp32

    # MeanMatchingAccuracy: both orderings, 2 and 3 columns; MatchingRatio
    for t in thr:
        e = R.row((t,), ())[1]
        assert 0 < e < 1
        for ordering, a, b in (("yx", mk0, mk1), ("yx", mk0[:, :2], mk1[:, :2]), ("xy", flip(mk0), flip(mk1))):
            mma = mm.MeanMatchingAccuracy("MMA", threshold=t, ordering=ordering)
            got = _twice(lambda: arr(mma.update_one(_t(np.ascontiguousarray(a)), _t(np.ascontiguousarray(b)), Ht), ["MMA"]))
            assert got["MMA"] == e, (t, ordering, a.shape)
    got = _twice(lambda: arr(mm.MatchingRatio("MR").update_one(_t(mk0), _t(mk1), _t(k0), _t(k1)), ["MR"]))
    assert got["MR"] == R.row((), ())[0] == len(mk0) / (min(len(k0), len(k1)) + 1e-8)
