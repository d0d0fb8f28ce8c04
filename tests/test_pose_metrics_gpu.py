"""GPU tests (-m gpu), component: the pair metrics under depth + motion (einx_pair_metrics_pose, csrc/metrics.hip)
against the numpy restatement tests/pose_metrics_f64.py on inputs on which fp32 is exact
(test_pose_metrics_cpu.py::test_fp32_evaluation_is_exact).  MR, MMA@t, judged_ratio, Repeatability@t, ValidDistance@t, EPI@t, the
projections, the masks, every counter, every nearest distance and every descriptor distance are compared with array_equal; only
the angle has a bound, the one test_metrics_f64_gpu.py derives from the plain fp32 evaluation's own error.  The cases
(pose_metrics_f64.CASES) are the smallest shapes that reach

  ragged              partial slots of metric_nearest_kernel's tail (65 / 130 candidates), a single candidate, an empty side; (y, x)
                      rows with 3 columns; T_1to0 = NULL
  trip_edge           one full trip of 256 candidates against a second trip of one; (x, y) rows with 2 columns; T_1to0 given; depth
                      maps larger than the images
  past_1024           a pair beyond 1024 keypoints on both sides (caps 1030 x 1040)
  matches_beyond_256  the second block of pose_match_kernel's grid (300 matches)
  d4 / d257           the channel loop's shortest run and its one-channel tail after a full trip (D = 36 and 64 elsewhere)
  unjudged            a pair whose matched rows all sit on holes (MMA NaN, judged_ratio 0), a pair behind the camera (N1 = 0: NaN
                      triple, MR intact), a pair without motion (F = 0: every match passes EPI)
  occlusion_on        the occlusion check on scenes it leaves alone: every consistent point comes back to itself exactly

with 5 % holes under keypoints, under one tap of four and under matched rows, projections exactly on u == 0 / W1 / v == 0 / H1 and a
quarter pixel either side, reprojection errors and neighbour distances exactly on a threshold and on the next lattice distance,
equidistant neighbours, rotations by 0 / 90 / 180 degrees.  Rows past a pair's count hold NaN; every call runs twice and must repeat
bit for bit."""
from importlib import import_module

import numpy as np
import pytest
import torch

import gt_matches_ref as R
import pose_metrics_f64 as F
import test_metrics_f64_gpu as TM
from helpers import synth, synth_raw_events
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu
N = pkg.native
NM = import_module(pkg.__name__ + ".core.metrics._native_metrics")
ICNT, IC_JUDGED, IC_EPI, IC_MMA = 16, 2, 4, 10


def _call(c, depth=True, occ="case", t10="case"):
    """-> a function that runs einx_pair_metrics_pose on the case's padded batch"""
    k0, k1, d0, d1, mk0, mk1 = (_t(a) for a in (c.k0, c.k1, c.d0, c.d1, c.mk0, c.mk1))
    n, m, nm = TM._i32(c.n), TM._i32(c.m), TM._i32(c.nm)
    K0, K1, T01 = _t(c.K0), _t(c.K1), _t(c.T01)
    T10 = (None if c.T10 is None else _t(c.T10)) if t10 == "case" else t10
    dp0, dp1 = (_t(c.depth0), _t(c.depth1)) if depth else (None, None)
    occ = c.occ if occ == "case" else occ
    return lambda: NM.pair_metrics_pose(k0, d0, n, k1, d1, m, mk0, mk1, nm, c.size0, c.size1, K0, K1, T01, T10, dp0, dp1, mma_thr=c.thr,
                                        vdd_thr=c.thr, epi_thr=c.epi, occlusion_th=occ, ordering="yx" if c.kp_yx else "xy")


def _assert_row(R_, got, exp, n_mma, vdd, rec_bound, tag):
    """one output row [MR, MMA.., judged_ratio, (Rep, VD, Angle).., EPI..]: everything but Angle@t equal (NaN at the same places);
    Angle@t within the per-record bound plus c 2^-52 max|angle| for the double-precision sum of c records, as
    test_metrics_f64_gpu._assert_row.  Returns the largest angle error."""
    assert got.shape == exp.shape, tag
    worst = 0.0
    first = 2 + n_mma
    for i in range(len(exp)):
        k = i - first
        if not (0 <= k < 3 * len(vdd) and k % 3 == 2):
            assert np.array_equal(got[i], exp[i], equal_nan=True), (tag, i, got, exp)
            continue
        assert np.isnan(got[i]) == np.isnan(exp[i]), (tag, i, got, exp)
        if np.isnan(exp[i]):
            continue  # nothing could be judged, or nothing within t: 0 / 0
        s0, s1 = R_.selected(vdd[k // 3])
        ang = np.concatenate([R_.angle[0][s0], R_.angle[1][s1]])
        err = abs(got[i] - exp[i])
        worst = max(worst, err)
        assert err <= rec_bound + len(ang) * 2.0 ** -52 * np.abs(ang).max(), (tag, i, got[i], exp[i], rec_bound)
    return worst


def _check_rows(oracle, c, rows, pairs, tag):
    assert rows.dtype == np.float64 and rows.shape == (c.B, 2 + 4 * len(c.thr) + len(c.epi))
    for b in range(c.B):
        _, rb = TM._record_bound(oracle, c, b)
        _assert_row(pairs[b], rows[b], pairs[b].row(c.thr, c.thr, c.epi), len(c.thr), c.thr, rb, (tag, b))


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_output_rows(oracle, name):
    """einx_pair_metrics_pose's [B, 2 + n_mma + 3 n_vdd + n_epi] rows against the restatement; two runs bit-equal"""
    c = F.build_case(name)
    rows = TM._twice(lambda f=_call(c): {"rows": _np(f())})["rows"]
    _check_rows(oracle, c, rows, c.pairs, name)
    if c.T10 is None:  # the inverse given explicitly is the inverse formed in the kernel
        assert _np(_call(c, t10=_t(R.invert_pose_f32(c.T01)))()).tobytes() == rows.tobytes()


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_per_keypoint_records(oracle, monkeypatch, name):
    """what the kernels leave in the workspace (einx_pair_metrics' layout): the projections of the points that count, both keep
    masks, the counters N1 / N2 / judged / EPI@t / MMA@t, and per kept keypoint the nearest distance, the descriptor distance of
    that neighbour -- a wrong one among equidistant candidates shows here -- and its angle; and the bytes behind the workspace"""
    c = F.build_case(name)
    made = []
    real = N._workspace
    GUARD = 4096

    def keep(nbytes, device):
        whole = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
        made.append((whole, nbytes))
        return whole[:nbytes]

    monkeypatch.setattr(N, "_workspace", keep)
    _call(c)()
    monkeypatch.setattr(N, "_workspace", real)
    assert len(made) == 1
    whole, nbytes = made[0]
    whole = _np(whole)
    assert (whole[nbytes:] == 0xA5).all(), "bytes behind the workspace were written"
    w = TM._carve(whole[:nbytes], c.B, c.cap0, c.cap1)
    xy = [1, 0] if c.kp_yx else [0, 1]
    for b, P in enumerate(c.pairs):
        n, m = c.n[b], c.m[b]
        tag = (name, b)
        assert np.array_equal(w["tw0"][b, :n][P.ok0].astype(np.float64), P.warped0[P.ok0]), tag
        assert np.array_equal(w["p1"][b, :m], c.k1[b, :m][:, xy]), tag
        assert np.array_equal(w["keep0"][b, :n], P.keep0.astype(np.uint8)) and np.array_equal(w["keep1"][b, :m], P.keep1.astype(np.uint8)), tag
        exp = np.zeros((ICNT,), np.int32)
        exp[0], exp[1], exp[IC_JUDGED] = P.N1, P.N2, P.judged.sum()
        for k, t in enumerate(c.thr):
            exp[IC_MMA + k] = P.mma_good(t).sum()
        for k, t in enumerate(c.epi):
            exp[IC_EPI + k] = (P.epi <= t).sum()
        assert np.array_equal(w["icnt"][b], exp), (tag, w["icnt"][b], exp)
        _, rb = TM._record_bound(oracle, c, b)
        for s, near, cnt in ((0, w["near0"][b], n), (1, w["near1"][b], m)):
            with np.errstate(invalid="ignore"):
                d = np.where(P.near_j[s] >= 0, np.float32(np.sqrt(P.near_sq[s])), np.float32(np.inf)).astype(np.float32)
            assert np.array_equal(near[:cnt, 0], d), (tag, s, "nearest distance")
            has = P.near_j[s] >= 0
            assert np.array_equal(near[:cnt, 1][has], np.float32(np.sqrt(P.desc_sq[s][has]))), (tag, s, "descriptor distance: which neighbour")
            if has.any():
                assert float(np.abs(near[:cnt, 2][has].astype(np.float64) - P.angle[s][has]).max()) <= rb, (tag, s)


def test_two_layer_scene(oracle):
    """occlusion_th = 1 removes the keypoints and matches hidden behind the foreground strip, occlusion_th = 0 keeps them"""
    c = F.two_layer_case()
    on = TM._twice(lambda f=_call(c): {"rows": _np(f())})["rows"]
    off = _np(_call(c, occ=0.0)())
    none = _np(_call(c, occ=None)())
    _check_rows(oracle, c, on, c.pairs, "two_layer on")
    _check_rows(oracle, c, off, c.pairs_off, "two_layer off")
    assert off.tobytes() == none.tobytes()
    jr = 1 + len(c.thr)
    assert off[0, jr] == 1.0 and on[0, jr] == float(np.float32((~c.hidden_matches).sum()) / np.float32(c.nm[0])) < 1.0
    assert on[0, 0] == off[0, 0] and on[0, -1] == off[0, -1]  # MR and EPI do not look at depth


@pytest.mark.parametrize("name", ["ragged", "matches_beyond_256", "unjudged"])
def test_depth_pointers_null(name):
    """without depth maps only MR and EPI@t are finite, and they are what they are with depth"""
    c = F.build_case(name)
    rows = TM._twice(lambda f=_call(c, depth=False): {"rows": _np(f())})["rows"]
    full = _np(_call(c)())
    e0 = 2 + 4 * len(c.thr)
    assert np.isnan(rows[:, 1:e0]).all()
    assert np.array_equal(rows[:, 0], full[:, 0]) and np.array_equal(rows[:, e0:], full[:, e0:], equal_nan=True)
    for b in range(c.B):
        assert np.array_equal(rows[b], c.restate(b, depth=False).row(c.thr, c.thr, c.epi), equal_nan=True), (name, b)
    assert np.isfinite(rows[:, e0:][np.array(c.nm) > 0]).all() and np.isnan(rows[:, e0:][np.array(c.nm) == 0]).all()


def test_refused_at_the_python_layer():
    c = F.build_case("d4")
    k0, k1, d0, d1, mk0, mk1 = (_t(a) for a in (c.k0, c.k1, c.d0, c.d1, c.mk0, c.mk1))
    args = (k0, d0, TM._i32(c.n), k1, d1, TM._i32(c.m), mk0, mk1, TM._i32(c.nm), c.size0, c.size1, _t(c.K0), _t(c.K1), _t(c.T01))
    with pytest.raises(ValueError, match="both depth maps or neither"):
        NM.pair_metrics_pose(*args, depth0=_t(c.depth0))
    with pytest.raises(ValueError, match="at most 4"):
        NM.pair_metrics_pose(*args, epi_thr=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="bad shape"):
        NM.pair_metrics_pose(*args[:9], (0, 64), c.size1, *args[11:])


# ------------------------------------------------------------------------------------------------ the evaluation harness
@pytest.fixture(scope="module")
def small_batch():
    """an SP+MNN model and one batch of 2 synthetic pairs at 346 x 260 with scene depth and pose"""
    H, W, B, bins = 260, 346, 2, 5
    model = pkg.EIM(pkg.default_config("SP_MNN", event_channels=bins), device=DEV).eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=31)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    evs = [synth_raw_events(dict(seed=700 + b, n=20000, H=H, W=W, bins=bins, frac=False, pneg=False)) for b in range(B)]
    return H, W, B, bins, model, evs, synth.synth_image(90, B, H, W), R.scene(40, B, 4, 4, (H, W), (H, W), f0=256.0, f1=256.0, n_corr=0)


def test_evaluator_reports_the_pose_form(small_batch):
    """result() with reproj_thr=(1, 3), epi_thr=(1, 3) equals the finite-value means of pair_metrics_pose called per pair on
    model._last_match; the rows `step` returns and every other key are what they are with the defaults"""
    H, W, B, bins, model, evs, img, sc = small_batch
    pose = (_t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"]))
    depth = (_t(sc["depth0"]), _t(sc["depth1"]))
    ev = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(W, H), reproj_thr=(1, 3), epi_thr=(1, 3))
    plain = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(W, H))
    rows0, _ = plain.step(evs, _t(img), None, pose=pose, depth=depth)
    rows, (ef, imf, _) = ev.step(evs, _t(img), None, pose=pose, depth=depth)
    assert _np(rows).tobytes() == _np(rows0).tobytes()
    mr, e, i = model._last_match, ef._batched, imf._batched
    per_pair = []
    for b in range(B):
        s = slice(b, b + 1)
        per_pair.append(_np(NM.pair_metrics_pose(e.det.positions[s].contiguous(), e.sparse_desc[s].contiguous(), e.det.counts[s].contiguous(),
                                                 i.det.positions[s].contiguous(), i.sparse_desc[s].contiguous(), i.det.counts[s].contiguous(),
                                                 mr.mk0[s].contiguous(), mr.mk1[s].contiguous(), mr.nmatch[s].contiguous(), e.image_size,
                                                 i.image_size, pose[0][s], pose[1][s], pose[2][s], None, depth[0][s], depth[1][s], mma_thr=(1, 3),
                                                 vdd_thr=(1, 3), epi_thr=(1, 3), ordering=e.ordering))[0])
    per_pair = np.stack(per_pair)
    names = NM.pose_metric_names((1, 3), (1, 3), (1, 3))
    assert per_pair.shape == (B, len(names)) and int(_np(mr.nmatch).min()) > 0
    res, res0 = ev.result(), plain.result()
    new = set(res) - set(res0)
    assert all(np.array_equal(res[k], res0[k], equal_nan=True) for k in res0) and "MR" in res0
    for col, k in enumerate(names[1:], 1):
        fin = per_pair[:, col][np.isfinite(per_pair[:, col])]
        assert (k in new) == (len(fin) > 0), k
        if len(fin):
            np.testing.assert_allclose(res[k], fin.mean(), rtol=1e-12, atol=1e-15)
    assert new <= set(names[1:]) and {"DT_judged_ratio", "EPI@1", "EPI@3"} <= new
    # pose without depth: only the EPI columns; epi_thr alone launches nothing for the depth form
    epi_only = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(W, H), epi_thr=(1, 3))
    epi_only.step(evs, _t(img), None, pose=pose, depth=depth)
    r = epi_only.result()
    assert set(r) - set(res0) == {"EPI@1", "EPI@3"} and r["EPI@1"] == res["EPI@1"] and r["EPI@3"] == res["EPI@3"]
    no_depth = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(W, H), reproj_thr=(1, 3), occlusion_th=1.0)
    no_depth.step(evs, _t(img), None, pose=pose)
    assert set(no_depth.result()) == set(plain.result()) - set(NM.MATCH_PR_NAMES)


def test_evaluator_defaults_are_unchanged(small_batch, monkeypatch):
    """with the defaults nothing is launched for the pose form and result() has the keys it had"""
    H, W, B, bins, model, evs, img, sc = small_batch
    harness = import_module(pkg.__name__ + ".harness")

    def refuse(*a, **k):
        raise AssertionError("batch_metrics_pose called with the defaults")

    monkeypatch.setattr(harness, "batch_metrics_pose", refuse)
    ev = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(W, H))
    ev.step(evs, _t(img), None, pose=(_t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"])), depth=(_t(sc["depth0"]), _t(sc["depth1"])))
    keys = set(ev.result())
    rpe = {k for k in keys if k.startswith("RPE")}
    assert keys == set(ev.names) | rpe | set(NM.MATCH_PR_NAMES) and len(rpe) == 10
    assert not any(k.startswith("DT_") or k.startswith("EPI") for k in keys)
