"""GPU tests of the absolute pose (csrc/abs_pose.hip) against the float64 restatement tests/abs_pose_f64.py on the
fixed cases of tests/abs_pose_cases.py, whose bounds tests/test_abs_pose_cpu.py establishes on the restatement alone: the ragged
batch, the minimal solver, the lift, the call contract and the evaluator's keys.  No pair is pinned or exempted."""
from importlib import import_module

import numpy as np
import pytest
import torch

import abs_pose_cases as C
import abs_pose_f64 as A
from gpu_support import DEV, _np, _t, pkg
from helpers import synth, synth_raw_events

pytestmark = pytest.mark.gpu
NM = import_module(pkg.__name__ + ".core.metrics._native_metrics")
absolute_pose, AbsolutePoseEstimation = NM.absolute_pose, import_module(pkg.__name__ + ".core.metrics").AbsolutePoseEstimation
CODES = {v: k for k, v in NM.ABS_POSE_STATUS.items()}
POSE_GATE = 10 * C.REFIT_FLOOR   # device against the restatement on refitted poses (pose_distance)
CLEAN_GATE = 10 * C.CLEAN_WORST  # device against the true pose on the noise-free, outlier-free cases
P3P_GATE = min(10 * C.P3P_WORST, C.P3P_CEILING)
# the RANSAC model itself (refine=False): two routes to the same root of the quartic and two constructions of the pose of a
# root agree to the root's conditioning, which the 24 problems put at P3P_WORST for the worst sample; the same factor of ten
MODEL_GATE = P3P_GATE


def _stack(scenes, cap, cols=3, ordering="yx", nmatch=None, T=True, form="d0"):
    """scene dicts -> the arguments of absolute_pose: (mk0, mk1, nmatch, K0, K1), keywords"""
    B = len(scenes)
    mk0, mk1 = np.zeros((B, cap, cols), np.float32), np.zeros((B, cap, cols), np.float32)
    nm = np.zeros(B, np.int32)
    d0, v0 = np.full((B, cap), np.nan, np.float32), np.zeros((B, cap), np.uint8)
    for b, s in enumerate(scenes):
        a0, a1 = s["kp0"].copy(), s["kp1"].copy()
        if ordering == "xy":
            a0[:, :2], a1[:, :2] = a0[:, 1::-1].copy(), a1[:, 1::-1].copy()
        n = min(len(a0), cap)
        mk0[b, :n], mk1[b, :n], nm[b] = a0[:n, :cols], a1[:n, :cols], len(a0)
        if form == "d0":
            d0[b, :n], v0[b, :n] = s["d0"][:n], s["valid0"][:n]
    if nmatch is not None:
        nm = np.asarray(nmatch, np.int32)
    kw = {"d0": _t(d0), "valid0": _t(v0)} if form == "d0" else {"depth0": _t(np.stack([s["depth0"] for s in scenes]))}
    if T:
        kw["T_0to1"] = _t(np.stack([s["T"] for s in scenes]))
    return (_t(mk0), _t(mk1), _t(nm), _t(np.stack([s["K0"] for s in scenes])), _t(np.stack([s["K1"] for s in scenes]))), kw


def _run(args, kw, **more):
    out = [_np(x) for x in absolute_pose(*args, **kw, **more)]
    torch.cuda.synchronize()
    return out


def _same(x, y, msg=None):
    for a, b in zip(x, y):
        assert np.array_equal(a, b, equal_nan=True), msg


def _row(out, b):
    return [x[b] for x in out]


@pytest.fixture(scope="module")
def batch():
    scenes = [C.pair(i) for i in range(len(C.PAIRS))]
    args, kw = _stack(scenes, C.CAP)
    return scenes, args, kw, _run(args, kw, **C.KW)


def _check_against(ref, got, s, tag, refit=True):
    """one pair's device outputs (R, t, mask, status, rows) against the restatement's result"""
    R, t, mask, status, rows = got
    n = len(s["kp0"])
    if ref["status"] != "ok":
        assert status == CODES[ref["status"]], tag
        assert not mask.any() and not R.any() and not t.any(), tag
        assert np.array_equal(rows, np.array(ref["rows"]), equal_nan=True), tag
        return 0.0
    assert status == 4 * ref["it"][0] + ref["it"][1], (tag, status, ref["it"])
    assert np.array_equal(mask[:n], ref["mask"]) and not mask[n:].any(), tag
    d = C.pose_distance(R, t, ref["R"], ref["t"])
    assert d <= (POSE_GATE if refit else MODEL_GATE), (tag, d)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0, tag
    want = np.array(ref["rows"])
    assert np.abs(rows[[0, 2]] - want[[0, 2]]).max() <= 1e-5, (tag, rows, want)       # degrees
    assert abs(rows[1] - want[1]) <= POSE_GATE * max(1.0, np.abs(ref["t"]).max()) * 2, tag  # |t - t_gt|: two entries' worth
    assert rows[3] == want[3] and rows[4] == want[4], tag
    return d


def test_batch_matches_restatement(batch):
    scenes, _, _, out = batch
    worst = 0.0
    for i, s in enumerate(scenes):
        worst = max(worst, _check_against(C.ref(i), _row(out, i), s, i))
    print(f"worst pose distance from the restatement {worst:.3e} (gate {POSE_GATE:.3e})")


def test_ground_truth(batch):
    scenes, _, _, out = batch
    for i, s in enumerate(scenes):
        rows = out[4][i]
        if C.gt_case(i):
            assert rows[0] <= C.GT_BOUND["R_err"] and rows[1] <= C.GT_BOUND["t_err"], (i, rows)
        if C.clean_case(i):
            d = C.pose_distance(out[0][i], out[1][i], s["T"][:3, :3], s["T"][:3, 3])
            assert d <= CLEAN_GATE, (i, d)


def test_p3p():
    X, f, _, _ = C.p3p_problems()
    R, t, ns = [_np(x) for x in NM.p3p(_t(X), _t(f))]
    worst = 0.0
    for k in range(len(X)):
        sols = A.p3p(X[k], f[k])
        assert ns[k] == len(sols), k
        for j, (Rs, ts) in enumerate(sols):
            res = C.p3p_residual(X[k], f[k], R[k, j], t[k, j])
            worst = max(worst, res)
            assert res <= P3P_GATE, (k, j, res)
            assert np.all((X[k] @ R[k, j].T + t[k, j])[:, 2] > 0)
            assert C.pose_distance(R[k, j], t[k, j], Rs, ts) <= MODEL_GATE * 10, (k, j)  # the same pose in the same place
        assert not R[k, ns[k]:].any() and not t[k, ns[k]:].any()
    print(f"worst device certificate {worst:.3e} (gate {P3P_GATE:.3e})")
    # the guards: collinear points, coincident points, coincident bearings
    line = np.stack([X[0][0], X[0][0] + (X[0][1] - X[0][0]) * 0.5, X[0][1]])
    Xg = np.stack([line, np.repeat(X[0][:1], 3, 0), X[0]])
    fg = np.stack([f[0], f[0], np.stack([f[0][0], f[0][0], f[0][2]])])
    assert not _np(NM.p3p(_t(Xg), _t(fg))[2]).any()


def test_lift_depth_map_equals_sampled_depths():
    scenes = [C.lift_pair(i) for i in range(len(C.LIFT_PAIRS))]
    cap = 96
    args, kw = _stack(scenes, cap, form="map")
    out = _run(args, kw, **C.LIFT_KW)
    for i, s in enumerate(scenes):
        _check_against(C.lift_ref(i), _row(out, i), s, ("lift", i))
    pts = args[0][..., [1, 0]].contiguous()  # (x, y)
    d, valid = NM.geom_sample(pts, kw["depth0"][:, None], depth_rule=True)
    kw2 = {"d0": d.reshape(len(scenes), cap), "valid0": valid.reshape(len(scenes), cap), "T_0to1": kw["T_0to1"]}
    _same(out, _run(args, kw2, **C.LIFT_KW), "depth map against sampled depths")


def test_ordering_xy_and_two_columns(batch):
    scenes, _, _, out = batch
    a, kw = _stack(scenes, C.CAP, ordering="xy")
    _same(_run(a, kw, ordering="xy", **C.KW), out, "xy")
    a, kw = _stack(scenes, C.CAP, cols=2)
    _same(_run(a, kw, **C.KW), out, "two columns")


def test_every_pair_alone_and_reversed_slots(batch):
    scenes, _, _, out = batch
    for i, s in enumerate(scenes):
        a, kw = _stack([s], C.CAP)
        _same(_row(_run(a, kw, **C.KW), 0), _row(out, i), ("alone", i))
    a, kw = _stack(scenes[::-1], C.CAP)
    _same([x[::-1] for x in _run(a, kw, **C.KW)], out, "reversed")


def test_nmatch_past_cap_is_clamped():
    idx = [4, 8, 16]  # 64 matches each at cap 64
    scenes = [C.pair(i) for i in idx]
    a, kw = _stack(scenes, 64)
    out = _run(a, kw, **C.KW)
    a2, kw2 = _stack(scenes, 64, nmatch=[64 + 7] * 3)
    _same(_run(a2, kw2, **C.KW), out, "nmatch = cap + 7")
    for b, i in enumerate(idx):
        _check_against(C.ref(i), _row(out, b), scenes[b], ("cap 64", i))


def test_without_ground_truth(batch):
    scenes, _, _, out = batch
    a, kw = _stack(scenes, C.CAP, T=False)
    got = _run(a, kw, **C.KW)
    _same(got[:4], out[:4], "T_0to1=None")
    ok = out[3] >= 0
    assert np.isnan(got[4][ok, :3]).all() and np.array_equal(got[4][ok, 3:], out[4][ok, 3:])
    assert np.array_equal(got[4][~ok], out[4][~ok], equal_nan=True)  # inf, inf, inf without a pose either way


@pytest.fixture(scope="module")
def tile():
    scenes = [C.pair(C.TILE[b % len(C.TILE)]) for b in range(C.TILE_B)]
    a, kw = _stack(scenes, C.TILE_CAP)
    return scenes, _run(a, kw, **C.TILE_KW)


def test_batch_over_64_pairs(tile):
    scenes, out = tile
    nt = len(C.TILE)
    for e in range(nt):  # every entry alone, then every slot against its entry
        a, kw = _stack([scenes[e]], C.TILE_CAP)
        alone = _row(_run(a, kw, **C.TILE_KW), 0)
        for b in range(e, C.TILE_B, nt):
            _same(_row(out, b), alone, (e, b))
    statuses = {int(out[3][b]) for b in (63, 64, 65, 127, 128, 129)}
    assert len(statuses) >= 3  # different pairs either side of slots 64 and 128


def test_max_iters_inside_a_round_equals_the_long_run(batch):
    scenes, _, _, out = batch
    a, kw = _stack(scenes, C.CAP)
    short, long = _run(a, kw, max_iters=33), _run(a, kw, max_iters=300)
    early = [i for i in range(len(scenes)) if 0 <= long[3][i] < 4 * 33]
    assert len(early) >= 8
    for i in early:
        _same(_row(short, i), _row(long, i), i)
        _same(_row(out, i), _row(long, i), i)
    for i in range(len(scenes)):  # the 33-iteration run against the restatement, whatever iteration it chose
        _check_against(C.ref(i, max_iters=33), _row(short, i), scenes[i], ("33", i))


def test_best_model_on_a_rounds_first_or_last_iteration():
    s = C.boundary_pair()
    for it, seed in C.BOUNDARY_SEEDS.items():
        a, kw = _stack([s], 64)
        out = _run(a, kw, seed=seed, **C.BOUNDARY_KW)
        assert out[3][0] // 4 == it, (it, seed, out[3][0])
        _check_against(C.boundary_ref(seed), _row(out, 0), s, ("boundary", it))


def test_refine_false_returns_the_ransac_model(batch):
    scenes, args, kw, out = batch
    got = _run(args, kw, refine=False, **C.KW)
    assert np.array_equal(got[2], out[2]) and np.array_equal(got[3], out[3])
    for i, s in enumerate(scenes):
        r = C.ref(i)
        if r["status"] != "ok":
            continue
        _check_against(dict(C.ref(i, refine=False)), _row(got, i), s, ("model", i), refit=False)
        # the model is the P3P pose of the sample its iteration drew: it reprojects those three points
        idx, X = A.lift(s["kp0"][:, 1::-1], s["K0"], d0=s["d0"], valid0=s["valid0"])
        f = A.bearings(s["kp1"][idx][:, 1::-1].astype(np.float64), s["K1"])
        tri = A.draw3(A.DEFAULT_SEED, r["it"][0], len(idx))
        assert C.p3p_residual(X[tri], f[tri], got[0][i], got[1][i]) <= P3P_GATE, i


def test_repeat_and_graph_replay(batch):
    _, args, kw, out = batch
    _same(_run(args, kw, **C.KW), out, "repeat")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        absolute_pose(*args, **kw, **C.KW)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = absolute_pose(*args, **kw, **C.KW)
    g.replay()
    torch.cuda.synchronize()
    _same([_np(x) for x in res], out, "graph replay")


def test_metric_class(batch):
    scenes = [C.lift_pair(i) for i in range(len(C.LIFT_PAIRS))]
    m = AbsolutePoseEstimation("APE", ((5, 0.1), (10, 0.5)), ransac_thresh=C.LIFT_KW["thresh"])
    one = m.update_one(_t(scenes[1]["kp0"]), _t(scenes[1]["kp1"]), scenes[1]["K0"], scenes[1]["K1"], scenes[1]["depth0"], scenes[1]["T"])
    want = C.lift_ref(1)["rows"]
    assert abs(one["APE_R_errs"] - want[0]) <= 1e-5 and one["APE_inliers"] == want[3] and one["APE_usable"] == want[4]
    res = m.update_batch([_t(s["kp0"]) for s in scenes], [_t(s["kp1"]) for s in scenes], [s["K0"] for s in scenes], [s["K1"] for s in scenes],
                         [s["depth0"] for s in scenes], [s["T"] for s in scenes])
    rows = np.array([C.lift_ref(i)["rows"] for i in range(len(scenes))])
    exp = AbsolutePoseEstimation.summary(rows, m.thresholds, "APE")
    assert list(res) == list(exp)
    for k in exp:
        assert abs(res[k] - exp[k]) <= 1e-5, k
    assert res["APE@5deg_0.1_ratio"] == 0.75  # three poses within (5 degrees, 0.1), the pair without depth counts 0


def test_evaluator_keys():
    H, W, B, BINS = 260, 346, 2, 5
    model = pkg.EIM(pkg.default_config("SP_MNN", event_channels=BINS), device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=31)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    K = _t(np.tile(np.array([[256.0, 0, W / 2], [0, 256.0, H / 2], [0, 0, 1]], np.float32), (B, 1, 1)))
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, 0, 3] = 1.0 / 8
    pose, depth = (K, K, _t(T)), (_t(np.full((B, H, W), 4.0, np.float32)), _t(np.full((B, H, W), 4.0, np.float32)))
    thr = ((5, 0.1), (10, 0.5))
    plain = pkg.DifferentTimeEvaluator(model, bins=BINS, resolution=(W, H))
    ape = pkg.DifferentTimeEvaluator(model, bins=BINS, resolution=(W, H), abs_pose_thresh=thr)
    direct = []
    for step in range(2):
        evs = [synth_raw_events(dict(seed=830 + 2 * step + b, n=20000, H=H, W=W, bins=BINS, frac=False, pneg=False)) for b in range(B)]
        img = synth.synth_image(96 + step, B, H, W)
        r0, _ = plain.step(evs, _t(img), None, pose=pose, depth=depth)
        r1, (ef, _, _) = ape.step(evs, _t(img), None, pose=pose, depth=depth)
        assert _np(r0).tobytes() == _np(r1).tobytes()
        direct.append(NM.batch_absolute_pose(model._last_match, K, K, depth0=depth[0], T_0to1=pose[2], ordering=ef._batched.ordering)[4])
    ape.step(evs, _t(img), None, pose=pose)  # pose without depth: no row
    plain.step(evs, _t(img), None, pose=pose)
    assert len(ape._abs_pose_rows) == 2 and not plain._abs_pose_rows
    a, b = plain.result(), ape.result()
    new = [k for k in b if k not in a]
    assert new == ["APE_R_errs", "APE_t_errs", "APE_t_angles", "APE_inliers", "APE_usable", "APE@5deg_0.1_ratio", "APE@10deg_0.5_ratio"]
    assert [k for k in b if k in a] == list(a) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)
    want = AbsolutePoseEstimation.summary(torch.cat(direct, 0), thr, "APE")
    assert all(b[k] == want[k] or (b[k] != b[k] and want[k] != want[k]) for k in new)
    assert _np(torch.cat(direct, 0))[:, 4].min() > 0  # constant depth: every match is usable
