"""GPU tests (-m gpu), component: ground-truth matches and matcher precision / recall (csrc/gt_matches.hip) against the
reference's fixture (tests/golden/gt_matches.npz) and the numpy restatement (tests/gt_matches_ref.py).

Discrete outputs are compared exactly (the fixture's seeds were searched until every decision of the reference clears its
threshold by 16 of the reference's own noise floors; test_gt_matches_cpu.py asserts the stored margins).  Floats use the fixture's
stored bound = 2 x that floor + 4 ulp of the largest coordinate / depth, through close_and_record.  The dense `reward` of the
full-size case skips the entries the generator lists as closer than 16 floors to a threshold in the reference itself."""
import ctypes
import json
from importlib import import_module

import numpy as np
import pytest
import torch

import gt_matches_ref as R
from helpers import Golden, close_and_record, synth, synth_raw_events
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu

M = import_module(pkg.__name__ + ".core.metrics._native_metrics")
GT = import_module(pkg.__name__ + ".core.geometry.gt_generation")
W = import_module(pkg.__name__ + ".core.geometry.wrappers")
LG = import_module(pkg.__name__ + ".core.modules.matchers.lightglue")
G = Golden("gt_matches")
_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = R.POSE_CASES[name](G.cases[name]["seed"])
    return _SCENES[name]


def _pairs(name):
    sc = _scene(name)
    return [(b, int(sc["n"][b]), int(sc["m"][b]), R.fixture_pair(G, f"{name}.{b}", int(sc["n"][b]), int(sc["m"][b]))) for b in range(len(sc["n"]))]


def _yx(a):
    return a[..., ::-1].copy()  # (ascontiguousarray keeps the negative stride of an empty array)


def _padded(name, extra=0, fill=np.nan):
    """the batch of a pose case in the PairBatch layout, (y, x, score) rows when the case's ordering is "yx"; rows past a pair's
    count (and `extra` more columns of capacity) hold `fill`"""
    c, sc = G.cases[name], _scene(name)
    B, cap0, cap1 = len(sc["n"]), sc["kp0"].shape[1] + extra, sc["kp1"].shape[1] + extra
    kp0, kp1 = np.full((B, cap0, 3), fill, np.float32), np.full((B, cap1, 3), fill, np.float32)
    for b in range(B):
        n, m = int(sc["n"][b]), int(sc["m"][b])
        kp0[b, :n, :2] = _yx(sc["kp0"][b, :n]) if c["ordering"] == "yx" else sc["kp0"][b, :n]
        kp1[b, :m, :2] = _yx(sc["kp1"][b, :m]) if c["ordering"] == "yx" else sc["kp1"][b, :m]
        kp0[b, :n, 2], kp1[b, :m, 2] = 0.5, 0.25
    return c, sc, kp0, kp1


def _reference_stage_a(name, cap0, cap1, fill=np.nan):
    """the fixture's proj_* / visible* (the reference's own stage A) and the restatement's validity, padded like _padded"""
    sc = _scene(name)
    B = len(sc["n"])
    p01, p10 = np.full((B, cap0, 2), fill, np.float32), np.full((B, cap1, 2), fill, np.float32)
    v = {k: np.ones((B, cap), np.uint8) for k, cap in (("visible0", cap0), ("visible1", cap1), ("valid0", cap0), ("valid1", cap1))}
    for b, n, m, exp in _pairs(name):
        if exp is None:
            continue
        pre = R.precomputed_depths(sc, b) if name == "b" else None
        e = R.project(sc, b, np.float32, depths=pre)
        p01[b, :n], p10[b, :m] = exp["proj_0to1"], exp["proj_1to0"]
        v["visible0"][b, :n], v["visible1"][b, :m] = exp["visible0"], exp["visible1"]
        v["valid0"][b, :n], v["valid1"][b, :m] = e["valid0"], e["valid1"]
    return p01, p10, v


def _check_labels(name, got, extra=0):
    """matches / scores / pos0 of a padded batch against the fixture, exactly; rows at or beyond the count are -2 / 0"""
    for b, n, m, exp in _pairs(name):
        m0, m1, pos0 = _np(got["matches0"])[b], _np(got["matches1"])[b], _np(got["pos0"])[b]
        if exp is None:
            e0, e1 = G[f"{name}.{b}.tuple.matches0"], G[f"{name}.{b}.tuple.matches1"]
            assert (pos0[:n] == -1).all()
        else:
            e0, e1 = exp["matches0"], exp["matches1"]
            assert np.array_equal(R.assignment_from_pos0(pos0[:n], m), exp["assignment"]), (name, b)
        assert np.array_equal(m0[:n], e0) and np.array_equal(m1[:m], e1), (name, b)
        assert (m0[n:] == -2).all() and (m1[m:] == -2).all(), (name, b)
        for side, mm in (("0", m0), ("1", m1)):
            assert np.array_equal(_np(got[f"matching_scores{side}"])[b], (mm > -1).astype(np.float32)), (name, b)
    assert got["matches0"].dtype == torch.int64 and got["matching_scores0"].dtype == torch.float32 and got["pos0"].dtype == torch.int32


def _homography_inputs(name):
    c = G.cases[name]
    return c, R.homography_scene(c["seed"], c["B"], c["n"], c["m"])


# ------------------------------------------------------------------------------------------------ stage B alone: bit-exact
@pytest.mark.parametrize("name", ["a", "d"])
def test_label_of_reference_projections_pose_form(name):
    c, sc, kp0, kp1 = _padded(name)
    p01, p10, v = _reference_stage_a(name, kp0.shape[1], kp1.shape[1])
    got = M.gt_label(_t(kp0), _t(kp1), _t(sc["n"]), _t(sc["m"]), _t(p01), _t(p10), _t(v["visible0"]), _t(v["visible1"]), _t(v["valid0"]),
                     _t(v["valid1"]), pos_th=c["pos_th"], neg_th=c["neg_th"], ordering=c["ordering"])
    _check_labels(name, got)


@pytest.mark.parametrize("name", ["c", "c_neg_lt_pos"])
def test_label_of_reference_projections_homography_form(name):
    c, sc = _homography_inputs(name)
    got = M.gt_label(_t(sc["kp0"]), _t(sc["kp1"]), None, None, _t(G[f"{name}.proj_0to1"]), _t(G[f"{name}.proj_1to0"]), pos_th=c["pos_th"],
                     neg_th=c["neg_th"], ordering="xy")
    B, n, m = c["B"], c["n"], c["m"]
    assert np.array_equal(_np(got["matches0"]), G[f"{name}.matches0"]) and np.array_equal(_np(got["matches1"]), G[f"{name}.matches1"])
    assignment = np.unpackbits(G[f"{name}.assignment"])[:B * n * m].reshape(B, n, m).astype(bool)
    for b in range(B):
        assert np.array_equal(R.assignment_from_pos0(_np(got["pos0"])[b], m), assignment[b])


# ------------------------------------------------------------------------------------------------ stage A alone
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_project_against_fixture(name):
    c, sc, kp0, kp1 = _padded(name)
    pre = None
    if name == "b":
        pre = [np.stack(x) for x in zip(*[R.precomputed_depths(sc, b) for b in range(len(sc["n"]))])]
        pre = tuple(_t(np.ascontiguousarray(x)) for x in pre)
    got = M.gt_project(_t(kp0), _t(kp1), _t(sc["n"]), _t(sc["m"]), None if pre else _t(sc["depth0"]), None if pre else _t(sc["depth1"]),
                       _t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"]), _t(sc["T10"]), ordering=c["ordering"], precomputed=pre)
    null = M.gt_project(_t(kp0), _t(kp1), _t(sc["n"]), _t(sc["m"]), None if pre else _t(sc["depth0"]), None if pre else _t(sc["depth1"]),
                        _t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"]), None, ordering=c["ordering"], precomputed=pre)
    inv = M.gt_project(_t(kp0), _t(kp1), _t(sc["n"]), _t(sc["m"]), None if pre else _t(sc["depth0"]), None if pre else _t(sc["depth1"]),
                       _t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"]), _t(R.invert_pose_f32(sc["T01"])), ordering=c["ordering"], precomputed=pre)
    for k in got:  # T_1to0 = NULL equals passing the inverse, bit for bit
        assert np.array_equal(_np(null[k]), _np(inv[k]), equal_nan=True), k
    for b, n, m, exp in _pairs(name):
        e = R.project(sc, b, np.float32, depths=None if pre is None else R.precomputed_depths(sc, b))
        for side, cnt in (("0", n), ("1", m)):
            # rows at or beyond the count: zeros
            for k in (f"depth_keypoints{side}", f"valid{side}", f"visible{side}", "proj_0to1" if side == "0" else "proj_1to0"):
                assert not _np(got[k])[b, cnt:].any(), (name, b, k)
            assert np.array_equal(_np(got[f"valid{side}"])[b, :cnt], e[f"valid{side}"]), (name, b)
        if exp is None:
            continue
        for side, cnt, pk in (("0", n, "proj_0to1"), ("1", m, "proj_1to0")):
            assert np.array_equal(_np(got[f"visible{side}"])[b, :cnt], exp[f"visible{side}"]), (name, b)
            d, p = _np(got[f"depth_keypoints{side}"])[b, :cnt], _np(got[pk])[b, :cnt]
            assert np.array_equal(np.isnan(d), np.isnan(exp[f"depth_keypoints{side}"])) and np.array_equal(np.isnan(p), np.isnan(exp[pk]))
            close_and_record(f"gt_matches.{name}.depth", d, exp[f"depth_keypoints{side}"], atol=c["bounds"]["depth"])
            close_and_record(f"gt_matches.{name}.proj", p, exp[pk], atol=c["bounds"]["proj"])
            # and the kernel follows the written operation order: equal to the float32 restatement bit for bit
            assert np.array_equal(d, e[f"d{side}"], equal_nan=True) and np.array_equal(p, e["proj01" if side == "0" else "proj10"], equal_nan=True)
    assert got["visible0"].dtype == torch.bool and got["proj_0to1"].dtype == torch.float32


@pytest.mark.parametrize("name", ["c", "c_neg_lt_pos"])
def test_warp_against_fixture(name):
    c, sc = _homography_inputs(name)
    got = M.gt_warp(_t(sc["kp0"]), _t(sc["kp1"]), None, None, _t(sc["H"]))
    close_and_record(f"gt_matches.{name}.proj", _np(got["proj_0to1"]), G[f"{name}.proj_0to1"], atol=c["bounds"]["proj"])
    close_and_record(f"gt_matches.{name}.proj", _np(got["proj_1to0"]), G[f"{name}.proj_1to0"], atol=c["bounds"]["proj"])
    for b in range(c["B"]):
        assert np.array_equal(_np(got["proj_0to1"])[b], R.warp(sc["kp0"][b], sc["H"][b]))
        assert np.array_equal(_np(got["proj_1to0"])[b], R.warp(sc["kp1"][b], sc["H"][b], inverse=True))


# ------------------------------------------------------------------------------------------------ A + B, the raw entry
def _gt_matches_batch(name, extra=0, fill=np.nan, T10=True):
    c, sc, kp0, kp1 = _padded(name, extra, fill)
    return M.gt_matches(_t(kp0), _t(kp1), _t(sc["n"]), _t(sc["m"]), _t(sc["depth0"]), _t(sc["depth1"]), _t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"]),
                        _t(sc["T10"]) if T10 else None, pos_th=c["pos_th"], neg_th=c["neg_th"], ordering=c["ordering"])


@pytest.mark.parametrize("name", ["a", "d"])
def test_gt_matches_ragged_batch_counts_determinism(name):
    got = _gt_matches_batch(name)
    _check_labels(name, got)
    again = _gt_matches_batch(name)
    wide = _gt_matches_batch(name, extra=37, fill=7.0)  # cap > count, other garbage past the counts
    sc = _scene(name)
    cap0, cap1 = sc["kp0"].shape[1], sc["kp1"].shape[1]
    pad = {"matches0": -2, "matches1": -2, "pos0": -1}  # what rows past the capacity-filling counts hold; zeros elsewhere
    for k, v in got.items():
        assert np.array_equal(_np(v), _np(again[k]), equal_nan=True), f"two runs differ in {k}"
        cap = cap0 if k in ("proj_0to1", "depth_keypoints0", "valid0", "visible0", "matches0", "matching_scores0", "pos0") else cap1
        assert np.array_equal(_np(v), _np(wide[k])[:, :cap], equal_nan=True), f"cap > count changes {k}"
        assert (_np(wide[k])[:, cap:] == pad.get(k, 0)).all(), k
    null = _gt_matches_batch(name, T10=False)
    c, sc, kp0, kp1 = _padded(name)
    inv = M.gt_matches(_t(kp0), _t(kp1), _t(sc["n"]), _t(sc["m"]), _t(sc["depth0"]), _t(sc["depth1"]), _t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"]),
                       _t(R.invert_pose_f32(sc["T01"])), pos_th=c["pos_th"], neg_th=c["neg_th"], ordering=c["ordering"])
    for k in null:
        assert np.array_equal(_np(null[k]), _np(inv[k]), equal_nan=True), f"T_1to0 = NULL differs from the inverse in {k}"


def test_negative_count_is_an_empty_side():
    """n[b] < 0 on one side only is the early return of an empty pair, not a read of unwritten workspace"""
    c, sc, kp0, kp1 = _padded("a")
    args = lambda n: (_t(kp0), _t(kp1), _t(n), _t(sc["m"]), _t(sc["depth0"]), _t(sc["depth1"]), _t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"]))  # noqa: E731
    zero, neg = sc["n"].copy(), sc["n"].copy()
    zero[0], neg[0] = 0, -3
    a, b = M.gt_matches(*args(zero)), M.gt_matches(*args(neg))
    for k in a:
        assert np.array_equal(_np(a[k]), _np(b[k]), equal_nan=True), k
    m = int(sc["m"][0])
    assert (_np(b["matches1"])[0, :m] == -1).all() and (_np(b["matches0"])[0] == -2).all()
    pr = _np(M.match_pr(b["matches0"], b["matches0"], _t(neg), scores0=b["matching_scores0"]))
    assert np.isnan(pr[0]).all()


def test_graph_capture_and_replay():
    """the raw einx_gt_matches + einx_match_pr calls captured on a side stream, replayed twice into poisoned outputs"""
    name = "a"
    c, sc, kp0, kp1 = _padded(name)
    eager = _gt_matches_batch(name)
    L, N = pkg.native.lib(), pkg.native
    P = N._ptr
    B, cap0, cap1 = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    p = M._gt_params(_t(kp0), _t(kp1), c["ordering"], c["pos_th"], c["neg_th"], False, sc["depth0"].shape[1:], sc["depth1"].shape[1:])
    t = {k: _t(v) for k, v in dict(kp0=kp0, kp1=kp1, n=sc["n"], m=sc["m"], d0=sc["depth0"], d1=sc["depth1"], K0=sc["K0"], K1=sc["K1"],
                                   T01=sc["T01"], T10=sc["T10"]).items()}
    o = M._gt_stage_a_outputs(B, cap0, cap1, DEV)
    o.update(M._gt_label_outputs(B, cap0, cap1, DEV))
    ws = torch.empty(L.einx_gt_matches_ws_bytes(ctypes.byref(p)), dtype=torch.uint8, device=DEV)
    pred = torch.from_numpy(R.ints(5, (B, cap0), cap1 + 1) - 1).to(DEV)
    score = torch.from_numpy(R.ints(6, (B, cap0), 1000).astype(np.float32)).to(DEV)
    pr = torch.empty((B, 4), dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        rc = L.einx_gt_matches(ctypes.byref(p), P(t["kp0"]), P(t["kp1"]), P(t["n"]), P(t["m"]), P(t["d0"]), P(t["d1"]), P(t["K0"]), P(t["K1"]),
                               P(t["T01"]), P(t["T10"]), None, None, None, None, None, P(ws), P(o["depth_keypoints0"]), P(o["depth_keypoints1"]),
                               P(o["valid0"]), P(o["valid1"]), P(o["proj_0to1"]), P(o["proj_1to0"]), P(o["visible0"]), P(o["visible1"]),
                               P(o["matches0"]), P(o["matches1"]), P(o["matching_scores0"]), P(o["matching_scores1"]), P(o["pos0"]), N._stream(pr))
        rc2 = L.einx_match_pr(P(pred), P(score), P(o["matches0"]), P(t["n"]), B, cap0, P(pr), N._stream(pr))
    assert rc == 0 and rc2 == 0
    expect_pr = _np(M.match_pr(pred, eager["matches0"], t["n"], scores0=score))
    for _ in range(2):
        for v in o.values():
            v.fill_(0x55 if v.dtype != torch.float32 else float("nan"))
        ws.fill_(0xAB)
        pr.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for k, v in eager.items():
            assert np.array_equal(_np(o[k]).astype(_np(v).dtype), _np(v), equal_nan=True), k
        assert np.array_equal(_np(pr), expect_pr, equal_nan=True)
    assert np.isnan(expect_pr[2]).all() and np.isfinite(expect_pr[:2]).all()  # pair 2 has no row


def test_bad_arguments_are_refused():
    L, N = pkg.native.lib(), pkg.native
    c, sc, kp0, kp1 = _padded("a")
    k0, k1 = _t(kp0), _t(kp1)
    p = M._gt_params(k0, k1, "yx", 3, 5)
    out = torch.zeros((3, 90, 2), device=DEV)
    H = _t(np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (3, 1)))
    n, m = _t(sc["n"]), _t(sc["m"])
    call = lambda q: L.einx_gt_warp(ctypes.byref(q), N._ptr(k0), N._ptr(k1), N._ptr(n), N._ptr(m), N._ptr(H), N._ptr(out), N._ptr(out), N._stream(out))  # noqa: E731
    p.struct_size -= 4
    assert call(p) == -1  # EINX_ERR_ARG: a struct of another size
    p.struct_size += 4
    p.cols0 = 1
    assert call(p) == -1
    p.cols0 = 3
    assert L.einx_gt_warp(ctypes.byref(p), N._ptr(k0), N._ptr(k1), N._ptr(n), N._ptr(m), None, N._ptr(out), N._ptr(out), N._stream(out)) == -1
    assert L.einx_match_pr(None, None, None, None, 1, 1, None, None) == -1
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        M.gt_matches(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2), homography=torch.eye(3))  # CPU tensors: there is no CPU path


# ------------------------------------------------------------------------------------------------ the drop-in functions
POSE_KEYS = ["assignment", "reward", "matches0", "matches1", "matching_scores0", "matching_scores1", "depth_keypoints0", "depth_keypoints1",
             "proj_0to1", "proj_1to0", "visible0", "visible1"]


def _check_dict(tag, r, exp, dtypes, bounds, n, m):
    assert list(r.keys()) == list(dtypes.keys()), (list(r.keys()), list(dtypes.keys()))
    for k, dt in dtypes.items():
        assert str(r[k].dtype) == "torch." + dt, (k, r[k].dtype, dt)
    for k in ("matches0", "matches1", "visible0", "visible1"):
        if k in exp:
            assert np.array_equal(_np(r[k])[0], exp[k]), (tag, k)
    for side in "01":
        assert np.array_equal(_np(r[f"matching_scores{side}"])[0], (exp[f"matches{side}"] > -1).astype(np.float32))
    assert np.array_equal(_np(r["assignment"])[0], exp["assignment"]) and tuple(r["assignment"].shape) == (1, n, m)
    sure = np.ones(n * m, bool)
    sure[exp.get("reward_unsure", np.zeros(0, np.int64))] = False
    assert np.array_equal(_np(r["reward"])[0].reshape(-1)[sure], exp["reward"].reshape(-1)[sure]) and tuple(r["reward"].shape) == (1, n, m)
    for k in ("depth_keypoints0", "depth_keypoints1", "proj_0to1", "proj_1to0"):
        if k in exp:
            got = _np(r[k])[0]
            assert np.array_equal(np.isnan(got), np.isnan(exp[k])), (tag, k)
            close_and_record(f"gt_matches.{tag}.{'depth' if k.startswith('depth') else 'proj'}", got, exp[k],
                             atol=bounds["depth" if k.startswith("depth") else "proj"])


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_gt_matches_from_pose_depth(name):
    c, sc = G.cases[name], _scene(name)
    for b, n, m, exp in _pairs(name):
        kp0, kp1 = sc["kp0"][b:b + 1, :n], sc["kp1"][b:b + 1, :m]
        if c["ordering"] == "yx":
            kp0, kp1 = _yx(kp0), _yx(kp1)
        cam0, cam1 = W.Camera.from_calibration_matrix(_t(sc["K0"][b:b + 1])), W.Camera.from_calibration_matrix(_t(sc["K1"][b:b + 1]))
        T01, T10 = W.Pose.from_4x4mat(_t(sc["T01"][b:b + 1])), W.Pose.from_4x4mat(_t(sc["T10"][b:b + 1]))
        kw = {}
        if name == "b":
            d0, v0, d1, v1 = R.precomputed_depths(sc, b)
            kw = dict(depth_keypoints0=_t(d0)[None], valid_depth_keypoints0=_t(v0)[None], depth_keypoints1=_t(d1)[None],
                      valid_depth_keypoints1=_t(v1)[None])
        r = GT.gt_matches_from_pose_depth(_t(kp0), _t(kp1), cam0, cam1, _t(sc["depth0"][b:b + 1]), _t(sc["depth1"][b:b + 1]), T01, T10,
                                          pos_th=c["pos_th"], neg_th=c["neg_th"], ordering=c["ordering"], **kw)
        if exp is None:  # the reference's empty-input tuple
            assert isinstance(r, tuple) and len(r) == 3 and r[0].dtype == torch.bool and tuple(r[0].shape) == (1, n, m)
            assert np.array_equal(_np(r[1])[0], G[f"{name}.{b}.tuple.matches0"]) and np.array_equal(_np(r[2])[0], G[f"{name}.{b}.tuple.matches1"])
            assert r[1].dtype == torch.int64 and r[2].dtype == torch.int64
            continue
        dtypes = json.loads(bytes(G[f"{name}.{b}.dtypes"]).decode())
        assert list(dtypes) == POSE_KEYS
        _check_dict(f"{name}", r, exp, dtypes, c["bounds"], n, m)
        if name == "a" and b == 0:  # T_1to0 = None: the kernel's inverse; K / T tensors instead of the holders
            r2 = GT.gt_matches_from_pose_depth(_t(kp0), _t(kp1), _t(sc["K0"][b:b + 1]), _t(sc["K1"][b:b + 1]), _t(sc["depth0"][b:b + 1]),
                                               _t(sc["depth1"][b:b + 1]), _t(sc["T01"][b:b + 1]), None)
            assert np.array_equal(_np(r2["matches0"]), _np(r["matches0"])) and np.array_equal(_np(r2["matches1"]), _np(r["matches1"]))


@pytest.mark.parametrize("name", ["c", "c_neg_lt_pos"])
def test_gt_matches_from_homography(name):
    c, sc = _homography_inputs(name)
    B, n, m = c["B"], c["n"], c["m"]
    r = GT.gt_matches_from_homography(_t(sc["kp0"]), _t(sc["kp1"]), _t(sc["H"]).reshape(B, 3, 3), pos_th=c["pos_th"], neg_th=c["neg_th"])
    dtypes = json.loads(bytes(G[f"{name}.dtypes"]).decode())
    assert list(r.keys()) == list(dtypes) and len(dtypes) == 8
    for k, dt in dtypes.items():
        assert str(r[k].dtype) == "torch." + dt, (k, r[k].dtype, dt)
        shapes = {"assignment": (B, n, m), "reward": (B, n, m), "proj_0to1": (B, n, 2), "proj_1to0": (B, m, 2)}
        assert tuple(r[k].shape) == shapes.get(k, (B, n) if k.endswith("0") else (B, m)), k
    assert np.array_equal(_np(r["matches0"]), G[f"{name}.matches0"]) and np.array_equal(_np(r["matches1"]), G[f"{name}.matches1"])
    assert np.array_equal(_np(r["assignment"]), np.unpackbits(G[f"{name}.assignment"])[:B * n * m].reshape(B, n, m).astype(bool))
    assert np.array_equal(_np(r["reward"]), G[f"{name}.reward"].astype(np.float32))
    for side in "01":
        assert np.array_equal(_np(r[f"matching_scores{side}"]), (G[f"{name}.matches{side}"] > -1).astype(np.float32))
    close_and_record(f"gt_matches.{name}.proj", _np(r["proj_0to1"]), G[f"{name}.proj_0to1"], atol=c["bounds"]["proj"])
    close_and_record(f"gt_matches.{name}.proj", _np(r["proj_1to0"]), G[f"{name}.proj_1to0"], atol=c["bounds"]["proj"])
    one = GT.gt_matches_from_homography(_t(sc["kp0"][:1]), _t(sc["kp1"][:1]), _t(sc["H"][0]))  # an un-batched [3,3] homography, defaults 3 / 6
    if (c["pos_th"], c["neg_th"]) == (3, 6):
        assert np.array_equal(_np(one["matches0"])[0], G[f"{name}.matches0"][0])


def test_empty_input_tuple_on_the_device():
    kp0, kp1 = torch.zeros(2, 0, 2, device=DEV), torch.zeros(2, 5, 2, device=DEV)
    for r in (GT.gt_matches_from_homography(kp0, kp1, torch.eye(3, device=DEV)[None].repeat(2, 1, 1)),
              GT.gt_matches_from_pose_depth(kp1, kp0, None, None, None, None, None, None)):
        assert isinstance(r, tuple) and r[0].dtype == torch.bool and r[0].device.type == "cuda" and not r[0].any()
        assert (r[1] == -1).all() and (r[2] == -1).all() and r[1].dtype == torch.int64


# ------------------------------------------------------------------------------------------------ stage C
def test_match_pr_and_matcher_metrics_against_fixture():
    for name, (m, gt, sc) in R.pr_cases().items():
        exp = G[f"pr.{name}"]
        rows = _np(M.match_pr(_t(m), _t(gt), scores0=_t(sc)))
        assert rows.dtype == np.float64 and rows.shape == exp.shape
        close_and_record("gt_matches.match_pr", rows, exp, atol=1e-4)
        assert np.array_equal(rows, np.stack([R.match_pr(m[b], gt[b], sc[b]) for b in range(len(m))]))  # integer counts, one float64 division
        r = LG.matcher_metrics({"matches0": _t(m), "matching_scores0": _t(sc)}, {"gt_matches0": _t(gt)})
        assert list(r) == ["match_recall", "match_precision", "accuracy", "average_precision"]
        for i, k in enumerate(r):
            assert r[k].dtype == torch.float32 and tuple(r[k].shape) == (len(m),)
            close_and_record("gt_matches.matcher_metrics", _np(r[k]), exp[:, i], atol=1e-4)
        r = LG.matcher_metrics({"x_matches0": _t(m), "x_matching_scores0": _t(sc)}, {"gt_y_matches0": _t(gt)}, prefix="x_", prefix_gt="y_")
        assert list(r) == ["x_match_recall", "x_match_precision", "x_accuracy", "x_average_precision"]
    # counts: rows at or beyond n[b] are not read; a tie at the top goes to the lowest index
    m, gt, sc = R.pr_cases()["mixed"]
    n = np.array([300, 120, 1, 0], np.int32)
    rows = _np(M.match_pr(_t(m), _t(gt), _t(n), scores0=_t(sc)))
    for b in range(4):
        assert np.array_equal(rows[b], R.match_pr(m[b, :n[b]], gt[b, :n[b]], sc[b, :n[b]]), equal_nan=True)
    assert np.isnan(rows[3]).all()
    sc2 = sc.copy()
    sc2[0, 5] = sc2[0, 200] = 0.9
    assert np.array_equal(_np(M.match_pr(_t(m), _t(gt), scores0=_t(sc2)))[0], R.match_pr(m[0], gt[0], sc2[0]))
    mr = pkg.native.MatchResult()  # the matcher's own result object: its matches0 / scores0 are taken
    mr.matches0, mr.scores0 = _t(m), _t(sc)
    assert np.array_equal(_np(M.match_pr(mr, _t(gt))), _np(M.match_pr(_t(m), _t(gt), scores0=_t(sc))))
    with pytest.raises(ValueError):
        M.match_pr(_t(m), _t(gt))


# ------------------------------------------------------------------------------------------------ the evaluation harness
@pytest.fixture(scope="module")
def depth_batches():
    """an SP+MNN model and two batches of 4 synthetic pairs at 346 x 260 with scene depth and pose: (H, W, B, bins, model, batches)"""
    H, Wd, B, bins = 260, 346, 4, 5
    cfg = pkg.default_config("SP_MNN", event_channels=bins)
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=31)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    batches = []
    for k in range(2):
        evs = [synth_raw_events(dict(seed=700 + 10 * k + b, n=20000, H=H, W=Wd, bins=bins, frac=False, pneg=False)) for b in range(B)]
        img = synth.synth_image(90 + k, B, H, Wd)
        sc = R.scene(40 + k, B, 4, 4, (H, Wd), (H, Wd), f0=256.0, f1=256.0, n_corr=0)
        batches.append((evs, img, sc))
    return H, Wd, B, bins, model, batches


def test_different_time_evaluator_with_depth(depth_batches):
    """the batches of `depth_batches`: the result() means equal the mean of matcher_metrics(restatement labels) over the same pairs;
    the returned rows are byte-equal to a run without depth"""
    H, Wd, B, bins, model, batches = depth_batches
    with_depth = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, H))
    without = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, H))
    assert with_depth.last_gt is None
    expect, positives = [], 0
    for evs, img, sc in batches:
        pose = (_t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"]))
        rows, (ef, imf, matches) = with_depth.step(evs, _t(img), None, pose=pose, depth=(_t(sc["depth0"]), _t(sc["depth1"])))
        rows0, _ = without.step(evs, _t(img), None, pose=pose)
        assert _np(rows).tobytes() == _np(rows0).tobytes()
        gt, mr = with_depth.last_gt, model._last_match
        n, m = _np(ef._batched.det.counts), _np(imf._batched.det.counts)
        k0, k1 = _np(ef._batched.det.positions), _np(imf._batched.det.positions)
        assert ef._batched.ordering == "yx"
        for b in range(B):
            one = dict(sc, kp0=_yx(k0[b:b + 1, :n[b], :2]), kp1=_yx(k1[b:b + 1, :m[b], :2]), n=n[b:b + 1], m=m[b:b + 1],
                       **{k: sc[k][b:b + 1] for k in ("depth0", "depth1", "K0", "K1", "T01")}, T10=R.invert_pose_f32(sc["T01"][b:b + 1]))
            e = R.project(one, 0, np.float32)
            m0, m1, _ = R.label(one["kp0"][0], one["kp1"][0], e["proj01"], e["proj10"], e["visible0"], e["visible1"], e["valid0"], e["valid1"], 3, 5)
            assert np.array_equal(_np(gt["matches0"])[b, :n[b]], m0) and np.array_equal(_np(gt["matches1"])[b, :m[b]], m1)
            expect.append(R.match_pr(_np(mr.matches0)[b, :n[b]], m0, _np(mr.scores0)[b, :n[b]]))
        assert n.min() > 0 and m.min() > 0
        positives += int((_np(gt["matches0"]) > -1).sum())
    assert positives > 0  # the labels are not all "unmatched / ignore": precision and recall measure something
    res, res0 = with_depth.result(), without.result()
    expect = np.stack(expect)
    for i, k in enumerate(("match_recall", "match_precision", "accuracy", "average_precision")):
        assert k not in res0
        np.testing.assert_allclose(res[k], np.nanmean(expect[:, i]), rtol=1e-12, atol=1e-15)
    assert all(np.array_equal(res[k], res0[k], equal_nan=True) for k in res0)  # every other key is what it was without depth
    with pytest.raises(ValueError, match="pose"):
        with_depth.step(batches[0][0], _t(batches[0][1]), None, depth=(_t(batches[0][2]["depth0"]), _t(batches[0][2]["depth1"])))
    # run(): depth as a further element of an item
    runner = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, H))
    items = [(evs, _t(img), None, (_t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"])), (_t(sc["depth0"]), _t(sc["depth1"]))) for evs, img, sc in batches]
    for _ in runner.run(items):
        pass
    with pytest.raises(ValueError, match="takes no depth"):  # the same-time loop does not swallow a depth element
        list(pkg.SameTimeEvaluator(model, bins=bins, resolution=(Wd, H)).run(items[:1]))
    res_run = runner.result()
    for k in ("match_recall", "match_precision", "accuracy", "average_precision"):
        assert res_run[k] == res[k]


def test_different_time_evaluator_with_homography_pose_and_depth_at_once(depth_batches):
    """every feature of the evaluator in one batch -- a per-pair homography with he_thresh, pose and depth: `step` and `run` give
    the same result() key for key, each key a single-feature evaluator reports has the combined evaluator's value, and the
    returned rows are byte-equal across all of them (everything is seeded and deterministic)"""
    H, Wd, B, bins, model, batches = depth_batches
    hom = _t(np.tile(np.array([[1.01, 0.01, -2.0], [-0.01, 0.99, 1.5], [1e-5, -1e-5, 1.0]], np.float32), (B, 1, 1)))
    make = lambda **kw: pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, H), **kw)  # noqa: E731
    same = lambda a, b: a == b or (a != a and b != b)  # noqa: E731
    full = [(evs, img, (_t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"])), (_t(sc["depth0"]), _t(sc["depth1"]))) for evs, img, sc in batches]
    stepped, streamed = make(he_thresh=(3, 5, 10)), make(he_thresh=(3, 5, 10))
    singles = {"homography": (make(he_thresh=(3, 5, 10)), False, False), "pose": (make(), True, False), "depth": (make(), True, True)}
    rows = [stepped.step(evs, _t(img), hom, pose=pose, depth=depth)[0] for evs, img, pose, depth in full]
    rows_run = [r for r, _ in streamed.run([(evs, _t(img), hom, pose, depth) for evs, img, pose, depth in full], depth=2)]
    assert len(rows_run) == len(rows) == 2
    for r0, r1 in zip(rows, rows_run):
        assert _np(r0).tobytes() == _np(r1).tobytes()
    res, res_run = stepped.result(), streamed.result()
    assert list(res) == list(res_run)
    for k in res:
        assert same(res[k], res_run[k]), (k, res[k], res_run[k])
    pr, he, rpe = set(M.MATCH_PR_NAMES), {k for k in res if k.startswith("HE")}, {k for k in res if k.startswith("RPE")}
    assert len(he) == 8 and len(rpe) == 10 and pr <= set(res) and set(res) == set(stepped.names) | he | rpe | pr
    for name, (ev, with_pose, with_depth) in singles.items():
        for (evs, img, pose, depth), r0 in zip(full, rows):
            r1, _ = ev.step(evs, _t(img), hom, pose=pose if with_pose else None, depth=depth if with_depth else None)
            assert _np(r0).tobytes() == _np(r1).tobytes(), name
        one = ev.result()
        assert set(one) == set(stepped.names) | (he if name == "homography" else rpe | pr if with_depth else rpe), name
        for k in one:
            assert same(one[k], res[k]), (name, k, one[k], res[k])
