"""GPU tests (-m gpu), component: ground-truth matches and matcher precision / recall (csrc/gt_matches.hip) against the
dense restatement tests/gt_matches_f64.py on inputs that fp32 evaluates exactly
(test_gt_matches_f64_cpu.py::test_fp32_evaluation_is_exact_for_every_gpu_case).  Every comparison is array_equal; only
average_precision (a closed form on the device) is held to cap0 * 2^-52 against the reference's long form.  What each case plants
is asserted from the restatement alone in test_gt_matches_f64_cpu.py::test_gpu_cases_hold_what_the_gpu_test_needs:

  gt_label    second and third trip of the 1024-point LDS chunk loop on either side, partners and exact ties across chunks and across
              the group of four, whole workgroups past the count, sides of one point, an empty side, dist / min dist0 equal to a
              threshold, max(dist0, dist1) decided by dist1, an invisible nearest neighbour, invisible row 0 and column 0, NaN
              projections on invisible points, neg_th < pos_th; pose and homography form, both orderings, NaN and finite garbage
              past the counts
  gt_project  the sampler's zero-padded taps on every border and corner, points wholly outside, far / infinite / NaN coordinates,
              holes under the one tap and under a weighted tap (nearest pixel good, a hole, outside the map); projections exactly on
              and a quarter pixel beyond each border of the other camera, q.z == 1e-4 and the next float, T_1to0 given and NULL,
              depth maps and precomputed depths
  gt_matches  both stages in one call at 1030 x 2049, twice, and captured in a graph
  match_pr    ties at the top score in one lane and across lanes, all-equal and all -inf scores, +inf, scores past the count, empty
              denominators"""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import gt_matches_f64 as F
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu
M = import_module(pkg.__name__ + ".core.metrics._native_metrics")
LABEL_KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1", "pos0")
DTYPES = {"matches0": torch.int64, "matches1": torch.int64, "matching_scores0": torch.float32, "matching_scores1": torch.float32,
          "pos0": torch.int32, "proj_0to1": torch.float32, "proj_1to0": torch.float32, "depth_keypoints0": torch.float32,
          "depth_keypoints1": torch.float32, "valid0": torch.bool, "valid1": torch.bool, "visible0": torch.bool, "visible1": torch.bool}
LAYOUTS = (("yx", 3), ("xy", 2))  # the PairBatch rows (y, x, score) and bare (x, y)


def _i32(v):
    return torch.tensor([int(x) for x in v], dtype=torch.int32, device=DEV)


def _assert_equal(got, exp, keys, tag):
    """every output equals the restatement bit for bit (float32 widened to float64), shapes and dtypes as documented"""
    out = {}
    for k in keys:
        assert got[k].dtype == DTYPES[k], (tag, k, got[k].dtype)
        out[k] = _np(got[k])
        assert out[k].shape == exp[k].shape, (tag, k, out[k].shape, exp[k].shape)
        assert np.array_equal(out[k].astype(exp[k].dtype), exp[k], equal_nan=True), (tag, k)
    return out


def _assert_same_bits(a, b, tag):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (tag, k)


# ------------------------------------------------------------------------------------------------ stage B
@pytest.mark.parametrize("name", list(F.LABEL_CASES))
def test_gt_label(name):
    c = F.label_case(name)
    n, m = _i32(p.n for p in c.pairs), _i32(p.m for p in c.pairs)
    for form in F.FORMS:
        exp = F.padded_expected([F.with_scores(e) for e in F.label_expected(name, form)], c.cap0, c.cap1, LABEL_KEYS)
        ins = [F.label_inputs(p, form) for p in c.pairs]
        first = None
        for ordering, cols in LAYOUTS:
            for fill in (np.nan, 7.0):  # rows past the counts: NaN, then finite garbage (visible and valid)
                kp0, kp1 = F.pad_rows([i[0] for i in ins], c.cap0, fill, ordering, cols), F.pad_rows([i[1] for i in ins], c.cap1, fill, ordering, cols)
                p01, p10 = F.pad_rows([i[2] for i in ins], c.cap0, fill), F.pad_rows([i[3] for i in ins], c.cap1, fill)
                masks = [None] * 4
                if form == "pose":
                    masks = [_t(F.pad_flags([i[k] for i in ins], cap, True)) for k, cap in ((4, c.cap0), (5, c.cap1), (6, c.cap0), (7, c.cap1))]
                got = M.gt_label(_t(kp0), _t(kp1), n, m, _t(p01), _t(p10), *masks, pos_th=c.pos_th, neg_th=c.neg_th, ordering=ordering)
                out = _assert_equal(got, exp, LABEL_KEYS, (name, form, ordering, fill))
                if first is None:
                    first = out
                _assert_same_bits(first, out, (name, form, ordering, fill))


# ------------------------------------------------------------------------------------------------ stage A
def _project(c, b_kp0, b_kp1, ordering, cols, T10, precomputed=None, fill=np.nan):
    kp0, kp1 = F.pad_rows(b_kp0, c.cap0, fill, ordering, cols), F.pad_rows(b_kp1, c.cap1, fill, ordering, cols)
    pre = None
    if precomputed is not None:
        pre = (_t(F.pad_values([p[0] for p in precomputed], c.cap0, fill)), _t(F.pad_flags([p[1] for p in precomputed], c.cap0, True)),
               _t(F.pad_values([p[2] for p in precomputed], c.cap1, fill)), _t(F.pad_flags([p[3] for p in precomputed], c.cap1, True)))
    return M.gt_project(_t(kp0), _t(kp1), _i32(c.n), _i32(c.m), None if pre else _t(c.depth0), None if pre else _t(c.depth1), _t(c.K0), _t(c.K1),
                        _t(c.T01), None if T10 is None else _t(T10), ordering=ordering, precomputed=pre)


@pytest.mark.parametrize("what", ["sampler", "projection_maps", "projection_precomputed"])
def test_gt_project(what):
    if what == "sampler":  # depths and validity only: a general depth k/64 leaves q.x / q.z inexact
        c = F.sampler_case()
        pairs = []
        for b in range(c.B):
            (d0, v0, _), (d1, v1, _) = F.sample_depth(c.kp0[b], c.depth0[b]), F.sample_depth(c.kp1[b], c.depth1[b])
            pairs.append({"depth_keypoints0": d0, "depth_keypoints1": d1, "valid0": v0, "valid1": v1})
        keys = ("depth_keypoints0", "depth_keypoints1", "valid0", "valid1")
        exp = F.padded_expected(pairs, c.cap0, c.cap1, keys)
        first = None
        for ordering, cols in LAYOUTS:
            for T10 in (c.T10, None):
                got = _project(c, c.kp0, c.kp1, ordering, cols, T10)
                out = _assert_equal(got, exp, keys, (what, ordering))
                first = first or out
                _assert_same_bits(first, out, (what, ordering))
                for k in ("proj_0to1", "proj_1to0", "visible0", "visible1"):  # zeros past the counts, whatever the rows hold
                    cnt = c.n if k.endswith(("0to1", "e0")) else c.m
                    assert all(not _np(got[k])[b, cnt[b]:].any() for b in range(c.B)), k
        return
    c = F.projection_case()
    pre = c.pre if what == "projection_precomputed" else None
    for T10 in (c.T10, None):  # the explicit inverse, and the kernel's own (R^T, -R^T t)
        pairs = [F.project_pair(c.kp0[b], c.kp1[b], c.K0[b], c.K1[b], c.T01[b], None if T10 is None else T10[b],
                                **(dict(precomputed=pre[b]) if pre else dict(depth0=c.depth0[b], depth1=c.depth1[b]))) for b in range(c.B)]
        exp = F.padded_expected(pairs, c.cap0, c.cap1, F.STAGE_A_KEYS)
        first = None
        for ordering, cols in LAYOUTS:
            for fill in (np.nan, 7.0):
                out = _assert_equal(_project(c, c.kp0, c.kp1, ordering, cols, T10, pre, fill), exp, F.STAGE_A_KEYS, (what, ordering, T10 is None))
                first = first or out
                _assert_same_bits(first, out, (what, ordering, fill))


# ------------------------------------------------------------------------------------------------ A + B in one call
SCENE_KEYS = F.STAGE_A_KEYS + LABEL_KEYS


def _scene_expected():
    c = F.scene_case()
    return c, F.padded_expected([F.with_scores(e) for e in F.scene_expected()], c.cap0, c.cap1, SCENE_KEYS)


def test_gt_matches():
    c, exp = _scene_expected()
    first = None
    for ordering, cols in LAYOUTS:
        for T10 in (c.T10, None):
            for _ in range(2):  # a second run equals the first
                kp0, kp1 = F.pad_rows(c.kp0, c.cap0, np.nan, ordering, cols), F.pad_rows(c.kp1, c.cap1, np.nan, ordering, cols)
                got = M.gt_matches(_t(kp0), _t(kp1), _i32(c.n), _i32(c.m), _t(c.depth0), _t(c.depth1), _t(c.K0), _t(c.K1), _t(c.T01),
                                   None if T10 is None else _t(T10), pos_th=c.pos_th, neg_th=c.neg_th, ordering=ordering)
                assert set(got) == set(SCENE_KEYS)
                out = _assert_equal(got, exp, SCENE_KEYS, ("scene", ordering, T10 is None))
                first = first or out
                _assert_same_bits(first, out, ("scene", ordering, T10 is None))


def test_graph_capture_and_replay_beyond_1024():
    """the raw einx_gt_matches call at 1030 x 2049 captured on a side stream, replayed twice into poisoned outputs and a poisoned
    workspace: every chunk trip reads what this replay staged, nothing a previous launch left"""
    c, exp = _scene_expected()
    L, N = pkg.native.lib(), pkg.native
    P = N._ptr
    kp0, kp1 = _t(F.pad_rows(c.kp0, c.cap0, np.nan, "yx", 3)), _t(F.pad_rows(c.kp1, c.cap1, np.nan, "yx", 3))
    p = M._gt_params(kp0, kp1, "yx", c.pos_th, c.neg_th, False, c.size0, c.size1)
    t = {k: _t(v) for k, v in dict(d0=c.depth0, d1=c.depth1, K0=c.K0.reshape(-1, 9), K1=c.K1.reshape(-1, 9), T01=c.T01.reshape(-1, 16),
                                   T10=c.T10.reshape(-1, 16)).items()}
    n, m = _i32(c.n), _i32(c.m)
    o = M._gt_stage_a_outputs(c.B, c.cap0, c.cap1, DEV)
    o.update(M._gt_label_outputs(c.B, c.cap0, c.cap1, DEV))
    ws = torch.empty(L.einx_gt_matches_ws_bytes(ctypes.byref(p)), dtype=torch.uint8, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        rc = L.einx_gt_matches(ctypes.byref(p), P(kp0), P(kp1), P(n), P(m), P(t["d0"]), P(t["d1"]), P(t["K0"]), P(t["K1"]), P(t["T01"]), P(t["T10"]),
                               None, None, None, None, None, P(ws), P(o["depth_keypoints0"]), P(o["depth_keypoints1"]), P(o["valid0"]),
                               P(o["valid1"]), P(o["proj_0to1"]), P(o["proj_1to0"]), P(o["visible0"]), P(o["visible1"]), P(o["matches0"]),
                               P(o["matches1"]), P(o["matching_scores0"]), P(o["matching_scores1"]), P(o["pos0"]), N._stream(kp0))
    assert rc == 0
    for _ in range(2):
        for v in o.values():
            v.fill_(0x55 if v.dtype != torch.float32 else float("nan"))
        ws.fill_(0xAB)
        graph.replay()
        torch.cuda.synchronize()
        for k in SCENE_KEYS:
            assert np.array_equal(_np(o[k]).astype(exp[k].dtype), exp[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------------ stage C
@pytest.mark.parametrize("cap", F.PR_CAPS)
def test_match_pr(cap):
    """recall, precision and accuracy equal the restatement; average_precision (closed form) within cap0 * 2^-52 of the long form:
    cap0 float64 roundings of terms of magnitude <= 1.  Measured on an MI355X: at most 1.1e-16 (cap 64, bound 1.4e-14); 5.6e-17 at
    cap 1030 against 2.3e-13."""
    m, gt, sc, n, names, _ = F.pr_case(cap)
    exp = F.pr_expected(cap)
    first = None
    for _ in range(2):
        rows = _np(M.match_pr(_t(m), _t(gt), _t(n), scores0=_t(sc)))
        assert rows.dtype == np.float64 and rows.shape == exp.shape
        first = rows if first is None else first
        assert rows.tobytes() == first.tobytes()
    assert np.array_equal(np.isnan(rows), np.isnan(exp))
    err = np.abs(rows[:, 3] - exp[:, 3])
    print(f"match_pr cap {cap}: max |closed form - long form| {np.nanmax(err):.3e} (bound {cap * 2.0 ** -52:.3e}), worst pair {names[int(np.nanargmax(err))]}")
    for b, name in enumerate(names):
        assert np.array_equal(rows[b, :3], exp[b, :3], equal_nan=True), (cap, name, rows[b], exp[b])
        assert np.isnan(exp[b, 3]) or err[b] <= cap * 2.0 ** -52, (cap, name, rows[b, 3], exp[b, 3])
