"""GPU tests (-m gpu), component: mnn, against the float64 restatement tests/mnn_f64.py on inputs whose fp32 similarity is exact
(test_mnn_f64_cpu.py::test_fp32_similarity_is_exact_for_every_gpu_case).  Matches, scores, second neighbours, the similarity and
every threshold decision are compared with array_equal; only log_assignment has a bound, derived in the test from the plain fp32
evaluation's own error.  The cases (mnn_f64.CASES) are the smallest shapes that reach

  tail_small      K tail of the tile engine (D = 36: a partial second K-slab), partial tiles, a single column, an empty side,
                  18 workgroups (no multiple of the 8 the XCD remap works in)
  tile_edge       caps of exactly one tile and of two tiles plus one column, counts 127 / 128 (6 workgroups)
  one_slab_*      D = 4: one partial slab; D = 32: exactly one slab
  whole_fast      the predicate-free buffer-load path (whole tiles, K % 32 == 0) and partial tiles in one launch
  whole_tail      whole tiles forced through the predicated path by the K tail (D = 260)
  beyond_1024(_t) second and third trip of the 1024-thread finalize / gather loops with different caps on the two sides
  clamp           a count tensor that says more than the cap

Rows past a pair's count hold NaN in descriptors and keypoints; every call runs twice and must repeat bit for bit."""
import numpy as np
import pytest
import torch

import mnn_f64 as F
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu
N = pkg.native
EPS32 = float(np.finfo(np.float32).eps)
CASE_IDS = [(name, fam) for name in F.CASES for fam in F.FAMILIES]


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _dev(c):
    return _t(c.d0), _i32(c.n_arg), _t(c.d1), _i32(c.m_arg)


def _twice(fn):
    """run `fn` (-> dict of numpy arrays) twice; the two results must be bit-equal; returns the first"""
    a, b = fn(), fn()
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{k} differs from run to run"
    return a


def _match_arrays(r):
    return {"matches0": _np(r.matches0), "matches1": _np(r.matches1), "scores0": _np(r.scores0), "scores1": _np(r.scores1)}


def _assert_matches(c, got, ratio=None, dist=None, tag=""):
    """every pair equals the restatement up to its count; -1 / 0.0 past it"""
    assert got["matches0"].dtype == np.int64 and got["matches0"].shape == (c.B, c.cap0) and got["matches1"].shape == (c.B, c.cap1)
    for b, R in enumerate(c.pairs):
        m0, m1, s0, s1 = R.matches(ratio, dist)
        for key, exp, cnt in (("matches0", m0, c.n[b]), ("matches1", m1, c.m[b]), ("scores0", s0, c.n[b]), ("scores1", s1, c.m[b])):
            assert np.array_equal(got[key][b, :cnt], exp), (c.name, c.family, tag, key, b)
            assert (got[key][b, cnt:] == (-1 if key.startswith("matches") else 0.0)).all(), (c.name, c.family, tag, key, b, "padding")


@pytest.mark.parametrize("name,family", CASE_IDS)
def test_matches_and_log_assignment(oracle, name, family):
    """MODE 0 (want_la=False) and MODE 5 (want_la=True) against the restatement and against each other; log_assignment of the
    exact-unit family over [:n+1, :m+1] within max(4 x the oracle's own error against float64, 8 eps32 max|la64|): the oracle is the
    plain fp32 evaluation of the same formula, the factor 4 covers the order in which the kernel merges per-chunk sum-exps, the
    second term keeps the bound from collapsing where the oracle happens to be exact."""
    c = F.build_case(name, family)
    d0, n, d1, m = _dev(c)
    plain = _twice(lambda: _match_arrays(N.mnn(d0, n, d1, m, want_la=False)))
    _assert_matches(c, plain, tag="mode0")

    def with_la():
        r = N.mnn(d0, n, d1, m, want_la=True)
        out = _match_arrays(r)
        la = _np(r.la)
        assert la.shape == (c.B, c.cap0 + 1, c.cap1 + 1)
        for b in range(c.B):
            out[f"la{b}"] = np.ascontiguousarray(la[b, :c.n[b] + 1, :c.m[b] + 1])
        return out

    full = _twice(with_la)
    _assert_matches(c, full, tag="mode5")
    for k in plain:
        assert np.array_equal(plain[k], full[k]), (k, "MODE 0 vs MODE 5")
    if family != "unit":
        return
    for b, R in enumerate(c.pairs):
        la64 = R.log_assignment()
        got = full[f"la{b}"].astype(np.float64)
        if R.empty:
            assert np.array_equal(got, la64)  # zeros
            continue
        orc = oracle.mnn(c.d0[b, :c.n[b]], c.d1[b, :c.m[b]])["log_assignment"].astype(np.float64)
        e_orc, e_gpu = float(np.abs(orc - la64).max()), float(np.abs(got - la64).max())
        bound = max(4 * e_orc, 8 * EPS32 * float(np.abs(la64).max()))
        print(f"log_assignment {name}.{b} ({c.n[b]}x{c.m[b]}, D={c.D}): oracle {e_orc:.3e}, kernel {e_gpu:.3e}, bound {bound:.3e}")
        assert np.array_equal(got[-1], la64[-1]) and np.array_equal(got[:, -1], la64[:, -1])  # the zero dustbin row / column
        assert e_gpu <= bound, (name, b, e_gpu, bound)


@pytest.mark.parametrize("name,family", CASE_IDS)
def test_threshold_decisions(name, family):
    """ratio only, distance only and both; on the exact-unit cases with D >= 32 one row and one column sit at d0 == ratio_sq d2
    (ratio 0.5) and one at d0 == dist_sq (distance 1.0) exactly, and keep their match only through the `<=`"""
    c = F.build_case(name, family)
    d0, n, d1, m = _dev(c)
    for ratio, dist in F.THRESHOLDS:
        got = _twice(lambda: _match_arrays(N.mnn(d0, n, d1, m, want_la=False, ratio_thresh=ratio, distance_thresh=dist)))
        _assert_matches(c, got, ratio, dist, tag=f"ratio={ratio} dist={dist}")
    got = _match_arrays(N.mnn(d0, n, d1, m, want_la=True, ratio_thresh=0.75, distance_thresh=1.0))  # MODE 5 + MODE 4
    _assert_matches(c, got, 0.75, 1.0, tag="with log_assignment")
    for b, info in enumerate(c.info):
        if info["ratio_eq"] is None:
            continue
        (i, j), (p, q) = info["ratio_eq"], info["dist_eq"]
        r = _match_arrays(N.mnn(d0, n, d1, m, want_la=False, ratio_thresh=0.5))
        assert r["matches0"][b, i] == j and r["matches1"][b, j] == i and r["matches0"][b, p] == -1
        r = _match_arrays(N.mnn(d0, n, d1, m, want_la=False, distance_thresh=1.0))
        assert r["matches0"][b, p] == q and r["matches1"][b, q] == p


def _unkey(k):
    """einx_ordered_unkey: ordered 32-bit key -> float32"""
    k = k.astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("name,family", CASE_IDS)
def test_second_neighbours(monkeypatch, name, family):
    """MODE 4's keys themselves: the last two regions of the matcher's workspace (match_tiles.h::carve: row2 [B,cap0] | col2
    [B,cap1], 32-bit ordered keys, each region rounded up to 256 bytes, 0 = no second candidate / past the count)"""
    c = F.build_case(name, family)
    d0, n, d1, m = _dev(c)
    made = []
    real = N._workspace

    def keep(nbytes, device):
        made.append(real(nbytes, device))
        return made[-1]

    monkeypatch.setattr(N, "_workspace", keep)
    N.mnn(d0, n, d1, m, want_la=False, ratio_thresh=0.5)
    assert len(made) == 1
    ws = _np(made[0])
    up = lambda v: (v + 255) & ~255  # noqa: E731
    s1, s0 = up(c.B * c.cap1 * 4), up(c.B * c.cap0 * 4)
    col2 = ws[len(ws) - s1:].view(np.uint32)[:c.B * c.cap1].reshape(c.B, c.cap1)
    row2 = ws[len(ws) - s1 - s0:len(ws) - s1].view(np.uint32)[:c.B * c.cap0].reshape(c.B, c.cap0)
    for b, R in enumerate(c.pairs):
        nb, mb = c.n[b], c.m[b]
        assert (row2[b, nb:] == 0).all() and (col2[b, mb:] == 0).all()
        if R.empty or mb < 2:
            assert (row2[b] == 0).all()
        else:
            assert (row2[b, :nb] != 0).all() and np.array_equal(_unkey(row2[b, :nb]).astype(np.float64), R.sec0), (name, b, "rows")
        if R.empty or nb < 2:
            assert (col2[b] == 0).all()
        else:
            assert (col2[b, :mb] != 0).all() and np.array_equal(_unkey(col2[b, :mb]).astype(np.float64), R.sec1), (name, b, "columns")


@pytest.mark.parametrize("name,family", CASE_IDS)
def test_matched_keypoints(name, family):
    """einx_mnn_gather (mutual check + compaction in one launch) == einx_gather_matches on the same matches == the restatement"""
    c = F.build_case(name, family)
    d0, n, d1, m = _dev(c)
    k0, k1 = _t(c.k0), _t(c.k1)

    def packed(r, cols):
        nm = _np(r.nmatch)
        assert nm.dtype == np.int32 and nm.shape == (c.B,)
        assert tuple(r.mk0.shape) == (c.B, c.cap0, cols) and tuple(r.mk1.shape) == (c.B, c.cap0, cols)
        out = dict(_match_arrays(r), nmatch=nm)
        mk0, mk1 = _np(r.mk0), _np(r.mk1)
        for b in range(c.B):
            out[f"mk0.{b}"] = np.ascontiguousarray(mk0[b, :max(int(nm[b]), 0)])
            out[f"mk1.{b}"] = np.ascontiguousarray(mk1[b, :max(int(nm[b]), 0)])
        return out

    def check(got, cols, ratio=None, dist=None):
        _assert_matches(c, got, ratio, dist, tag=f"gather cols={cols}")
        for b, R in enumerate(c.pairs):
            m0 = R.matches(ratio, dist)[0]
            e0, e1 = F.matched_kpts(c.k0[b, :c.n[b]], c.k1[b, :c.m[b]], m0, cols)
            assert got["nmatch"][b] == len(e0), (name, b, cols)
            assert np.array_equal(got[f"mk0.{b}"], e0) and np.array_equal(got[f"mk1.{b}"], e1), (name, b, cols)

    for cols in (1, 2, 3):
        fused = _twice(lambda: packed(N.mnn(d0, n, d1, m, want_la=False, gather=(k0, k1, cols)), cols))
        check(fused, cols)
        if cols == 1:
            continue  # einx_gather_matches takes 2 or 3 columns
        alone = _twice(lambda: packed(N.gather_matches(N.mnn(d0, n, d1, m, want_la=False), k0, k1, n, cols), cols))
        check(alone, cols)
        for k in fused:
            assert np.array_equal(fused[k], alone[k]), (k, cols)
    thr = _twice(lambda: packed(N.mnn(d0, n, d1, m, want_la=False, ratio_thresh=0.75, distance_thresh=1.0, gather=(k0, k1, 3)), 3))
    check(thr, 3, 0.75, 1.0)
    if name.startswith("beyond_1024"):  # the carried compaction offset really carries: matched rows on both sides of 1024
        hit = np.nonzero(c.pairs[0].matches()[0] > -1)[0]
        assert (hit >= 1024).any() and (hit < 1024).any()
        hit = np.nonzero(c.pairs[0].matches(0.75, 1.0)[0] > -1)[0]
        assert (hit >= 1024).any() and (hit < 1024).any()


@pytest.mark.parametrize("name,family", CASE_IDS)
def test_similarity(name, family):
    c = F.build_case(name, family)
    d0, n, d1, m = _dev(c)
    got = _twice(lambda: {"sim": _np(N.similarity(d0, n, d1, m))})["sim"]
    exp = np.zeros((c.B, c.cap0, c.cap1), np.float64)
    for b, R in enumerate(c.pairs):
        exp[b, :c.n[b], :c.m[b]] = R.sim
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), exp)  # zero outside every n x m block


@pytest.mark.parametrize("cols", [2, 3])
def test_compact_matches_beyond_256_pairs(cols):
    """compact_rows_kernel's prefix loop `for (i = tid; i < b; i += 256)` takes its second trip from pair 256 on"""
    c = F.compact_case()
    assert c.B > 256
    d0, n, d1, m = _dev(c)
    k0, k1 = _t(c.k0), _t(c.k1)

    def run():
        r = N.compact_matches(N.mnn(d0, n, d1, m, want_la=False, gather=(k0, k1, cols)))
        nm = _np(r.nmatch)
        total = int(nm.sum())
        assert tuple(r.mk0_flat.shape) == (c.B * c.cap0, cols)
        return dict(_match_arrays(r), nmatch=nm, mk0=_np(r.mk0), mk1=_np(r.mk1), flat0=_np(r.mk0_flat)[:total], flat1=_np(r.mk1_flat)[:total])

    a, b = run(), run()
    for k in ("matches0", "matches1", "nmatch", "flat0", "flat1"):
        assert a[k].tobytes() == b[k].tobytes(), k
    _assert_matches(c, a)
    exp = [F.matched_kpts(c.k0[i, :c.n[i]], c.k1[i, :c.m[i]], c.pairs[i].matches()[0], cols) for i in range(c.B)]
    assert np.array_equal(a["nmatch"], [len(e[0]) for e in exp])
    assert a["nmatch"][256:].sum() > 0 and (a["nmatch"] == 0).any() and (a["nmatch"] > 1).any()
    assert np.array_equal(a["flat0"], np.concatenate([e[0] for e in exp])) and np.array_equal(a["flat1"], np.concatenate([e[1] for e in exp]))
    assert np.array_equal(a["flat0"], np.concatenate([a["mk0"][i, :a["nmatch"][i]] for i in range(c.B)]))
    assert np.array_equal(a["flat1"], np.concatenate([a["mk1"][i, :a["nmatch"][i]] for i in range(c.B)]))


@pytest.mark.parametrize("ratio,dist", [(None, None), (0.5, None), (0.75, 1.0)])
def test_matcher_module_beyond_1024_keypoints(oracle, ratio, dist):
    """NearestNeighborMatcher on one pair of 1100 x 1300 keypoints: no layer limits a side to 1024"""
    d0, d1, k0, k1, info = F.matcher_pair()
    n, m = d0.shape[0], d1.shape[0]
    R = F.Restated(d0, d1)
    m0, m1, s0, s1 = R.matches(ratio, dist)
    hit = np.nonzero(m0 > -1)[0]
    assert (hit >= 1024).any() and (hit < 1024).any()
    mm = pkg.NearestNeighborMatcher(ratio_thresh=ratio or False, distance_thresh=dist or False, mutual_check=True)
    size = torch.tensor([260, 346])
    f0 = {"sparse_descriptors": _t(d0)[None], "sparse_positions": _t(k0)[None], "image_size": [size]}
    f1 = {"sparse_descriptors": _t(d1)[None], "sparse_positions": _t(k1)[None], "image_size": [size]}

    def run():
        r = mm(f0, f1)
        return {k: _np(r[k]) for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "matched_kpts0", "matched_kpts1",
                                       "log_assignment")}

    got = _twice(run)
    assert got["matches0"].shape == (1, n) and got["matches1"].shape == (1, m) and got["log_assignment"].shape == (1, n + 1, m + 1)
    assert np.array_equal(got["matches0"][0], m0) and np.array_equal(got["matches1"][0], m1)
    assert np.array_equal(got["matching_scores0"][0], s0) and np.array_equal(got["matching_scores1"][0], s1)
    e0, e1 = F.matched_kpts(k0, k1, m0, 3)
    assert got["matched_kpts0"].shape == e0.shape == (len(hit), 3)
    assert np.array_equal(got["matched_kpts0"], e0) and np.array_equal(got["matched_kpts1"], e1)
    if ratio == 0.5:
        i, j = info["ratio_eq"]
        assert i >= 1024 and m0[i] == j
    la64 = R.log_assignment()
    e_orc = float(np.abs(oracle.mnn(d0, d1)["log_assignment"].astype(np.float64) - la64).max())
    e_gpu = float(np.abs(got["log_assignment"][0].astype(np.float64) - la64).max())
    print(f"log_assignment matcher_pair ({n}x{m}): oracle {e_orc:.3e}, kernel {e_gpu:.3e}")
    assert e_gpu <= max(4 * e_orc, 8 * EPS32 * float(np.abs(la64).max()))  # as in test_matches_and_log_assignment
