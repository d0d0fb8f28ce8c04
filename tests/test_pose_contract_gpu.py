"""Relative pose on the device (csrc/pose.hip) across its whole call contract: the fixed cases of tests/ransac_cases.py (two
different cameras, a float64 K, thresh / conf / seed / max_iters, n = 5 and 6, n past the score kernel's 256-point trips) against
the float64 restatement and against a certificate computed from the kernel's outputs alone; bit-for-bit invariances (ordering,
columns, slot, nmatch past cap, no ground truth); batches over 64 pairs; best models on a round's first and last iteration; the
branches of the error epilogue.  tests/test_ransac_contract_cpu.py establishes on the CPU what these tests rely on.

Measured on the MI355X on 2026-10-20 over the sixteen POSE_CASES (ragged batches grouped by K's dtype and kwargs): the worst
certificate residual |x2' E' x1| of the device's (R, t) over the five drawn matches is 4.712e-14, against a gate of 3.6e-13 =
10 x the restatement's own worst (ransac_cases.CERT_WORST); |dR| 7.9e-14, |dt| 3.1e-13 and |d errors| 9.7e-9 against the
restatement at most.  No case is pinned.  Cases 0, 1 (ill-conditioned samples) and 11 (solutions far out in z) failed until
the two faults of DESIGN.md 8b were fixed in solve5."""
import numpy as np
import pytest
import torch

import pose_f64 as P
import ransac_cases as C
from gpu_support import _np, _t, pkg
from ransac_cases import CERT_CEILING, CERT_GATE

pytestmark = pytest.mark.gpu
from importlib import import_module  # noqa: E402

_nm = import_module(pkg.__name__ + ".core.metrics._native_metrics")
CODES = {v: k for k, v in _nm.POSE_STATUS.items()}
CERT_MEASURED = 4.712e-14  # the device's worst certificate residual over POSE_CASES (header)
PINNED = {}  # case index -> (hypothesis, the two inlier counts): at most one, for a shown route difference (none)


def _cap_for(n):
    return 64 if n <= 64 else 128 if n <= 128 else 64 * ((n + 63) // 64)


def _stack(pairs, cap, cols=3, ordering="yx", nmatch=None, T=True):
    B = len(pairs)
    mk0 = np.zeros((B, cap, cols), np.float32)
    mk1 = np.zeros((B, cap, cols), np.float32)
    nm = np.zeros(B, np.int32)
    for b, (a0, a1, _, _, _) in enumerate(pairs):
        if ordering == "xy":
            a0, a1 = a0.copy(), a1.copy()
            a0[:, :2], a1[:, :2] = a0[:, 1::-1], a1[:, 1::-1]
        mk0[b, :len(a0)], mk1[b, :len(a1)], nm[b] = a0[:, :cols], a1[:, :cols], len(a0)
    if nmatch is not None:
        nm = np.asarray(nmatch, np.int32)
    K0 = np.stack([p[2] for p in pairs])
    K1 = np.stack([p[3] for p in pairs])
    Ts = _t(np.stack([p[4] for p in pairs])) if T else None
    return _t(mk0), _t(mk1), _t(nm), _t(K0), _t(K1), Ts


def _run(args, **kw):
    out = [_np(x) for x in _nm.relative_pose(*args, **kw)]
    torch.cuda.synchronize()
    return out


def _same(x, y, msg=None):
    for a, b in zip(x, y):
        assert np.array_equal(a, b, equal_nan=True), msg


def _row(out, b):
    return [x[b] for x in out]


@pytest.fixture(scope="module")
def cases():
    """every POSE_CASES entry through the device, stacked into ragged batches grouped by K's dtype and kwargs
    -> {case index: (pair, kwargs, restatement, device outputs of its slot, cap)}"""
    groups = {}
    for i, c in enumerate(C.POSE_CASES):
        groups.setdefault((c[4], tuple(sorted(c[5].items()))), []).append(i)
    res = {}
    for (kdt, kw), idx in groups.items():
        refs = [C.pose_ref(i) for i in idx]
        cap = _cap_for(max(len(r[0][0]) for r in refs))
        args = _stack([r[0] for r in refs], cap)
        assert args[3].dtype == (torch.float64 if kdt == np.float64 else torch.float32)
        out = _run(args, **dict(kw))
        for b, i in enumerate(idx):
            res[i] = refs[b] + (_row(out, b), cap)
    return res


def test_cases_match_restatement(cases):
    worst = [0.0, 0.0, 0.0]
    assert len(PINNED) <= 1
    for i in sorted(cases):
        pair, kw, r, (R, t, mask, status, rows), cap = cases[i]
        n = len(pair[0])
        assert mask.shape == (cap,) and not mask[n:].any(), i
        if r["status"] != "ok":
            assert status == CODES[r["status"]], (i, status, r["status"])
            assert not mask.any() and np.all(np.isinf(rows[:3])) and rows[3] == 0.0
            continue
        if i in PINNED:
            assert status >= 0 and (status >> 4) != r["it"][0], f"case {i} now agrees: unpin it"
            continue
        assert status >= 0 and (status >> 4) == r["it"][0], (i, status, r["it"])
        assert np.array_equal(mask[:n], r["mask"]), (i, np.nonzero(mask[:n] != r["mask"])[0][:10])
        assert rows[3] == mask.sum() / n == r["mask"].mean(), i
        e = P.pose_errors(pair[4], r["R"], r["t"])
        d = (np.abs(R - r["R"]).max(), min(np.abs(t - r["t"]).max(), np.abs(t + r["t"]).max()), np.abs(rows[:3] - e).max())
        print(f"case {i}: n {n} it {status >> 4} |dR| {d[0]:.2e} |dt| {d[1]:.2e} |d errors| {d[2]:.2e}")
        worst = [max(w, v) for w, v in zip(worst, d)]
    print(f"measured: max |dR|, |dt|, |d errors| = {worst}")
    assert worst[0] < 1e-9 and worst[1] < 1e-9 and worst[2] < 1e-5, worst


def _certificate(pair, kw, out, tag):
    """checks of the device's outputs of one solved pair that need no restatement -> the residual of (b)"""
    R, t, mask, status, rows = out
    n = len(pair[0])
    seed, max_iters = kw.get("seed", P.DEFAULT_SEED), kw.get("max_iters", 1000)
    it = int(status) >> 4
    assert 0 <= it < max_iters and P.draw(seed, it, n) is not None, tag                             # (a)
    res = C.sample_residual(pair, R, t, it, seed)                                                    # (b)
    x1, x2 = C.pose_points(pair)
    E = P.skew(t) @ R
    E = E / np.linalg.norm(E)
    thr2 = np.float32(P.ransac_threshold(kw.get("thresh", 1.0), pair[2], pair[3]) ** 2)
    inl = P.sampson_f32(E, x1, x2)[0] <= thr2
    want = np.zeros(n, bool)
    want[inl] = P.triangulate_ok(R, t, x1[inl], x2[inl])
    assert np.array_equal(mask[:n], want), (tag, np.nonzero(mask[:n] != want)[0][:10])               # (c)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12, tag   # (d)
    assert abs(np.linalg.norm(t) - 1.0) < 1e-12, tag
    e = np.array(P.pose_errors(pair[4], R, t))                                                       # (e)
    assert np.array_equal(np.isnan(e), np.isnan(rows[:3])) and np.nanmax(np.abs(rows[:3] - e)) < 1e-5, (tag, rows, e)
    return res


def test_certificate(cases):
    """for every solved case with n > 5, from the kernel's outputs alone: the pose vanishes on the sample of the iteration that
    `status` names, the mask is that pose's, R is a rotation and t a unit vector, the error rows are that pose's errors"""
    worst, checked = 0.0, 0
    for i in sorted(cases):
        pair, kw, r, out, _ = cases[i]
        if out[3] < 0 or len(pair[0]) <= 5:
            continue
        res = _certificate(pair, kw, out, i)
        print(f"case {i}: certificate residual {res:.3e}")
        worst, checked = max(worst, res), checked + 1
    print(f"measured: worst certificate residual on the device {worst:.3e} (gate {CERT_GATE:.3e})")
    assert checked >= 14
    assert worst <= CERT_GATE <= CERT_CEILING, worst


# ------------------------------------------------------------------ invariances, bit for bit, on float32 K0 != K1 pairs
@pytest.fixture(scope="module")
def tile():
    """the eleven pairs of ransac_cases.tile_pairs: (pairs, the batch's outputs, every pair's outputs run alone)"""
    pairs = C.tile_pairs("pose")
    out = _run(_stack(pairs, C.TILE_CAP), **C.TILE_KW)
    alone = [_row(_run(_stack([p], C.TILE_CAP), **C.TILE_KW), 0) for p in pairs]
    return pairs, out, alone


def test_tile_pairs_solve(tile):
    """the pairs the invariances run on are not trivial: nine poses that pass their certificate, a "few" and a "noE" """
    pairs, out, _ = tile
    status = out[3]
    for k, spec in enumerate(C.TILE_SPEC):
        if spec in ("few", "same"):
            assert status[k] == CODES["few" if spec == "few" else "noE"], k
        else:
            assert status[k] >= 0, (k, status[k])
            if spec[0] > 5:
                assert _certificate(pairs[k], C.TILE_KW, _row(out, k), ("tile", k)) <= CERT_GATE


def test_ordering_xy_and_two_columns(tile):
    pairs, out, _ = tile
    for cols, ordering in ((3, "xy"), (2, "yx"), (2, "xy")):
        _same(_run(_stack(pairs, C.TILE_CAP, cols, ordering), ordering=ordering, **C.TILE_KW), out, (cols, ordering))


def test_every_pair_alone_and_reversed_slots(tile):
    pairs, out, alone = tile
    for k in range(len(pairs)):
        _same(alone[k], _row(out, k), k)
    _same(_run(_stack(pairs[::-1], C.TILE_CAP), **C.TILE_KW), [x[::-1] for x in out])


def test_nmatch_past_cap_is_clamped(tile):
    pairs, out, _ = tile
    full = [k for k, p in enumerate(pairs) if len(p[0]) == C.TILE_CAP]
    assert full
    nm = [len(p[0]) for p in pairs]
    for k in full:
        nm[k] = C.TILE_CAP + 7
    _same(_run(_stack(pairs, C.TILE_CAP, nmatch=nm), **C.TILE_KW), out)


def test_without_ground_truth(tile):
    pairs, out, _ = tile
    R, t, mask, status, rows = _run(_stack(pairs, C.TILE_CAP, T=False), **C.TILE_KW)
    _same((R, t, mask, status, rows[:, 3]), (out[0], out[1], out[2], out[3], out[4][:, 3]))
    ok = status >= 0
    assert ok.sum() == 9 and np.all(np.isnan(rows[ok, :3])) and np.all(np.isinf(rows[~ok, :3]))


def test_batch_over_64_pairs(tile):
    """B = 130: three blocks of the one-lane-per-pair selection scan; slots 63 | 64 | 65 and 127 | 128 | 129 hold different pairs,
    slot 64 the "few" pair and slot 128 the "noE" pair.  Every slot equals the bits of its pair run alone."""
    pairs, _, alone = tile
    m = len(pairs)
    out = _run(_stack([pairs[b % m] for b in range(C.TILE_B)], C.TILE_CAP), **C.TILE_KW)
    assert out[3][64] == CODES["few"] and out[3][128] == CODES["noE"] and out[3][63] >= 0 and out[3][129] >= 0
    for b in range(C.TILE_B):
        _same(_row(out, b), alone[b % m], b)


# ------------------------------------------------------------------ round boundaries
def test_best_model_on_a_rounds_first_or_last_iteration():
    worst = 0.0
    for scene_seed, it, seed in C.BOUNDARY_SEEDS["pose"]:
        pair, r = C.boundary_ref("pose", scene_seed, seed)
        assert r["status"] == "ok" and r["it"][0] == it
        R, t, mask, status, rows = _row(_run(_stack([pair], 64), seed=seed, **C.BOUNDARY_KW), 0)
        n = len(pair[0])
        assert status >= 0 and (status >> 4) == it, (it, seed, status)
        assert np.array_equal(mask[:n], r["mask"]) and not mask[n:].any(), it
        d = max(np.abs(R - r["R"]).max(), min(np.abs(t - r["t"]).max(), np.abs(t + r["t"]).max()))
        worst = max(worst, d)
        assert _certificate(pair, dict(C.BOUNDARY_KW, seed=seed), (R, t, mask, status, rows), ("boundary", it)) <= CERT_GATE
    print(f"measured: boundary pairs max |dR|, |dt| = {worst:.3e}")
    assert worst < 1e-9


def test_max_iters_inside_a_round_equals_the_long_run(cases):
    """max_iters = 33 against max_iters = 300 wherever the restatement's chosen iteration is below 33: the shrinking bound makes
    the two scans identical, whatever the round schedule and the workspace layout"""
    idx = [i for i in sorted(cases) if C.POSE_CASES[i][4] == np.float32 and C.POSE_CASES[i][5] == C.IT300]
    idx = [i for i in idx if cases[i][2]["status"] == "ok" and cases[i][2]["it"][0] < 33]
    assert len(idx) >= 4
    cap = _cap_for(max(len(cases[i][0][0]) for i in idx))
    short = _run(_stack([cases[i][0] for i in idx], cap), max_iters=33)
    long = _run(_stack([cases[i][0] for i in idx], cap), max_iters=300)
    _same(short, long)
    for b, i in enumerate(idx):
        assert (long[3][b] >> 4) == cases[i][2]["it"][0]
    pair, kw, r, out, cap = cases[11]  # the max_iters = 33 case itself, alone at both lengths
    assert kw == {"max_iters": 33} and r["it"][0] < 33
    _same(_row(_run(_stack([pair], cap), max_iters=300), 0), out)


# ------------------------------------------------------------------ error epilogue
def test_error_epilogue_branches(cases):
    pair = cases[0][0]
    R, t = cases[0][3][:2]
    Tgt = pair[4].astype(np.float64)
    Ts = []
    for k in range(7):
        T = Tgt.copy()
        if k == 1:
            T[:3, 3] = 0.0                                  # t_gt = 0: NaN t_err, pose_err = R_err
        elif k == 2:
            T[:3, 3] = -t                                   # antiparallel: min(t_err, 180 - t_err) gives 0, not 180
        elif k == 3:
            T[0, 3] = np.inf                                # a non-finite t_gt: t_err = 0
        elif k == 4:
            T[1, 3] = np.nan
        elif k == 5:
            T[:3, :3] = R                                   # the cosine clips at +1
        elif k == 6:
            T[:3, :3] = R @ np.diag([1.0, -1.0, -1.0])      # turned by 180 degrees about x: the cosine clips at -1
        Ts.append(T)
    Ts = np.stack(Ts)
    for dt in (np.float64, np.float32):
        Td = Ts.astype(dt)
        args = list(_stack([pair] * len(Td), 64))
        args[5] = _t(Td)
        assert args[5].dtype == (torch.float64 if dt == np.float64 else torch.float32)
        Ro, to, mask, status, rows = _run(args, max_iters=300)
        with np.errstate(all="ignore"):
            want = np.array([P.pose_errors(Td[k], Ro[k], to[k]) for k in range(len(Td))])
        for k in range(len(Td)):
            assert np.array_equal(Ro[k], R) and np.array_equal(to[k], t) and status[k] == cases[0][3][3]
        assert np.array_equal(np.isnan(want), np.isnan(rows[:, :3])) and np.array_equal(np.isinf(want), np.isinf(rows[:, :3]))
        fin = np.isfinite(want)
        print(f"T {np.dtype(dt).name}: rows\n{rows[:, :3]}\nmax diff {np.abs(rows[:, :3][fin] - want[fin]).max():.3e}")
        assert np.abs(rows[:, :3][fin] - want[fin]).max() < 1e-5
        if dt == np.float64:  # each branch is the one its slot is there for
            assert np.isnan(rows[1, 1]) and rows[1, 2] == rows[1, 0]
            assert rows[2, 1] < 1e-5 and rows[3, 1] == 0.0 and rows[4, 1] == 0.0
            assert rows[5, 0] < 1e-5 and abs(rows[6, 0] - 180.0) < 1e-5
