"""The mutual-nearest-neighbour matcher restated in float64 numpy, and inputs on which fp32 computes it exactly.

Not collected by pytest (no test_ prefix).  tests/test_mnn_f64_cpu.py checks this restatement against the C oracle and the
reference's fixtures; tests/test_mnn_f64_gpu.py compares the kernels of csrc/mnn.hip / match_tiles.h / gemm_tile.h with it.

Why a second restatement: the C oracle mirrors the kernels (the same k-ordered fmaf chain, the same first-index rule), so a
mistake shared by both is invisible to `array_equal` between them.  This one shares nothing with either: `d0 @ d1.T` in float64,
numpy's arg-max, numpy's boolean algebra.

Why exact inputs: with the two families below every partial sum of every similarity is representable in fp32, so the fp32
similarity equals the float64 one bit for bit IN ANY SUMMATION ORDER (test_mnn_f64_cpu.py asserts that for every case list).
Matches, scores, second neighbours, the similarity matrix and every threshold decision are then compared with `array_equal`: no
tolerance, no margin, no skipped row.  Only `log_assignment` (exp / log) needs a bound."""
import zlib

import numpy as np

from helpers import synth

NEG_INF = -np.inf


# ------------------------------------------------------------------------------------------------ the restatement
def log_softmax(x, axis):
    mx = x.max(axis=axis, keepdims=True)
    e = x - mx
    return e - np.log(np.exp(e).sum(axis=axis, keepdims=True))


class Restated:
    """One pair.  d0 [n,D], d1 [m,D] (any float dtype; promoted to float64).

    sim            [n,m] float64
    best0 / best1  row / column arg-max, the FIRST index among equals (the project's rule, test_mnn_exact_ties_first_index_rule)
    sec0 / sec1    second neighbour as match_tiles.h MODE 4 documents it: the maximum over all OTHER indices (an equal value at
                   another index counts); NaN where there is no other index
    """

    def __init__(self, d0, d1):
        d0, d1 = np.asarray(d0, np.float64), np.asarray(d1, np.float64)
        self.n, self.m = d0.shape[0], d1.shape[0]
        self.sim = d0 @ d1.T
        n, m = self.n, self.m
        self.empty = n == 0 or m == 0
        if self.empty:
            self.best0, self.best1 = np.zeros((n,), np.int64), np.zeros((m,), np.int64)
            self.top0 = self.sec0 = np.full((n,), np.nan)
            self.top1 = self.sec1 = np.full((m,), np.nan)
            return
        self.best0 = self.sim.argmax(1)  # numpy: the first occurrence of the maximum
        self.best1 = self.sim.argmax(0)
        self.top0 = self.sim[np.arange(n), self.best0]
        self.top1 = self.sim[self.best1, np.arange(m)]
        rest = self.sim.copy()
        rest[np.arange(n), self.best0] = NEG_INF
        self.sec0 = rest.max(1) if m > 1 else np.full((n,), np.nan)
        rest = self.sim.copy()
        rest[self.best1, np.arange(m)] = NEG_INF
        self.sec1 = rest.max(0) if n > 1 else np.full((m,), np.nan)

    def _find_nn(self, best, top, sec, ratio, dist):
        """thresh_match of match_tiles.h: d = 2 (1 - sim); keep while d0 <= ratio^2 d2 (skipped with a single candidate) and
        d0 <= dist^2; the squared thresholds are rounded to fp32 once, as _native.mnn passes them."""
        ok = np.ones(best.shape, bool)
        d0 = 2.0 * (1.0 - top)
        if ratio and not np.isnan(sec).all():
            r2 = float(np.float32(float(ratio) ** 2))
            ok &= d0 <= r2 * (2.0 * (1.0 - sec))
        if dist:
            t2 = float(np.float32(float(dist) ** 2))
            ok &= d0 <= t2
        return np.where(ok, best, -1)

    def matches(self, ratio=None, dist=None):
        """-> matches0 [n] int64, matches1 [m] int64, scores0 [n] float32, scores1 [m] float32 after the mutual check"""
        n, m = self.n, self.m
        if self.empty:
            return np.full((n,), -1, np.int64), np.full((m,), -1, np.int64), np.zeros((n,), np.float32), np.zeros((m,), np.float32)
        f0 = self._find_nn(self.best0, self.top0, self.sec0, ratio, dist)
        f1 = self._find_nn(self.best1, self.top1, self.sec1, ratio, dist)
        m0 = np.where((f0 > -1) & (f1[np.maximum(f0, 0)] == np.arange(n)), f0, -1).astype(np.int64)
        m1 = np.where((f1 > -1) & (f0[np.maximum(f1, 0)] == np.arange(m)), f1, -1).astype(np.int64)
        return m0, m1, (m0 > -1).astype(np.float32), (m1 > -1).astype(np.float32)

    def log_assignment(self):
        """[n+1,m+1] float64: log_softmax(sim, -1) + log_softmax(sim, -2), zero dustbin row [n,:] and column [:,m]"""
        la = np.zeros((self.n + 1, self.m + 1))
        if not self.empty:
            la[:self.n, :self.m] = log_softmax(self.sim, 1) + log_softmax(self.sim, 0)
        return la


def matched_kpts(k0, k1, matches0, cols):
    """the matched keypoints, compacted in ascending i"""
    sel = np.nonzero(matches0 > -1)[0]
    return k0[sel][:, :cols], k1[matches0[sel]][:, :cols]


# ------------------------------------------------------------------------------------------------ exact input families
RESERVED = 16  # leading coordinates of the exact-unit family that only the threshold-equality rows use (D >= 32)


def exact_unit(seed, n, D):
    """[n,D] float32, every row exactly s entries of +-1/sqrt(s): s = 16 (+-0.25), or 4 (+-0.5) when D < 16.  Norms are exactly 1
    and every product of two entries is +-1/16 (+-1/4), so every similarity is a multiple of 1/16 in [-1, 1].  For D >= 32 the
    rows keep off the first RESERVED coordinates (see plant_threshold_equalities)."""
    r = np.random.default_rng(seed)
    s = 16 if D >= 16 else 4
    lo = RESERVED if D >= 2 * RESERVED else 0
    pos = np.argsort(r.random((n, D - lo)), axis=1)[:, :s] + lo
    sign = np.where(r.integers(0, 2, (n, s)) == 1, 1.0, -1.0)
    out = np.zeros((n, D), np.float32)
    np.put_along_axis(out, pos, (sign / np.sqrt(s)).astype(np.float32), axis=1)
    return out


def exact_dense(seed, n, D):
    """[n,D] float32, every entry a multiple of 1/8 in [-1, 1].  Products are multiples of 1/64 of magnitude <= 1, so for
    D <= 260 every partial sum is a multiple of 1/64 below 2^24 / 64: exact in fp32 in any order."""
    assert D <= 260
    r = np.random.default_rng(seed)
    return (r.integers(-8, 9, (n, D)) / 8.0).astype(np.float32)


def _special_rows(D):
    """Four unit rows on the RESERVED coordinates (zero similarity with every ordinary exact-unit row):
        a1 . b1 = 3/4, a2 . b2 = 1/2, a1 . b2 = a2 . b1 = 0
    Row a1 / column b1: best 3/4, every other similarity 0  ->  d0 = 1/2 = 0.5^2 x 2      (ratio 0.5 at equality)
    Row a2 / column b2: best 1/2, every other similarity 0  ->  d0 = 1   = 1.0^2          (distance 1.0 at equality)"""
    a1 = np.zeros((D,), np.float32)
    a1[:16] = 0.25
    a2 = a1.copy()
    a2[8:16] = -0.25
    b1 = a1.copy()
    b1[[0, 8]] *= -1
    b2 = a2.copy()
    b2[[1, 2, 9, 10]] *= -1
    return a1, a2, b1, b2


def plant_threshold_equalities(d0, d1, rows, cols):
    """rows = (i1, i2) of d0 and cols = (j1, j2) of d1 become the special rows; returns [(i1, j1), (i2, j2)]"""
    a1, a2, b1, b2 = _special_rows(d0.shape[1])
    d0[rows[0]], d0[rows[1]] = a1, a2
    d1[cols[0]], d1[cols[1]] = b1, b2
    return [(rows[0], cols[0]), (rows[1], cols[1])]


def make_pair(family, seed, n, m, D):
    """One pair of the family with planted structure.  Returns d0 [n,D], d1 [m,D] float32 and `info`:
    info["planted"]  (i, j) with d1[j] = d0[i]: real correspondences at permuted positions (spread over the whole index range, so in
                     a pair beyond 1024 keypoints they lie on both sides of index 1024)
    info["dups"]     rows overwritten with a copy of another row of the same side: exact ties in sim
    info["ratio_eq"] / info["dist_eq"]  (i, j) whose d0 equals ratio_sq d2 / dist_sq exactly (exact-unit family, D >= 32, n, m >= 8)"""
    gen = exact_unit if family == "unit" else exact_dense
    d0, d1 = gen(seed, n, D), gen(seed + 1, m, D)
    r = np.random.default_rng(seed + 2)
    info = {"planted": [], "dups": [], "ratio_eq": None, "dist_eq": None}
    k = min(n, m) // 3
    if k:
        src, dst = r.permutation(n)[:k], r.permutation(m)[:k]
        d1[dst] = d0[src]
        info["planted"] = list(zip(src.tolist(), dst.tolist()))
    if n >= 8:  # a later copy of a planted row: its column sees two equal maxima, the first index must win
        a, b = sorted(r.permutation(n)[:2].tolist())
        d0[b] = d0[a]
        info["dups"].append(("side0", a, b))
    if m >= 8:
        a, b = sorted(r.permutation(m)[:2].tolist())
        d1[b] = d1[a]
        info["dups"].append(("side1", a, b))
    if family == "unit" and D >= 2 * RESERVED and n >= 8 and m >= 8:
        # the last rows of each side, so that beyond 1024 keypoints the equalities are decided on a later trip too
        (p, q) = plant_threshold_equalities(d0, d1, (n - 1, n // 2), (m - 2, m // 3))
        info["ratio_eq"], info["dist_eq"] = p, q
    return d0, d1, info


# ------------------------------------------------------------------------------------------------ the GPU test's cases
# name -> (B, cap0, cap1, D, [(n, m) per pair], count tensor or None).  The smallest shapes that reach each path of the tile engine
# (BM = BN = 128, BK = 32) and of the 1024-thread finalize / gather loops; see test_mnn_f64_gpu.py.
CASES = {
    "tail_small": (3, 129, 257, 36, [(129, 257), (128, 1), (0, 200)], None),
    "tile_edge": (2, 128, 257, 64, [(128, 257), (127, 128)], None),
    "one_slab_d4": (2, 130, 130, 4, [(130, 130), (1, 130)], None),
    "one_slab_d32": (2, 130, 130, 32, [(130, 130), (1, 130)], None),
    "whole_fast": (2, 256, 256, 64, [(256, 256), (255, 256)], None),
    "whole_tail": (1, 256, 256, 260, [(256, 256)], None),
    "beyond_1024": (2, 1025, 2049, 32, [(1025, 2049), (700, 1500)], None),
    "beyond_1024_t": (2, 2049, 1025, 32, [(2049, 1025), (1500, 700)], None),
    "clamp": (1, 64, 64, 64, [(64, 64)], [(70, 64)]),
}
FAMILIES = ("unit", "dense")
# (ratio, distance): squares are dyadic, so ratio_sq * d2 is exact
THRESHOLDS = [(0.5, None), (0.75, None), (None, 0.5), (None, 1.0), (None, 1.5), (0.5, 1.5), (0.75, 1.0)]


class Case:
    """Padded arrays of one case: d0 [B,cap0,D], d1 [B,cap1,D], k0 [B,cap0,3], k1 [B,cap1,3] float32 with NaN in every row past a
    pair's count; n / m the true counts, n_arg / m_arg what the count tensors say (larger than the cap in `clamp`)."""


_CACHE = {}


def build_case(name, family):
    key = (name, family)
    if key in _CACHE:
        return _CACHE[key]
    B, cap0, cap1, D, counts, said = CASES[name]
    seed = zlib.crc32(name.encode()) % 100000 * 1000 + 100 * FAMILIES.index(family)  # of the name: adding a case moves no other
    c = Case()
    c.name, c.family, c.B, c.cap0, c.cap1, c.D = name, family, B, cap0, cap1, D
    c.d0 = np.full((B, cap0, D), np.nan, np.float32)
    c.d1 = np.full((B, cap1, D), np.nan, np.float32)
    c.k0 = np.full((B, cap0, 3), np.nan, np.float32)
    c.k1 = np.full((B, cap1, 3), np.nan, np.float32)
    c.n, c.m, c.info = [n for n, _ in counts], [m for _, m in counts], []
    for b, (n, m) in enumerate(counts):
        a0, a1, info = make_pair(family, seed + 10 * b, n, m, D)
        c.d0[b, :n], c.d1[b, :m] = a0, a1
        c.k0[b, :n] = synth.uniform(seed + 10 * b + 5, (n, 3), 0, 260)
        c.k1[b, :m] = synth.uniform(seed + 10 * b + 6, (m, 3), 0, 260)
        c.info.append(info)
    c.n_arg = [v[0] for v in said] if said else c.n
    c.m_arg = [v[1] for v in said] if said else c.m
    c.pairs = [Restated(c.d0[b, :c.n[b]], c.d1[b, :c.m[b]]) for b in range(B)]
    _CACHE[key] = c
    return c


def compact_case(B=300, cap=4, D=4):
    """B pairs of at most `cap` keypoints (exact-unit, D = 4: 16 distinct vectors, ties everywhere) with ragged counts: more
    pairs than compact_rows_kernel has threads, so its prefix loop takes a second trip."""
    r = np.random.default_rng(77)
    c = Case()
    c.name, c.family, c.B, c.cap0, c.cap1, c.D = "compact", "unit", B, cap, cap, D
    c.d0 = np.full((B, cap, D), np.nan, np.float32)
    c.d1 = np.full((B, cap, D), np.nan, np.float32)
    c.k0 = np.full((B, cap, 3), np.nan, np.float32)
    c.k1 = np.full((B, cap, 3), np.nan, np.float32)
    c.n = r.integers(0, cap + 1, B).tolist()
    c.m = r.integers(0, cap + 1, B).tolist()
    c.n[0], c.m[0], c.n[-1], c.m[-1] = cap, cap, cap, cap
    for b in range(B):
        n, m = c.n[b], c.m[b]
        c.d0[b, :n], c.d1[b, :m] = exact_unit(5000 + 2 * b, n, D), exact_unit(5001 + 2 * b, m, D)
        if n and m:
            c.d1[b, m - 1] = c.d0[b, 0]
        c.k0[b, :n] = synth.uniform(9000 + 2 * b, (n, 3), 0, 260)
        c.k1[b, :m] = synth.uniform(9001 + 2 * b, (m, 3), 0, 260)
    c.n_arg, c.m_arg = c.n, c.m
    c.pairs = [Restated(c.d0[b, :c.n[b]], c.d1[b, :c.m[b]]) for b in range(B)]
    return c


def matcher_pair(n=1100, m=1300, D=64):
    """one exact-unit pair beyond 1024 keypoints on both sides, for the NearestNeighborMatcher module"""
    d0, d1, info = make_pair("unit", 424242, n, m, D)
    k0, k1 = synth.uniform(31, (n, 3), 0, 260), synth.uniform(32, (m, 3), 0, 260)
    return d0, d1, k0, k1, info


def exactness_lists():
    """(tag, d0 [n,D], d1 [m,D]) of every pair the GPU test feeds the kernels"""
    out = []
    for name in CASES:
        for fam in FAMILIES:
            c = build_case(name, fam)
            for b in range(c.B):
                out.append((f"{name}.{fam}.{b}", c.d0[b, :c.n[b]], c.d1[b, :c.m[b]]))
    cc = compact_case()
    for b in range(cc.B):
        out.append((f"compact.{b}", cc.d0[b, :cc.n[b]], cc.d1[b, :cc.m[b]]))
    d0, d1, _, _, _ = matcher_pair()
    out.append(("matcher_pair", d0, d1))
    return out
