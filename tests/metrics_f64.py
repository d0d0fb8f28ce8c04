"""The pair metrics (MatchingRatio, MeanMatchingAccuracy@t, Repeatability / ValidDescriptorsDistance@t) restated in float64 numpy,
and inputs on which fp32 computes every decision of them exactly.

Not collected by pytest (no test_ prefix).  tests/test_metrics_f64_cpu.py checks this restatement against the C oracle and the
reference's fixtures; tests/test_metrics_f64_gpu.py compares the kernels of csrc/metrics.hip with it.

Why a second restatement: the C oracle mirrors the kernels (the same fmaf chains, the same fp32 cofactor inverse, the same
strict-`<` first-index rule, the same einx_acosf), so a mistake shared by both is invisible to a comparison between them.  This
one is written from the reference's text (core/metrics/util.py:5-104, keypoints_metrics.py:54-157 and :160-290,
matching_metrics.py:30-51 and :84-156) and shares nothing with either: `H @ [x; y; 1]` and the division, numpy's inverse, the
[N1, N2] norm matrix over the kept points, numpy's arg-min.

Why exact inputs: keypoints on a lattice of halves, homographies with dyadic entries and a power-of-two determinant, descriptors
whose products are multiples of 1/64.  Every warp, every visibility test, every squared distance and every descriptor sum is then
representable in fp32, so fp32 equals float64 bit for bit at every decision (test_metrics_f64_cpu.py asserts that for every case),
and exact distance ties, distances equal to a threshold and warped coordinates equal to 0 / W / H can be planted.  Counts,
neighbours, distances and every quotient of counts are compared with `array_equal`; only the angle (acos) needs a bound."""
import zlib

import numpy as np

from mnn_f64 import exact_unit

SIZE0, SIZE1 = (48, 64), (40, 56)  # (H, W) of image 0 / image 1: different and not square
THRESHOLDS = (1, 2.5, 3, 5)


# ------------------------------------------------------------------------------------------------ the restatement
def warp(points, H):
    """util.py:5-39: points [2,N] (x row, y row) -> [2,N]"""
    homogeneous = H @ np.vstack((points[:2], np.ones((1, points.shape[1]))))
    return np.vstack((homogeneous[0] / homogeneous[2], homogeneous[1] / homogeneous[2]))


def filter_points(points, img_shape):
    """util.py:43-70: the mask alone; img_shape = (H, W)"""
    return (points[0] >= 0) & (points[0] < img_shape[1]) & (points[1] >= 0) & (points[1] < img_shape[0])


def _desc_records(v1, v2):
    """keypoints_metrics.py:248-256 per row: squared distance, distance, angle in degrees (v1 of image 0, v2 of image 1)"""
    sq = ((v1 - v2) ** 2).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = (v1 * v2).sum(1) / (np.sqrt((v1 * v1).sum(1)) * np.sqrt((v2 * v2).sum(1)))
        return sq, np.sqrt(sq), np.degrees(np.arccos(cos))


class Restated:
    """One pair.  k0 [n,>=2], k1 [m,>=2] keypoint rows ((y, x, ..) if kp_yx else (x, y, ..)), d0 [n,D], d1 [m,D], mk0 / mk1 [M,2|3]
    matched rows in the same convention, size0 / size1 = (H, W), hom [3,3] or None (identity).  Everything is promoted to float64.

    warped0 [n,2]      every keypoint of image 0 warped by H (x, y)
    keep0 [n], keep1 [m], N1, N2   the visibility masks (image 0's points inside size1 after H, image 1's inside size0 after H^-1)
    near_d[s] / near_j[s] / near_sq[s]   per keypoint of side s: distance to the nearest kept keypoint of the other image, its index
                       in that image's ORIGINAL numbering (the first among equals) and the exact squared distance; +inf / -1 / NaN
                       where the keypoint is filtered out or the other side keeps nothing
    desc_sq[s] / desc_d[s] / angle[s]    of that pair of descriptors: |v1 - v2|^2, |v1 - v2|, the angle in degrees (NaN where none)
    mma_d [M]          |warp(mk0) - mk1| per match"""

    def __init__(self, k0, k1, d0, d1, mk0, mk1, size0, size1, hom=None, kp_yx=True):
        f = lambda a: np.asarray(a, np.float64)  # noqa: E731
        xy = [1, 0] if kp_yx else [0, 1]
        k0, k1, mk0, mk1 = f(k0), f(k1), f(mk0), f(mk1)
        self.n, self.m, self.M = k0.shape[0], k1.shape[0], mk0.shape[0]
        self.H = np.eye(3) if hom is None else f(hom).reshape(3, 3)
        self.Hinv = np.linalg.inv(self.H)
        p1, p2 = k0[:, xy].T, k1[:, xy].T  # [2,n], [2,m]
        w1 = warp(p1, self.H)
        self.warped0 = w1.T
        self.keep1 = filter_points(warp(p2, self.Hinv), size0)
        self.keep0 = filter_points(w1, size1)
        self.N1, self.N2 = int(self.keep0.sum()), int(self.keep1.sum())
        a, b = self.warped0[self.keep0], p2.T[self.keep1]
        sq = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)  # [N1,N2]
        self.norm_sq, self.norm = sq, np.sqrt(sq)
        counts = (self.n, self.m)
        self.near_d = [np.full((c,), np.inf) for c in counts]
        self.near_j = [np.full((c,), -1, np.int64) for c in counts]
        self.near_sq, self.desc_sq, self.desc_d, self.angle = ([np.full((c,), np.nan) for c in counts] for _ in range(4))
        if self.N1 and self.N2:
            d0, d1 = f(d0), f(d1)
            orig0, orig1 = np.nonzero(self.keep0)[0], np.nonzero(self.keep1)[0]
            i1 = self.norm.argmin(1)  # numpy: the first occurrence of the minimum
            i0 = self.norm.argmin(0)
            rows, cols = np.arange(self.N1), np.arange(self.N2)
            self.near_d[0][orig0], self.near_sq[0][orig0], self.near_j[0][orig0] = self.norm[rows, i1], sq[rows, i1], orig1[i1]
            self.near_d[1][orig1], self.near_sq[1][orig1], self.near_j[1][orig1] = self.norm[i0, cols], sq[i0, cols], orig0[i0]
            self.desc_sq[0][orig0], self.desc_d[0][orig0], self.angle[0][orig0] = _desc_records(d0[orig0], d1[orig1[i1]])
            self.desc_sq[1][orig1], self.desc_d[1][orig1], self.angle[1][orig1] = _desc_records(d0[orig0[i0]], d1[orig1])
        dm = warp(mk0[:, xy].T, self.H).T - mk1[:, xy]
        self.mma_d = np.sqrt((dm ** 2).sum(1))

    def selected(self, t):
        """the records within t: boolean masks over image 0's and image 1's keypoints"""
        return self.near_d[0] <= t, self.near_d[1] <= t

    def row(self, mma_thr=(1, 3), vdd_thr=(1, 3), rep_nan_if_empty=False):
        """[MR, MMA@t.., (Repeatability, ValidDistance, Angle)@t..] float64.  MMA and repeatability are fp32 quotients of counts
        (`mask.float().mean()`, an integer tensor divided by an integer); the distances are summed as the fp32 values
        torch.linalg.norm returns; (0, 0, 0) when either side keeps nothing, 0 / 0 = NaN when both keep points but none is within t.
        rep_nan_if_empty: Repeatability's own class reports no entry when N1 + N2 == 0, marked with NaN."""
        out = [self.M / (min(self.n, self.m) + 1e-8)]
        for t in mma_thr:
            out.append(float(np.float32((self.mma_d <= t).sum()) / np.float32(self.M)) if self.M > 0 else 0.0)
        for t in vdd_thr:
            rep = vd = ang = 0.0
            if self.N1 != 0 and self.N2 != 0:
                s0, s1 = self.selected(t)
                c = np.float64(s0.sum() + s1.sum())
                rep = float(np.float32(c) / np.float32(self.N1 + self.N2))
                dist = np.concatenate([self.desc_d[0][s0], self.desc_d[1][s1]]).astype(np.float32).astype(np.float64)
                with np.errstate(invalid="ignore"):
                    vd = float(dist.sum() / c)
                    ang = float(np.concatenate([self.angle[0][s0], self.angle[1][s1]]).sum() / c)
            if rep_nan_if_empty and self.N1 + self.N2 == 0:
                rep = float("nan")
            out += [rep, vd, ang]
        return np.array(out, np.float64)


# ------------------------------------------------------------------------------------------------ exact homographies
HOM_KINDS = ("identity", "shift", "double", "half", "swap", "c2")
HOM_SHIFT = {"identity": (0, 0), "shift": (5, -3), "double": (-20, -10), "half": (6, 4), "swap": (3, -6), "c2": (2, -3)}


def homography(kind, tx=None, ty=None):
    """[3,3] float64, all entries dyadic, determinant +- a power of two, bottom row (0, 0, c) with c in {1, 2}; (tx, ty) an integer
    translation.  "c2" with (2, -3) is [[2,0,4],[0,2,-6],[0,0,2]]."""
    if tx is None:
        tx, ty = HOM_SHIFT[kind]
    if kind == "identity":
        return np.eye(3)
    if kind == "shift":
        return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)
    if kind == "double":
        return np.array([[2, 0, tx], [0, 2, ty], [0, 0, 1]], np.float64)
    if kind == "half":
        return np.array([[0.5, 0, tx], [0, 0.5, ty], [0, 0, 1]], np.float64)
    if kind == "swap":
        return np.array([[0, 1, tx], [1, 0, ty], [0, 0, 1]], np.float64)
    assert kind == "c2"
    return np.array([[2, 0, 2 * tx], [0, 2, 2 * ty], [0, 0, 2]], np.float64)


def adjugate_inverse(H):
    """the adjugate divided by the determinant, entry by entry: exact in float64 for the homographies above"""
    c = lambda i, j: H[(i + 1) % 3, (j + 1) % 3] * H[(i + 2) % 3, (j + 2) % 3] - H[(i + 1) % 3, (j + 2) % 3] * H[(i + 2) % 3, (j + 1) % 3]  # noqa: E731
    cof = np.array([[c(i, j) for j in range(3)] for i in range(3)])
    det = H[0, 0] * cof[0, 0] + H[0, 1] * cof[0, 1] + H[0, 2] * cof[0, 2]
    return cof.T / det, det


# ------------------------------------------------------------------------------------------------ exact input families
def exact_dense(seed, n, D):
    """[n,D] float32, every entry a multiple of 1/8 in [-1, 1], no zero row.  Products are multiples of 1/64 of magnitude <= 4
    ((x1 - x2)^2), so for D <= 600 every partial sum is a multiple of 1/64 below 2^24 / 64: exact in fp32 in any order."""
    assert 36 <= D <= 600
    r = np.random.default_rng(seed)
    out = (r.integers(-8, 9, (n, D)) / 8.0).astype(np.float32)
    out[:, 0] = np.where((out != 0).any(1), out[:, 0], 1.0)
    return out


# offsets (dx, dy) on the lattice of halves.  AT[t]: distance exactly t; ABOVE[t]: the smallest lattice distance beyond t (4 d^2 is
# a sum of two squares: 5 after 4, 26 after 25, 37 after 36, 101 after 100), so nothing on the lattice lies between t and it
AT = {1: (1.0, 0.0), 2.5: (1.5, 2.0), 3: (0.0, 3.0), 5: (3.0, 4.0)}
ABOVE = {1: (0.5, 1.0), 2.5: (0.5, 2.5), 3: (0.5, 3.0), 5: (0.5, 5.0)}
# equidistant candidates: index offsets (first, second) from a base j.  The first minimum is the smaller index.
TIE_PATTERNS = {"slots": (0, 64),    # the same lane in two slots of one trip
                "trips": (0, 256),   # the same lane in two trips
                "lanes": (0, 1),     # neighbouring lanes
                "cross": (64, 1)}    # the lower lane holds the larger index
TIE_OFFSETS = [((1.0, 0.0), (-1.0, 0.0)), ((0.0, 1.0), (0.0, -1.0)), ((1.0, 1.0), (-1.0, 1.0)), ((1.0, -1.0), (1.0, 1.0))]


def _zone(H, size0, size1):
    """the half-open rectangle [x0, x1) x [y0, y1) of image 1's frame in which a point of either image is kept: image 1 itself
    intersected with H(image 0) (a rectangle again for the homographies above)"""
    c = warp(np.array([[0.0, size0[1]], [0.0, size0[0]]]), H)
    return (max(0.0, c[0].min()), min(float(size1[1]), c[0].max()), max(0.0, c[1].min()), min(float(size1[0]), c[1].max()))


class _Layout:
    """Positions of one pair in image 1's frame: A [n,2] the warped keypoints of image 0, B [m,2] the keypoints of image 1 (x, y).
    A structure is one keypoint (the owner) with planted nearest candidates on the other side; nothing else of the other side may
    come as near, which placement and the background's rejection sampling guarantee."""

    def __init__(self, r, n, m, H, step_a):
        self.r, self.H, self.step = r, H, (step_a, 0.5)
        self.P = [np.full((n, 2), np.nan), np.full((m, 2), np.nan)]
        self.free = [list(r.permutation(n)), list(r.permutation(m))]
        self.zone = _zone(H, SIZE0, SIZE1)
        self.structs = []  # (owner side, centre, squared radius)

    def _inside(self, p):
        x0, x1, y0, y1 = self.zone
        return x0 <= p[0] < x1 and y0 <= p[1] < y1

    def _clear(self, side, p):
        """may a point of `side` sit at p: strictly farther from the owner of every structure whose candidates are of that side
        than the planted candidates are (on the rim it would be one more equidistant candidate)"""
        return all(s == side or ((p - c) ** 2).sum() > r2 for s, c, r2 in self.structs)

    def draw(self, side, box=None):
        x0, x1, y0, y1 = box or self.zone
        st = self.step[side]
        return np.array([self.r.integers(np.ceil(x0 / st), np.ceil(x1 / st)), self.r.integers(np.ceil(y0 / st), np.ceil(y1 / st))]) * st

    def take(self, side, idx=None):
        """an unused index of `side` (a given one, or any); None when there is none"""
        if idx is None:
            return self.free[side].pop() if self.free[side] else None
        if idx in self.free[side]:
            self.free[side].remove(idx)
            return idx
        return None

    def give_back(self, side, idx):
        self.free[side].append(idx)

    def place(self, side, owner, cands, offsets, tries=400):
        """owner (index of `side`) at a centre, cands (indices of the other side) at centre + offset; True when a place was found"""
        o = 1 - side
        offsets = [np.array(v) for v in offsets]
        r2 = float((offsets[0] ** 2).sum())
        assert all(float((v ** 2).sum()) == r2 for v in offsets)
        for _ in range(tries):
            # draw the point of image 0 on its own (coarser) lattice, derive the others from it
            c = self.draw(0) if side == 0 else self.draw(0) - offsets[0]
            pts = [c + v for v in offsets]
            if not (self._inside(c) and all(self._inside(p) for p in pts)):
                continue
            if any(np.modf(p / self.step[o])[0].any() for p in pts) or np.modf(c / self.step[side])[0].any():
                continue
            placed = self.P[o][~np.isnan(self.P[o][:, 0])]
            if (((placed - c) ** 2).sum(1) <= r2).any():
                continue  # an earlier point of the other side would be as near as the planted ones
            if not (self._clear(side, c) and all(self._clear(o, p) for p in pts)):
                continue
            self.P[side][owner] = c
            for j, p in zip(cands, pts):
                self.P[o][j] = p
            self.structs.append((side, c, r2))
            return True
        return False

    def fill(self, side, idx, make):
        """point `idx` of `side` from make() until it is clear of every structure"""
        for _ in range(400):
            p = make()
            if p is not None and self._clear(side, p):
                self.P[side][idx] = p
                return True
        return False


def make_pair(family, seed, n, m, nmatch, D, hom, cols, kp_yx):
    """One pair with planted structure.  hom = (kind, tx, ty) or None (the null pointer: identity).  Returns float32 arrays
    k0 [n,3], k1 [m,3], d0 [n,D], d1 [m,D], mk0 / mk1 [nmatch,cols], the float64 homography and `info`:
      info["ties"]    (side, owner, first, second, pattern): keypoint `owner` of `side` has the other image's keypoints `first` and
                      `second` at the same, smallest distance; `first` is the smaller index
      info["at"] / info["above"]   (side, owner, candidate, t): the nearest distance is exactly t / the next lattice distance
      info["corr"]    (i, j): image 0's keypoint i warps exactly onto image 1's keypoint j"""
    r = np.random.default_rng(seed)
    kind = "identity" if hom is None else hom[0]
    H = homography(*hom) if hom is not None else np.eye(3)
    Hinv, _ = adjugate_inverse(H)
    L = _Layout(r, n, m, H, 1.0 if kind == "double" else 0.5)  # "double": image 0's halves warp onto whole numbers
    info = {"ties": [], "at": [], "above": [], "corr": [], "kind": kind}
    cnt = (n, m)

    def plant(side, cands_idx, offsets, owner=None):
        o = 1 - side
        own = L.take(side, owner)
        got = [L.take(o, j) for j in cands_idx]
        if own is not None and None not in got and L.place(side, own, got, offsets):
            return own, got
        for s, i in [(side, own)] + [(o, j) for j in got]:
            if i is not None:
                L.give_back(s, i)
        return None

    if n >= 2 and m >= 2:  # the last keypoints of both images correspond: beyond 512 where a side has that many
        p = plant(0, [m - 1], [(0.0, 0.0)], owner=n - 1)
        if p:
            info["corr"].append((n - 1, m - 1))
    def tie(side, k, name):
        first, second = TIE_PATTERNS[name]
        span, other_n = max(first, second), cnt[1 - side]
        for _ in range(8 if other_n > span else 0):
            j = int(r.integers(0, other_n - span))
            p = plant(side, [j + first, j + second], TIE_OFFSETS[(k + side) % 4])
            if p:
                a, b = sorted(p[1])
                info["ties"].append((side, p[0], a, b, name))
                return

    def threshold(side, key, t):
        p = plant(side, [None], [(AT if key == "at" else ABOVE)[t]])
        if p:
            info[key].append((side, p[0], p[1][0], t))

    plans = [(tie, (side, k, name)) for side in (0, 1) for k, name in enumerate(TIE_PATTERNS)]
    plans += [(threshold, (side, key, t)) for side in (0, 1) for t in THRESHOLDS for key in ("at", "above")]
    if min(n, m) <= 16:  # too few keypoints for all of it: another part in every pair
        plans = [plans[i] for i in r.permutation(len(plans))]
    for fn, args in plans:
        fn(*args)
    for _ in range(min(n, m) // 4):
        p = plant(0, [None], [(0.0, 0.0)])
        if p:
            info["corr"].append((p[0], p[1][0]))
    # warped coordinates exactly 0, W, H and W - 1/2 (image 0 through H into image 1's frame, image 1 through H^-1 into image 0's)
    W1, H1, W0, H0 = SIZE1[1], SIZE1[0], SIZE0[1], SIZE0[0]
    edge_a = [lambda: np.array([0.0, L.draw(0)[1]]), lambda: np.array([float(W1), L.draw(0)[1]]), lambda: np.array([L.draw(0)[0], float(H1)]),
              lambda: np.array([W1 - 0.5, L.draw(0)[1]]) if L.step[0] == 0.5 else None, lambda: np.array([L.draw(0)[0], 0.0]),
              # and outside on every side
              lambda: np.array([-2.0, L.draw(0)[1]]), lambda: np.array([W1 + 2.0, L.draw(0)[1]]), lambda: np.array([L.draw(0)[0], -2.0]),
              lambda: np.array([L.draw(0)[0], H1 + 2.0])]

    def from_image0(q):  # image 1's keypoint whose inverse warp is q, when it lies on the lattice of halves
        p = warp(q.reshape(2, 1), H)[:, 0]
        return p if not np.modf(p * 2)[0].any() else None

    y0 = lambda: float(r.integers(1, H0 - 1))  # noqa: E731
    x0 = lambda: float(r.integers(1, W0 - 1))  # noqa: E731
    edge_b = [lambda: from_image0(np.array([0.0, y0()])), lambda: from_image0(np.array([float(W0), y0()])),
              lambda: from_image0(np.array([x0(), float(H0)])), lambda: from_image0(np.array([W0 - 0.5, y0()])),
              lambda: from_image0(np.array([x0(), 0.0])),
              lambda: from_image0(np.array([-2.0, y0()])), lambda: from_image0(np.array([W0 + 2.0, y0()])),
              lambda: from_image0(np.array([x0(), -2.0])), lambda: from_image0(np.array([x0(), H0 + 2.0]))]
    for side, edges in ((0, edge_a), (1, edge_b)):
        if len(L.free[side]) >= 2 * len(edges):
            for make in edges:
                idx = L.take(side)
                if not L.fill(side, idx, make):
                    L.give_back(side, idx)
    # the rest: anywhere on the lattice up to 4 beyond image 1, so a share lies outside on every side
    box = (-4.0, W1 + 4.5, -4.0, H1 + 4.5)
    for side in (0, 1):
        while L.free[side]:
            idx = L.take(side)
            assert L.fill(side, idx, lambda: L.draw(side, box))
    A, B = L.P
    assert not np.isnan(A).any() and not np.isnan(B).any()
    p0 = warp(A.T, Hinv).T if n else A  # image 0's own coordinates
    xy = [1, 0] if kp_yx else [0, 1]
    k0, k1 = np.zeros((n, 3), np.float32), np.zeros((m, 3), np.float32)
    k0[:, xy], k1[:, xy] = p0, B
    k0[:, 2], k1[:, 2] = r.random(n), r.random(m)
    # descriptors
    gen = (lambda s, c: exact_unit(s, c, D)) if family == "unit" else (lambda s, c: exact_dense(s, c, D))
    d0, d1 = gen(seed + 1, n), gen(seed + 2, m)
    if family == "unit":  # identical descriptors on the correspondences: quotient exactly 1, angle exactly 0
        for i, j in info["corr"]:
            d1[j] = d0[i]
    for side, own, a, b, _ in info["ties"]:  # different descriptor distances on the tied candidates: a wrong choice shows
        mine, theirs = (d0, d1) if side == 0 else (d1, d0)
        sq = lambda j: float(((mine[own].astype(np.float64) - theirs[j]) ** 2).sum())  # noqa: E731
        for k in range(64):
            if sq(a) != sq(b):
                break
            theirs[b] = gen(seed + 100 + k, 1)[0]
    # matches: image 0's row on its lattice, image 1's row at the warp plus an offset from the threshold tables (or any)
    special = [(0.0, 0.0)] + list(AT.values()) + list(ABOVE.values())
    mk0, mk1 = np.zeros((nmatch, cols), np.float32), np.zeros((nmatch, cols), np.float32)
    for i in range(nmatch):
        w = L.draw(0, (0.0, float(W1), 0.0, float(H1)))
        off = np.array(special[int(r.integers(len(special)))]) if r.random() < 0.6 else r.integers(-12, 13, 2) * 0.5
        if r.random() < 0.5:
            off = -off[::-1]
        mk0[i, :2][xy], mk1[i, :2][xy] = warp(w.reshape(2, 1), Hinv)[:, 0], w + off
    if cols == 3:
        mk0[:, 2], mk1[:, 2] = r.random(nmatch), r.random(nmatch)
    return k0, k1, d0, d1, mk0, mk1, H, info


# ------------------------------------------------------------------------------------------------ the GPU test's cases
# name -> (B, cap0, cap1, D, [(n, m, nmatch) per pair], said counts [(n, m, nmatch) per pair] or None).  The smallest shapes that
# reach each path of metric_nearest_kernel (64 lanes x 4 slots of candidates / channels per trip), of metric_mma_kernel (256
# matches per block) and the per-pair indexing; see test_metrics_f64_gpu.py.
CASES = {
    "lane_tail": (3, 65, 130, 36, [(65, 130, 40), (64, 1, 1), (0, 100, 0)], None),
    "trip_edge": (2, 256, 257, 64, [(256, 257, 100), (255, 256, 255)], None),
    "three_trips": (2, 513, 300, 32, [(513, 300, 200), (260, 40, 30)], None),
    "d4": (2, 20, 30, 4, [(20, 30, 10), (7, 5, 3)], None),
    "d257": (2, 30, 40, 257, [(30, 40, 12), (9, 17, 5)], None),
    "d260": (2, 24, 24, 260, [(24, 20, 8), (11, 24, 4)], None),
    "d600": (2, 16, 20, 600, [(16, 20, 6), (10, 9, 9)], None),
    "matches_beyond_256": (2, 320, 16, 36, [(10, 12, 300), (8, 6, 0)], None),
    "clamp": (2, 64, 64, 64, [(64, 64, 64), (30, 64, 64)], [(70, 64, 80), (30, 70, 64)]),
    "many_pairs": (70, 8, 8, 40, None, None),  # ragged counts 0..8, drawn in build_case
}
# name -> kp_yx, columns of the matched rows, MMA thresholds, VDD thresholds, homography kind per pair (None: the null pointer)
SETTINGS = {
    "lane_tail": dict(kp_yx=True, cols=3, mma=(1, 3, 5), vdd=(1, 3), homs=("identity", "shift", "double")),
    "trip_edge": dict(kp_yx=False, cols=2, mma=(3,), vdd=(1, 2.5, 3, 5), homs=("half", "swap")),
    "three_trips": dict(kp_yx=True, cols=3, mma=(1, 2.5, 3, 5), vdd=(2.5, 5), homs=("c2", "shift")),
    "d4": dict(kp_yx=False, cols=2, mma=(1,), vdd=(3,), homs=None),
    "d257": dict(kp_yx=True, cols=3, mma=(3, 5, 1), vdd=(1, 5), homs=("double", "half")),
    "d260": dict(kp_yx=False, cols=3, mma=(), vdd=(1, 2.5, 3, 5), homs=("swap", "c2")),
    "d600": dict(kp_yx=True, cols=2, mma=(1, 2.5, 3, 5), vdd=(3,), homs=("shift", "identity")),
    "matches_beyond_256": dict(kp_yx=True, cols=2, mma=(1, 2.5, 3, 5), vdd=(), homs=("double", "swap")),
    "clamp": dict(kp_yx=False, cols=3, mma=(2.5,), vdd=(1, 3), homs=("c2", "half")),
    "many_pairs": dict(kp_yx=True, cols=3, mma=(3,), vdd=(1, 3), homs="all different"),
}
FAMILIES = ("unit", "dense")


def families_of(name):
    """the dense family only for D >= 36"""
    return FAMILIES if CASES[name][3] >= 36 else ("unit",)


CASE_IDS = [(name, fam) for name in CASES for fam in families_of(name)]


def _many_pairs(seed, B, cap):
    r = np.random.default_rng(seed)
    counts = [(int(a), int(b), int(c)) for a, b, c in r.integers(0, cap + 1, (B, 3))]
    counts[0], counts[1], counts[2], counts[-1] = (cap, cap, cap), (0, 0, 0), (0, cap, 0), (cap, cap, cap)
    homs = []
    for b in range(B):  # six kinds x a translation of its own: no two pairs share a homography
        kind = HOM_KINDS[1 + b % 5]
        tx, ty = HOM_SHIFT[kind]
        homs.append((kind, tx + b // 5 - 6, ty + (b // 5) % 3))
    homs[0] = ("identity", 0, 0)
    return counts, homs


class Case:
    """Padded arrays of one case: k0 [B,cap0,3], k1 [B,cap1,3], d0 [B,cap0,D], d1 [B,cap1,D], mk0 / mk1 [B,cap0,cols] float32 with
    NaN in every row past a pair's count, hom [B,3,3] float32 or None; n / m / nm the true counts, n_arg / m_arg / nm_arg what the
    count tensors say (larger than the capacities in `clamp`); pairs[b] the restatement of pair b."""

    def row(self, b, rep_nan_if_empty=False):
        return self.pairs[b].row(self.mma, self.vdd, rep_nan_if_empty)

    def pair_inputs(self, b):
        """the unpadded arrays of pair b, as oracle.pair_metrics and Restated take them"""
        n, m, M = self.n[b], self.m[b], self.nm[b]
        return self.k0[b, :n], self.k1[b, :m], self.d0[b, :n], self.d1[b, :m], self.mk0[b, :M], self.mk1[b, :M]


_CACHE = {}


def build_case(name, family):
    key = (name, family)
    if key in _CACHE:
        return _CACHE[key]
    B, cap0, cap1, D, counts, said = CASES[name]
    s = SETTINGS[name]
    seed = zlib.crc32(name.encode()) % 100000 * 1000 + 100 * FAMILIES.index(family)  # of the name: adding a case moves no other
    homs = s["homs"]
    if name == "many_pairs":
        counts, homs = _many_pairs(seed + 7, B, cap0)
    elif homs is not None:
        homs = [(k,) + HOM_SHIFT[k] for k in homs]
    c = Case()
    c.name, c.family, c.B, c.cap0, c.cap1, c.D = name, family, B, cap0, cap1, D
    c.kp_yx, c.cols, c.mma, c.vdd = s["kp_yx"], s["cols"], s["mma"], s["vdd"]
    c.size0, c.size1 = SIZE0, SIZE1
    c.k0, c.k1 = np.full((B, cap0, 3), np.nan, np.float32), np.full((B, cap1, 3), np.nan, np.float32)
    c.d0, c.d1 = np.full((B, cap0, D), np.nan, np.float32), np.full((B, cap1, D), np.nan, np.float32)
    c.mk0, c.mk1 = np.full((B, cap0, c.cols), np.nan, np.float32), np.full((B, cap0, c.cols), np.nan, np.float32)
    c.hom = None if homs is None else np.zeros((B, 3, 3), np.float32)
    c.n, c.m, c.nm = [v[0] for v in counts], [v[1] for v in counts], [v[2] for v in counts]
    c.info, c.pairs = [], []
    for b, (n, m, M) in enumerate(counts):
        k0, k1, d0, d1, mk0, mk1, H, info = make_pair(family, seed + 10 * b, n, m, M, D, None if homs is None else homs[b], c.cols, c.kp_yx)
        c.k0[b, :n], c.k1[b, :m], c.d0[b, :n], c.d1[b, :m], c.mk0[b, :M], c.mk1[b, :M] = k0, k1, d0, d1, mk0, mk1
        if c.hom is not None:
            c.hom[b] = H
        c.info.append(info)
        c.pairs.append(Restated(k0, k1, d0, d1, mk0, mk1, c.size0, c.size1, None if c.hom is None else c.hom[b], c.kp_yx))
    c.n_arg, c.m_arg, c.nm_arg = ([v[i] for v in said] for i in range(3)) if said else (c.n, c.m, c.nm)
    _CACHE[key] = c
    return c


def class_pair(n=300, m=270, M=280, D=64):
    """one exact-unit pair beyond 256 keypoints per side with (y, x, score) rows, for the metric classes"""
    k0, k1, d0, d1, mk0, mk1, H, info = make_pair("unit", 515151, n, m, M, D, ("shift", 5, -3), 3, True)
    return k0, k1, d0, d1, mk0, mk1, H.astype(np.float32), info


def oracle_record_angles(oracle, v1, v2):
    """the C oracle's angle (degrees) of each descriptor pair v1[k], v2[k]: orc_pair_metrics on a pair of one keypoint each at the
    same place, whose Angle entry is the double-precision mean (a + a) / 2 = a of the two records' fp32 angle"""
    k = np.zeros((1, 3), np.float32)
    e = np.zeros((0, 3), np.float32)
    out = np.empty((len(v1),), np.float64)
    for i in range(len(v1)):
        out[i] = oracle.pair_metrics(k, k, v1[i:i + 1], v2[i:i + 1], e, e, (1, 1), (1, 1), None, mma_thr=(), vdd_thr=(1,))[3]
    return out


def record_pairs(c, b):
    """per side s of pair b of a case: (indices of the keypoints that have a record, v1 rows, v2 rows) -- v1 of image 0, v2 of image 1"""
    R = c.pairs[b]
    out = []
    for s in (0, 1):
        idx = np.nonzero(R.near_j[s] >= 0)[0]
        other = R.near_j[s][idx]
        d0, d1 = c.d0[b], c.d1[b]
        out.append((idx, d0[idx], d1[other]) if s == 0 else (idx, d0[other], d1[idx]))
    return out


def oracle_angle_error(oracle, c, b):
    """e_orc of pair b: max |oracle - float64| over the angle records of both sides (0.0 without records)"""
    R = c.pairs[b]
    e = 0.0
    for s, (idx, v1, v2) in enumerate(record_pairs(c, b)):
        if len(idx):
            e = max(e, float(np.abs(oracle_record_angles(oracle, v1, v2) - R.angle[s][idx]).max()))
    return e
