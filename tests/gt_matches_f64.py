"""Ground-truth labelling and matcher_metrics restated in dense numpy, and inputs on which fp32 computes them exactly.

Not collected by pytest (no test_ prefix).  tests/test_gt_matches_f64_cpu.py checks this restatement against the reference's
fixture and against tests/gt_matches_ref.py; tests/test_gt_matches_f64_gpu.py compares the kernels of csrc/gt_matches.hip with it.

Why a second restatement: gt_matches_ref.py follows the kernel's operation order in stage A and the kernel's running arg-min in
stage B, so a mistake shared by both is invisible.  This one is written from the reference's text (gt_generation.py:65-126 and
172-213, depth.py:9-60, the pinhole Camera / Pose it calls, lightglue.py:17-63) with dense [n,m] matrices, numpy's arg-min, a scatter
and two `where`s; it shares no code with gt_matches_ref's stage A or B (only `ints`, the integer hash every input comes from).

Why exact inputs: keypoints and projections on a lattice of quarter pixels below 512, depths k/64, power-of-two focal lengths,
signed-permutation rotations, dyadic translations and depths that put q.z on a power of two make every quantity the sampler, the
projection and the labelling compute representable in fp32.  Every function below takes the dtype it computes in; the CPU test
asserts that float32 and float64 agree bit for bit on every case, so the GPU test compares with array_equal: no tolerance, no
margin.  Only average_precision (a closed form on the device, the reference's cumulative sums here) has a bound."""
import numpy as np

from gt_matches_ref import ints

F64 = np.float64
IGNORE, UNMATCHED = -2, -1
EPS_Z = np.float32(1e-4)  # Camera.eps as a float32 tensor sees it


# ------------------------------------------------------------------------------------------------ the restatement: stage A
def sample_depth(xy, depth, dt=F64):
    """depth.py:9-25 for one view: xy [n,2] (x, y), depth [H,W] -> d [n], valid [n], info.

    Holes (<= 0 or NaN) become NaN; a bilinear sample with zero padding at the pixel coordinate ix = x - 0.5 (grid_sample's
    x / W * 2 - 1 followed by its ((g + 1) W - 1) / 2 is the identity in exact arithmetic); a NaN tap poisons the sum even at weight
    zero, and a NaN sum is replaced by the nearest pixel (half to even), 0 outside the map.  A tap outside the map is skipped
    (8e: "contributes 0"), so a point with every tap outside -- also a far, infinite or NaN coordinate -- samples 0.
    info: taps_outside [n] (0, 2, 3 or 4: a single tap cannot be outside a rectangle), fallback [n], nearest [n] (0 = a good pixel,
    1 = a hole, 2 = outside the map)."""
    xy, depth = np.asarray(xy, dt), np.asarray(depth, dt)
    H, W = depth.shape
    n = len(xy)
    with np.errstate(invalid="ignore"):
        dm = np.where(depth > 0, depth, dt(np.nan))
        ix, iy = xy[:, 0] - dt(0.5), xy[:, 1] - dt(0.5)
        x0, y0 = np.floor(ix), np.floor(iy)
        total, outside = np.zeros(n, dt), np.zeros(n, np.int64)

        def pixel(xx, yy):
            inmap = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            return inmap, dm[np.where(inmap, yy, 0).astype(np.int64), np.where(inmap, xx, 0).astype(np.int64)]

        for yy, wy in ((y0, y0 + dt(1) - iy), (y0 + dt(1), iy - y0)):
            for xx, wx in ((x0, x0 + dt(1) - ix), (x0 + dt(1), ix - x0)):
                inmap, tap = pixel(xx, yy)
                total = total + np.where(inmap, tap * (wx * wy), dt(0))
                outside += ~inmap
        inmap, tap = pixel(np.rint(ix), np.rint(iy))
        near = np.where(inmap, tap, dt(0))
        fallback = np.isnan(total)
        d = np.where(fallback, near, total).astype(dt)
        valid = ~np.isnan(d) & (d > 0)
    return d, valid, {"taps_outside": outside, "fallback": fallback, "nearest": np.where(inmap, np.isnan(tap).astype(np.int64), 2)}


def invert_pose(T, dt=F64):
    """Pose.inv: (R^T, -R^T t)"""
    T = np.asarray(T, dt)
    out = np.zeros((4, 4), dt)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -np.einsum("rk,k->r", T[:3, :3].T, T[:3, 3])
    out[3, 3] = 1
    return out


def project_side(xy, d, valid, K_self, K_other, T, dt=F64):
    """depth.py:37-60 with ccth=None: image2cam, times the depth, Pose.transform, pinhole cam2image of the other camera whose
    size is (2 cx, 2 cy).  -> proj [n,2], visible [n], info (front, inside, qz)"""
    xy, d, Ks, Ko, T = (np.asarray(a, dt) for a in (xy, d, K_self, K_other, T))
    eps = dt(EPS_Z)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c, f = np.array([Ks[0, 2], Ks[1, 2]], dt), np.array([Ks[0, 0], Ks[1, 1]], dt)
        co, fo = np.array([Ko[0, 2], Ko[1, 2]], dt), np.array([Ko[0, 0], Ko[1, 1]], dt)
        p3 = np.concatenate([(xy - c) / f, np.ones((len(xy), 1), dt)], 1) * d[:, None]
        q = np.einsum("nk,rk->nr", p3, T[:3, :3]) + T[:3, 3]  # p @ R^T + t
        front = q[:, 2] > eps
        z = np.maximum(q[:, 2], eps)  # clamp(min=eps): NaN stays NaN
        uv = q[:, :2] / z[:, None] * fo + co
        inside = ((uv >= 0) & (uv <= dt(2) * co - dt(1))).all(1)
    return uv.astype(dt), valid & front & inside, {"front": front, "inside": inside, "qz": q[:, 2]}


def project_pair(kp0, kp1, K0, K1, T01, T10=None, depth0=None, depth1=None, precomputed=None, dt=F64):
    """stage A of one pair, keypoints (x, y): the depth maps or precomputed = (d0, valid0, d1, valid1); T10 None: Pose.inv"""
    if precomputed is None:
        d0, v0, i0 = sample_depth(kp0, depth0, dt)
        d1, v1, i1 = sample_depth(kp1, depth1, dt)
    else:
        d0, v0, d1, v1 = precomputed
        d0, d1, v0, v1, i0, i1 = np.asarray(d0, dt), np.asarray(d1, dt), np.asarray(v0, bool), np.asarray(v1, bool), None, None
    T10 = invert_pose(T01, dt) if T10 is None else T10
    p01, vis0, s0 = project_side(kp0, d0, v0, K0, K1, T01, dt)
    p10, vis1, s1 = project_side(kp1, d1, v1, K1, K0, T10, dt)
    return {"depth_keypoints0": d0, "depth_keypoints1": d1, "valid0": v0, "valid1": v1, "proj_0to1": p01, "proj_1to0": p10,
            "visible0": vis0, "visible1": vis1, "sample0": i0, "sample1": i1, "side0": s0, "side1": s1}


# ------------------------------------------------------------------------------------------------ the restatement: stage B
def label(kp0, kp1, p01, p10, vis0, vis1, valid0, valid1, pos_th, neg_th, dt=F64, keep=False):
    """gt_generation.py:97-126 (pose form) / 186-213 (homography form: vis and valid None) for one pair, keypoints (x, y).
    -> matches0, matches1, pos0 (the row's column in `positive`, -1 without one) and what the coverage test asks about; with
    `keep` the dense matrices too.  n == 0 or m == 0: the early return, -1 everywhere."""
    kp0, kp1, p01, p10 = (np.asarray(a, dt) for a in (kp0, kp1, p01, p10))
    n, m = len(kp0), len(kp1)
    if n == 0 or m == 0:
        return {"matches0": np.full(n, UNMATCHED, np.int64), "matches1": np.full(m, UNMATCHED, np.int64), "pos0": np.full(n, -1, np.int64)}
    with np.errstate(invalid="ignore", over="ignore"):
        dist0 = ((p01[:, None, :] - kp1[None, :, :]) ** 2).sum(-1)
        dist1 = ((kp0[:, None, :] - p10[None, :, :]) ** 2).sum(-1)
        dist = np.maximum(dist0, dist1)
        inf = dt(np.inf)
        if vis0 is not None:
            mask_visible = np.asarray(vis0, bool)[:, None] & np.asarray(vis1, bool)[None, :]
            dist = np.where(mask_visible, dist, inf)
        min0, min1 = dist.argmin(1), dist.argmin(0)  # the first of equals
        ismin0, ismin1 = np.zeros(dist.shape, bool), np.zeros(dist.shape, bool)
        ismin0[np.arange(n), min0] = True
        ismin1[min1, np.arange(m)] = True
        positive = ismin0 & ismin1 & (dist < dt(pos_th ** 2))
        near0, near1 = dist0.min(1), dist1.min(0)
        negative0, negative1 = near0 > dt(neg_th ** 2), near1 > dt(neg_th ** 2)
        if valid0 is not None:
            negative0, negative1 = negative0 & np.asarray(valid0, bool), negative1 & np.asarray(valid1, bool)
        m0 = np.where(positive.any(1), min0, IGNORE)
        m1 = np.where(positive.any(0), min1, IGNORE)
        m0 = np.where(negative0, UNMATCHED, m0).astype(np.int64)
        m1 = np.where(negative1, UNMATCHED, m1).astype(np.int64)
        rowmin, colmin = dist.min(1), dist.min(0)
        out = {"matches0": m0, "matches1": m1, "pos0": np.where(positive.any(1), min0, -1).astype(np.int64), "min0": min0, "min1": min1,
               "dmin0": rowmin, "dmin1": colmin, "near0": near0, "near1": near1,
               # rows / columns whose finite minimum is reached more than once, and the second index that reaches it
               "tied0": np.isfinite(rowmin) & ((dist == rowmin[:, None]).sum(1) > 1),
               "tied1": np.isfinite(colmin) & ((dist == colmin[None, :]).sum(0) > 1),
               "last0": m - 1 - (dist == rowmin[:, None])[:, ::-1].argmax(1), "last1": n - 1 - (dist == colmin[None, :])[::-1].argmax(0),
               "at_pos": int((dist == dt(pos_th ** 2)).sum()), "at_neg": int((dist0 == dt(neg_th ** 2)).sum())}
        # what dist0 alone would have matched: the arg-min of dist0 under the same mask
        only0 = dist0 if vis0 is None else np.where(mask_visible, dist0, inf)
        out["min0_dist0_only"] = only0.argmin(1)
        # the nearest dist0 neighbour of every row, visible or not
        out["nearest0_any"] = np.where(np.isnan(dist0), inf, dist0).argmin(1)
        if keep:
            out.update(dist0=dist0, dist1=dist1, dist=dist, positive=positive)
    return out


# ------------------------------------------------------------------------------------------------ the restatement: stage C
def matcher_metrics(m, gt, scores):
    """lightglue.py:17-63 for one pair in float64 -> [recall, precision, accuracy, average_precision]; ranking_ap in the reference's
    long form with a STABLE argsort of -scores (the lowest index first among equal scores: 8e's rule where the reference's unstable
    sort leaves the order open).  A pair without rows is NaN (8e; the reference has no counts)."""
    m, gt = np.asarray(m, np.int64), np.asarray(gt, np.int64)
    if len(m) == 0:
        return np.full(4, np.nan)
    tp = (m == gt).astype(F64)
    r_mask, a_mask, p_mask = (gt > -1).astype(F64), (gt >= -1).astype(F64), ((m > -1) & (gt >= -1)).astype(F64)
    recall = (tp * r_mask).sum() / (1e-8 + r_mask.sum())
    accuracy = (tp * a_mask).sum() / (1e-8 + a_mask.sum())
    precision = (tp * p_mask).sum() / (1e-8 + p_mask.sum())
    order = np.argsort(-np.asarray(scores, F64), kind="stable")
    sp, sr, st = p_mask[order], r_mask[order], tp[order]
    p_pts = np.cumsum(st * sp) / (1e-8 + np.cumsum(sp))
    r_pts = np.cumsum(st * sr) / (1e-8 + sr.sum())
    ap = np.sum((r_pts[1:] - r_pts[:-1]) * p_pts[-1])
    return np.array([recall, precision, accuracy, ap])


# ------------------------------------------------------------------------------------------------ stage B cases
class Case:
    pass


LABEL_CASES = {  # name -> (cap0, cap1, [(n, m) per pair], pos_th, neg_th)
    "cols_third_chunk": (1030, 2049, [(1030, 2049), (300, 2049)], 3, 5),
    "rows_second_chunk": (2048, 1027, [(2048, 1027), (1500, 400)], 3, 5),
    "groups_past_count": (1536, 1100, [(1030, 1100), (1536, 600), (0, 300)], 3, 5),
    "single_point_sides": (257, 1025, [(257, 1025), (1, 1025), (200, 1)], 3, 5),
    "neg_below_pos": (257, 1025, [(257, 1025), (100, 1025)], 3, 2),
}
SHIFT = np.array([8.25, -4.5])  # the background's true motion
_SITES = [(304.0 + 24 * (k % 8), 24.0 + 24 * (k // 8)) for k in range(152)]


class _Pair:
    """one pair under construction: background points in x < 285, gadgets on sites in x >= 296, 24 px apart (further than any
    threshold from each other and from the background), each gadget on rows / columns no other gadget uses"""

    def __init__(self, seed, n, m):
        self.n, self.m, self.site, self.used0, self.used1 = n, m, 0, set(), set()
        q = lambda s, k, mod: ints(seed + s, (k,), mod)  # noqa: E731
        self.kp0 = np.stack([16 + q(1, n, 1024) / 4.0, 16 + q(2, n, 1920) / 4.0], 1)
        self.kp1 = np.stack([24 + q(3, m, 1024) / 4.0, 16 + q(4, m, 1900) / 4.0], 1)
        k = min(n, m) // 2  # correspondences at permuted positions: side 1 = the moved point + up to 2.5 px in quarter steps
        src = np.argsort(q(5, n, 1 << 30), kind="stable")[:k]
        dst = np.argsort(q(6, m, 1 << 30), kind="stable")[:k]
        self.kp1[dst] = self.kp0[src] + SHIFT + (ints(seed + 7, (k, 2), 21) - 10) / 4.0
        self.p01 = self.kp0 + SHIFT + (ints(seed + 8, (n, 2), 5) - 2) / 4.0
        self.p10 = self.kp1 - SHIFT + (ints(seed + 9, (m, 2), 5) - 2) / 4.0
        far = q(10, m, 8) == 0  # an eighth of the columns: proj_1to0 6 px off, so dist1 >> dist0 and max picks the other term
        self.p10[far] += np.array([6.0, -6.0])
        self.valid0, self.valid1 = q(11, n, 16) != 0, q(12, m, 16) != 0
        self.vis0, self.vis1 = self.valid0 & (q(13, n, 8) != 0), self.valid1 & (q(14, m, 8) != 0)
        nan0, nan1 = ~self.valid0 & (q(15, n, 2) == 0), ~self.valid1 & (q(16, m, 2) == 0)  # NaN projections: invisible, invalid points only
        self.p01[nan0], self.p10[nan1] = np.nan, np.nan
        self.info = {}

    def gadget(self, tag, rows, cols):
        """rows: [(i, a, e, visible, valid)]: kp0[i] = site + a, proj_0to1[i] = site + a + e; cols: [(j, b, f, visible, valid)]:
        kp1[j] = site + b, proj_1to0[j] = site + b + f.  Then dist0[i,j] = |a + e - b|^2 and dist1[i,j] = |a - b - f|^2.
        Skipped (False) when an index is past the pair's count or taken."""
        ri, cj = [r[0] for r in rows], [c[0] for c in cols]
        if (min(ri + cj) < 0 or max(ri, default=-1) >= self.n or max(cj, default=-1) >= self.m or self.used0 & set(ri) or self.used1 & set(cj)
                or len(set(ri)) < len(ri) or len(set(cj)) < len(cj)):
            return False
        c = np.array(_SITES[self.site])
        self.site += 1
        for i, a, e, vis, val in rows:
            self.kp0[i], self.p01[i], self.vis0[i], self.valid0[i] = c + a, c + np.add(a, e), vis, val
        for j, b, f, vis, val in cols:
            self.kp1[j], self.p10[j], self.vis1[j], self.valid1[j] = c + b, c + np.add(b, f), vis, val
        self.used0 |= set(ri)
        self.used1 |= set(cj)
        self.info.setdefault(tag, []).append((ri, cj))
        return True


Z = (0.0, 0.0)


def _plant(p, b):
    """the planted edges of one pair (issue part 2, stage B); every one is asserted from the restatement by the CPU test"""
    n, m, g = p.n, p.m, p.gadget
    on = (True, True)
    if n < 8 or m < 8:
        return
    # row 0 and column 0 invisible, 1 px apart: the all-inf arg-min is 0 on both sides and the mutual check holds
    g("origin_invisible", [(0, Z, Z, False, True)], [(0, (1.0, 0.0), Z, False, True)])
    # mutual positives with partners in the second / third chunk on both sides
    for i, j in ((n - 1, m - 1), (1026, 1500), (1500, 1026), (1028, 1029), (12, 13)) if b == 0 else ((n - 1, m - 2), (2, m - 3)):
        g("mutual", [(i, Z, Z, *on)], [(j, (1.0, 0.5), Z, *on)])
    # bit-identical columns in different chunks, across the chunk boundary and across the group of four: the lowest index wins
    for cols in ((3, 2040), (1022, 1023, 1024, 1025), (5, m - 1), (6, 1000, m - 4)):
        g("col_tie", [(20 + len(p.info.get("col_tie", [])), Z, Z, *on)], [(j, (1.0, 0.0), Z, *on) for j in cols])
    for rows in ((7, 2041), (1021, 1023, 1024, 1025), (8, 1027), (9, 1001, n - 7)):
        g("row_tie", [(i, Z, Z, *on) for i in rows], [(m - 6 - len(p.info.get("row_tie", [])), (0.0, 1.0), Z, *on)])
    # distances equal to a threshold, and their neighbours on the lattice
    top0, top1 = n - 12, m - 12
    for k, (tag, off, valid) in enumerate((("pos_eq", (3.0, 0.0), True), ("pos_in", (2.75, 1.0), True), ("neg_eq", (3.0, 4.0), True),
                                           ("neg_out_valid", (3.0, 4.25), True), ("neg_out_invalid", (3.0, 4.25), False),
                                           ("neg_eq_2", (2.0, 0.0), True), ("neg_out_2", (2.0, 0.25), True))):
        g(tag, [(top0 - k, Z, Z, valid, valid)], [(top1 - k, off, Z, valid, valid)])
    # proj_0to1 close, proj_1to0 far: by dist0 alone the row would take the first column, max(dist0, dist1) gives it the second
    g("asymmetric", [(top0 - 8, Z, Z, *on)], [(top1 - 8, (1.0, 0.0), (5.0, 0.0), *on), (top1 - 9, (0.0, 2.0), Z, *on)])
    # the nearest dist0 neighbour is invisible: it counts for `negative` and not for the arg-min
    g("invisible_nearest", [(top0 - 9, Z, Z, *on)], [(top1 - 10, (0.5, 0.0), Z, False, True), (top1 - 11, (2.0, 0.0), Z, *on)])
    g("invisible_nearest_far", [(top0 - 10, Z, Z, *on)], [(top1 - 12, (1.0, 0.0), Z, False, True), (top1 - 13, (6.0, 0.0), Z, *on)])
    # an invisible, invalid point with NaN projections beyond index 1024 (the background has them at random indices)
    g("nan_projection", [(top0 - 11, Z, (np.nan, np.nan), False, False)], [(top1 - 14, (30.0, 0.0), (np.nan, np.nan), False, False)])


_LABEL = {}


def label_case(name):
    """Unpadded per-pair arrays (float32, (x, y)) of a stage B case.  c.pairs[b]: kp0, kp1, p01, p10, vis0, vis1, valid0, valid1,
    info; the homography form reads p01_h / p10_h (NaN projections replaced by the background's motion) and no masks."""
    if name in _LABEL:
        return _LABEL[name]
    cap0, cap1, counts, pos_th, neg_th = LABEL_CASES[name]
    c = Case()
    c.name, c.cap0, c.cap1, c.counts, c.pos_th, c.neg_th, c.B, c.pairs = name, cap0, cap1, counts, pos_th, neg_th, len(counts), []
    for b, (n, m) in enumerate(counts):
        p = _Pair(1000 * (1 + list(LABEL_CASES).index(name)) + 100 * b, n, m)
        _plant(p, b)
        for k in ("kp0", "kp1", "p01", "p10"):
            setattr(p, k, getattr(p, k).astype(np.float32))
        p.p01_h = np.where(np.isnan(p.p01), p.kp0 + SHIFT.astype(np.float32), p.p01)
        p.p10_h = np.where(np.isnan(p.p10), p.kp1 - SHIFT.astype(np.float32), p.p10)
        c.pairs.append(p)
    _LABEL[name] = c
    return c


FORMS = ("pose", "homography")


def label_inputs(p, form):
    if form == "pose":
        return p.kp0, p.kp1, p.p01, p.p10, p.vis0, p.vis1, p.valid0, p.valid1
    return p.kp0, p.kp1, p.p01_h, p.p10_h, None, None, None, None


_EXPECT = {}


def label_expected(name, form, dt=F64):
    """the restatement's answer for every pair of a case (computed once per (case, form, dtype))"""
    key = (name, form, np.dtype(dt).name)
    if key not in _EXPECT:
        c = label_case(name)
        _EXPECT[key] = [label(*label_inputs(p, form), c.pos_th, c.neg_th, dt) for p in c.pairs]
    return _EXPECT[key]


def pad_rows(rows, cap, fill, ordering="xy", cols=2):
    """[B,cap,cols] float32 from per-pair [n,2] (x, y) arrays: (y, x) when ordering is "yx", further columns and rows past the
    count hold `fill`"""
    out = np.full((len(rows), cap, cols), fill, np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r), :2] = r[:, ::-1] if ordering == "yx" else r
    return out


def pad_flags(rows, cap, fill):
    out = np.full((len(rows), cap), fill, bool)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def pad_values(rows, cap, fill, dtype=np.float32):
    out = np.full((len(rows), cap), fill, dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


# ------------------------------------------------------------------------------------------------ sampler cases
def _sampler_points(H, W):
    """keypoints (x, y) for an H x W map, wholly on the half-integer grid or wholly on odd quarters.  No off-grid point has
    ix = k + 0.5 exactly (an integer coordinate): the nearest-pixel fallback would then sit on a rounding tie, where the reference's
    own outcome hangs on how its x / W * 2 - 1 round trip rounds, so half-to-even is exercised only through the on-grid points'
    exact integers."""
    pts = []
    for y in range(H):  # every pixel of the left and right border, the corners included
        pts += [(0.5, y + 0.5), (W - 0.5, y + 0.5)]
    for x in range(1, W - 1):
        pts += [(x + 0.5, 0.5), (x + 0.5, H - 0.5)]
    # quarter offsets: two taps outside on each border, three in each corner
    for y in (3.25, 3.75, 6.25):
        pts += [(0.25, y), (W - 0.25, y)]
    for x in (5.25, 5.75, 10.75):
        pts += [(x, 0.25), (x, H - 0.25)]
    pts += [(0.25, 0.25), (W - 0.25, 0.25), (0.25, H - 0.25), (W - 0.25, H - 0.25)]
    # holes under a weighted tap (see _sampler_holes): nearest good, nearest a hole, nearest outside the map
    pts += [(7.25, 5.25), (10.25, 7.25), (-0.25, 6.25), (W + 0.25, 2.75), (4.75, -0.25), (8.25, H + 0.25)]
    # every tap outside: a few pixels out on each side and in a corner, half-integer and quarter offsets
    pts += [(-3.5, 4.5), (W + 2.5, 4.5), (5.5, -3.5), (5.5, H + 3.5), (-1.25, 3.25), (W + 1.75, 3.75), (-2.5, -2.5), (W + 0.5, H + 0.5),
            (-1.5, 4.5), (W + 1.5, 4.5), (-0.75, 2.25), (6.75, H + 0.75)]
    big, inf, nan = 1e10, np.inf, np.nan
    pts += [(big, 4.5), (-big, 4.5), (inf, 4.5), (nan, 4.5), (5.5, big), (5.5, -big), (5.5, inf), (5.5, nan), (5.25, -inf), (-inf, 3.25),
            (nan, nan), (inf, -inf), (big, big)]
    seed = 31 * H + W
    k = 24  # interior points, half of them on the grid
    on = np.stack([ints(seed, (k,), W) + 0.5, ints(seed + 1, (k,), H) + 0.5], 1)
    off = np.stack([ints(seed + 2, (k,), W - 1) + 0.75 + 0.5 * ints(seed + 3, (k,), 2), ints(seed + 4, (k,), H - 1) + 0.75 + 0.5 * ints(seed + 5, (k,), 2)], 1)
    return np.concatenate([np.array(pts), on, off]).astype(np.float32)


def _sampler_map(seed, H, W):
    """depths k/64 in [4, 6], 8 % holes (0, negative, NaN), then the planted holes and the good pixels beside them"""
    d = (256 + ints(seed, (H, W), 129)) / 64.0
    r = ints(seed + 1, (H, W), 36)
    d[r == 0], d[r == 1], d[r == 2] = 0.0, -1.5, np.nan
    good = lambda y, x: d.__setitem__((y, x), (300 + 7 * y + x) / 64.0)  # noqa: E731
    d[0, 3], d[5, 0], d[H - 1, W - 1] = 0.0, -1.0, np.nan  # under the one tap of a border point
    good(0, 4), good(H - 1, 0), good(0, W - 1)
    d[4, 6] = np.nan  # (7.25, 5.25): weight 1/16 on the hole, nearest pixel (5, 7) good
    good(5, 7), good(4, 7), good(5, 6)
    d[6, 10], d[7, 10] = -2.0, np.nan  # (10.25, 7.25): nearest pixel (7, 10) a hole
    d[6, 0] = 0.0  # (-0.25, 6.25): a weighted hole, nearest pixel x = -1 outside -> 0
    d[2, W - 1] = np.nan  # (W + 0.25, 2.75): nearest x = W outside
    good(0, 5)  # (4.75, -0.25) reads pixels (0, 4) and (0, 5), both good: two taps of four, the nearest pixel is not consulted
    d[H - 1, 8] = 0.0  # (8.25, H + 0.25): nearest y = H outside
    return d


_SAMPLER = None


def sampler_case():
    """two pairs on a 12 x 20 and a 9 x 16 map; pair 1 has other depths and ragged counts"""
    global _SAMPLER
    if _SAMPLER is None:
        c = Case()
        c.size0, c.size1, c.B = (12, 20), (9, 16), 2
        k0, k1 = _sampler_points(*c.size0), _sampler_points(*c.size1)
        c.cap0, c.cap1 = len(k0), len(k1)
        c.n, c.m = [c.cap0, c.cap0 - 7], [c.cap1, c.cap1 - 30]
        c.kp0, c.kp1 = [k0[:n] for n in c.n], [k1[:m] for m in c.m]
        c.depth0 = np.stack([_sampler_map(50 + b, *c.size0) for b in range(2)]).astype(np.float32)
        c.depth1 = np.stack([_sampler_map(60 + b, *c.size1) for b in range(2)]).astype(np.float32)
        K = lambda H, W: np.array([[16, 0, W / 2], [0, 16, H / 2], [0, 0, 1]], np.float32)  # noqa: E731
        c.K0, c.K1 = np.stack([K(*c.size0)] * 2), np.stack([K(*c.size1)] * 2)
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = [0.25, -0.5, 0.125]
        c.T01 = np.stack([T, T])
        c.T10 = np.stack([invert_pose(T).astype(np.float32)] * 2)
        _SAMPLER = c
    return _SAMPLER


# ------------------------------------------------------------------------------------------------ projection cases
RZ = {0: [[1, 0, 0], [0, 1, 0], [0, 0, 1]], 90: [[0, -1, 0], [1, 0, 0], [0, 0, 1]], 180: [[-1, 0, 0], [0, -1, 0], [0, 0, 1]]}


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _kmat(f, cx, cy):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])


def _preimage(uv, z, K_self, K_other, T):
    """the keypoint of this view whose projection is `uv` at q.z = z (rotation about the optical axis): exact on dyadic inputs"""
    q = np.array([(uv[0] - K_other[0, 2]) / K_other[0, 0] * z, (uv[1] - K_other[1, 2]) / K_other[1, 1] * z, z])
    p = T[:3, :3].T @ (q - T[:3, 3])
    return np.array([p[0] / p[2] * K_self[0, 0] + K_self[0, 2], p[1] / p[2] * K_self[1, 1] + K_self[1, 2]]), p[2]


def _lattice_points(seed, k, H, W):
    """k interior keypoints, wholly on the half-integer grid (even index) or wholly on odd quarters"""
    on = np.stack([ints(seed, (k,), W - 2) + 1.5, ints(seed + 1, (k,), H - 2) + 1.5], 1)
    off = np.stack([ints(seed + 2, (k,), W - 3) + 1.75 + 0.5 * ints(seed + 3, (k,), 2), ints(seed + 4, (k,), H - 3) + 1.75 + 0.5 * ints(seed + 5, (k,), 2)], 1)
    return np.where((np.arange(k) % 2 == 0)[:, None], on, off)


_PROJ = None
PLANE = 2.0


def projection_case():
    """three pairs, f = 32 on both sides, depth maps 32 x 48 and 36 x 52 holding the plane d = 2 (so q.z = 2) plus holes:
      pair 0  rotation by 180 degrees about the optical axis, t = (-1/32, -1/32, 0); camera 0 is 48 x 32, camera 1 32 x 24
      pair 1  rotation by 90 degrees, the same translation; camera 0 is 32 x 24, camera 1 48 x 32
      pair 2  identity, t = 0, principal points (16.5, 12.5) and (24.5, 16.5): the first two keypoints of each side sit on the
              principal point, where the maps hold float32(1e-4) (side 0: q.z == eps, not in front, u = cx') and the next float
              above it (side 1: in front and visible)
    In pair 1 the cameras change places (camera 0 is 32 x 24 there), so that each side reaches every border of the other camera from
    inside its own map in one pair or the other.  Planted in pairs 0 and 1: projections with u == 0, v == 0, u == 2cx'-1, v == 2cy'-1
    exactly (inside) and a quarter pixel beyond each (outside), wherever the preimage lies in the view's map.  The precomputed depths
    are 2 on the planted rows and 0.5 .. 4 elsewhere."""
    global _PROJ
    if _PROJ is not None:
        return _PROJ
    c = Case()
    c.B, c.size0, c.size1 = 3, (32, 48), (36, 52)
    t = [-1 / 32, -1 / 32, 0.0]
    Ts = [_pose(RZ[180], t), _pose(RZ[90], t), _pose(RZ[0], [0, 0, 0])]
    K0s = [_kmat(32, 24, 16), _kmat(32, 16, 12), _kmat(32, 16.5, 12.5)]
    K1s = [_kmat(32, 16, 12), _kmat(32, 24, 16), _kmat(32, 24.5, 16.5)]
    eps, nxt = float(EPS_Z), float(np.nextafter(EPS_Z, np.float32(1)))
    c.depth0 = np.full((3,) + c.size0, PLANE)
    c.depth1 = np.full((3,) + c.size1, PLANE)
    for b in range(3):
        for d, s in ((c.depth0[b], 70 + b), (c.depth1[b], 80 + b)):
            r = ints(s, d.shape, 24)
            d[r == 0], d[r == 1], d[r == 2] = 0.0, -1.0, np.nan
    c.kp0, c.kp1, c.pre, c.planted = [], [], [], []
    for b in range(3):
        T, Ti, K0, K1 = Ts[b], invert_pose(Ts[b]), K0s[b], K1s[b]
        sides = []
        for side, (Ks, Ko, Tso, size) in enumerate(((K0, K1, T, c.size0), (K1, K0, Ti, c.size1))):
            pts, planted = [], []
            dmap = c.depth0[b] if side == 0 else c.depth1[b]
            if b == 2:
                pts += [(Ks[0, 2], Ks[1, 2])] * 2
                dmap[int(Ks[1, 2] - 0.5), int(Ks[0, 2] - 0.5)] = eps if side == 0 else nxt
            else:
                wmax, hmax = 2 * Ko[0, 2] - 1, 2 * Ko[1, 2] - 1
                targets = {"u0": (0, 10), "umax": (wmax, 10), "v0": (10, 0), "vmax": (10, hmax), "c00": (0, 0), "cmm": (wmax, hmax),
                           "c0m": (0, hmax), "cm0": (wmax, 0), "u-": (-0.25, 10.25), "u+": (wmax + 0.25, 10.25), "v-": (10.25, -0.25),
                           "v+": (10.25, hmax + 0.25)}
                for tag, uv in targets.items():
                    xy, d = _preimage(uv, PLANE, Ks, Ko, Tso)
                    assert d == PLANE
                    if not (0.5 <= xy[0] <= size[1] - 0.5 and 0.5 <= xy[1] <= size[0] - 0.5):
                        continue  # a preimage outside this view's map would sample depth 0: q = t, q.z = eps and an inexact quotient
                    planted.append((len(pts), tag, uv))
                    pts.append(tuple(xy))
                    x0, y0 = int(np.floor(xy[0] - 0.5)), int(np.floor(xy[1] - 0.5))
                    dmap[y0:min(y0 + 2, size[0]), x0:min(x0 + 2, size[1])] = PLANE  # no hole under a planted point
            pts = np.concatenate([np.array(pts).reshape(-1, 2), _lattice_points(90 + 10 * b + side, 50, *size)])
            depths = 0.5 * 2.0 ** ints(95 + 10 * b + side, (len(pts),), 4)  # 0.5, 1, 2, 4: q.z = d is a power of two
            depths[:len(planted)] = PLANE
            if b == 2:
                depths[:2] = [eps, nxt]
            valid = ints(97 + 10 * b + side, (len(pts),), 10) != 0
            valid[:max(len(planted), 2)] = True
            sides.append((pts, depths, valid, planted))
        c.kp0.append(sides[0][0].astype(np.float32))
        c.kp1.append(sides[1][0].astype(np.float32))
        c.pre.append((sides[0][1].astype(np.float32), sides[0][2], sides[1][1].astype(np.float32), sides[1][2]))
        c.planted.append((sides[0][3], sides[1][3]))
    c.n, c.m = [len(k) for k in c.kp0], [len(k) for k in c.kp1]
    c.cap0, c.cap1 = max(c.n) + 3, max(c.m) + 5
    c.depth0, c.depth1 = c.depth0.astype(np.float32), c.depth1.astype(np.float32)
    c.K0, c.K1 = np.stack(K0s).astype(np.float32), np.stack(K1s).astype(np.float32)
    c.T01 = np.stack(Ts).astype(np.float32)
    c.T10 = np.stack([invert_pose(T) for T in Ts]).astype(np.float32)
    _PROJ = c
    return c


# ------------------------------------------------------------------------------------------------ one whole scene
_SCENE = None


def scene_case():
    """pose form end to end beyond 1024 keypoints on both sides: caps 1030 x 2049, counts (1030, 2049) and (1027, 1500); view 0 is
    448 x 336 (f = 256), view 1 its rotation by 90 degrees about the optical axis (336 x 448) with t = (3/128, -2/128, 0), so that
    u = 339 - y and v = x - 2 on the plane d = 2: half-integer keypoints land on half-integers, odd quarters on odd quarters.  Depth
    is that plane with 3 % holes.  Half of the smaller side corresponds, at permuted indices, up to 2 px off in whole pixels (a
    keypoint stays on its grid)."""
    global _SCENE
    if _SCENE is not None:
        return _SCENE
    c = Case()
    c.B, c.cap0, c.cap1, c.n, c.m = 2, 1030, 2049, [1030, 1027], [2049, 1500]
    c.size0, c.size1, c.pos_th, c.neg_th = (336, 448), (448, 336), 3, 5
    T = _pose(RZ[90], [3 / 128, -2 / 128, 0.0])
    K0, K1 = _kmat(256, 224, 168), _kmat(256, 168, 224)
    c.kp0, c.kp1, d0s, d1s = [], [], [], []
    for b in range(2):
        sd = 5000 + 100 * b
        kp0, kp1 = _lattice_points(sd, c.n[b], *c.size0), _lattice_points(sd + 10, c.m[b], *c.size1)
        k = min(c.n[b], c.m[b]) // 2
        src = np.argsort(ints(sd + 20, (c.n[b],), 1 << 30), kind="stable")[:k]
        dst = np.argsort(ints(sd + 21, (c.m[b],), 1 << 30), kind="stable")[:k]
        moved = np.stack([339 - kp0[src, 1], kp0[src, 0] - 2], 1)
        moved = moved + (ints(sd + 22, (k, 2), 3) + ints(sd + 23, (k, 2), 3) - 2.0)
        ok = (moved[:, 0] >= 1) & (moved[:, 0] <= c.size1[1] - 1) & (moved[:, 1] >= 1) & (moved[:, 1] <= c.size1[0] - 1)
        kp1[dst[ok]] = moved[ok]  # every keypoint stays inside its map: depth 0 would give q = t, q.z = eps and an inexact quotient
        for d, s, size in ((d0s, sd + 30, c.size0), (d1s, sd + 31, c.size1)):
            dm = np.full(size, PLANE)
            r = ints(s, size, 100)
            dm[r == 0], dm[r == 1], dm[r == 2] = 0.0, -1.0, np.nan
            d.append(dm)
        c.kp0.append(kp0.astype(np.float32))
        c.kp1.append(kp1.astype(np.float32))
    c.depth0, c.depth1 = np.stack(d0s).astype(np.float32), np.stack(d1s).astype(np.float32)
    c.K0, c.K1 = np.stack([K0] * 2).astype(np.float32), np.stack([K1] * 2).astype(np.float32)
    c.T01, c.T10 = np.stack([T] * 2).astype(np.float32), np.stack([invert_pose(T)] * 2).astype(np.float32)
    _SCENE = c
    return c


_SCENE_EXPECT = {}


def scene_expected(dt=F64):
    """stage A + B of every pair of scene_case()"""
    key = np.dtype(dt).name
    if key not in _SCENE_EXPECT:
        c, out = scene_case(), []
        for b in range(c.B):
            e = project_pair(c.kp0[b], c.kp1[b], c.K0[b], c.K1[b], c.T01[b], c.T10[b], c.depth0[b], c.depth1[b], dt=dt)
            e.update(label(c.kp0[b], c.kp1[b], e["proj_0to1"], e["proj_1to0"], e["visible0"], e["visible1"], e["valid0"], e["valid1"],
                           c.pos_th, c.neg_th, dt))
            out.append(e)
        _SCENE_EXPECT[key] = out
    return _SCENE_EXPECT[key]


STAGE_A_KEYS = ("depth_keypoints0", "depth_keypoints1", "valid0", "valid1", "proj_0to1", "proj_1to0", "visible0", "visible1")
SIDE0_KEYS = ("depth_keypoints0", "valid0", "proj_0to1", "visible0", "matches0", "matching_scores0", "pos0")
PADDING = {"matches0": -2, "matches1": -2, "pos0": -1}  # rows at or beyond a pair's count; zero in every other output


def padded_expected(pairs, cap0, cap1, keys):
    """[B,cap,...] float64 / int64 / bool arrays of per-pair results, the kernels' padding past each count"""
    out = {}
    for k in keys:
        cap = cap0 if k in SIDE0_KEYS else cap1
        first = np.asarray(pairs[0][k])
        a = np.full((len(pairs), cap) + first.shape[1:], PADDING.get(k, 0), first.dtype)
        for b, p in enumerate(pairs):
            a[b, :len(p[k])] = p[k]
        out[k] = a
    return out


def with_scores(e):
    e = dict(e)
    e["matching_scores0"], e["matching_scores1"] = (e["matches0"] > -1).astype(F64), (e["matches1"] > -1).astype(F64)
    return e


# ------------------------------------------------------------------------------------------------ stage C cases
PR_CAPS = (1, 63, 64, 65, 130, 1030)
_PR = {}


def pr_case(cap):
    """-> m, gt [B,cap] int64, sc [B,cap] float32, n [B] int32, names [B], ties {pair: (low, high)}.  Background: a third of the
    predictions wrong or missing, scores k/128 below 0.5.  Rows past n[b] hold a true positive with the highest score of all."""
    if cap in _PR:
        return _PR[cap]
    names = ["all_equal", "same_lane_low_right", "same_lane_high_right", "higher_lane_low_right", "higher_lane_high_right", "all_minus_inf",
             "plus_inf_top", "plus_inf_tie", "past_count", "no_recall_rows", "no_precision_rows", "no_accuracy_rows", "no_rows"]
    B, seed = len(names), 7000 + cap
    gt = ints(seed, (B, cap), cap + 3) - 2
    gt[gt >= cap // 2 + 1] = -1
    m = np.where(ints(seed + 1, (B, cap), 3) == 0, ints(seed + 2, (B, cap), cap // 2 + 2) - 1, gt)
    sc = (ints(seed + 3, (B, cap), 64) / 128.0).astype(np.float32)
    n = np.array([max(min(cap, 1), cap - (b % 4)) for b in range(B)], np.int32)
    n[names.index("no_rows")] = 0
    ties = {}

    def right(b, i):
        m[b, i] = gt[b, i] = 4

    def wrong(b, i):
        m[b, i], gt[b, i] = 3, 5

    def tie(b, low, high, low_right, value=0.75):
        if high >= n[b] or low >= high or low < 0:
            return
        sc[b, low] = sc[b, high] = value
        (right if low_right else wrong)(b, low)
        (wrong if low_right else right)(b, high)
        ties[b] = (low, high)

    for b, name in enumerate(names):
        nb = int(n[b])
        if name == "all_equal":
            sc[b] = 0.25
            right(b, 0)
            if nb > 1:
                wrong(b, nb - 1)
                ties[b] = (0, nb - 1)
        elif name.startswith("same_lane"):  # rows 5 and 69 are lane 5's first and second row; below 70 rows, lane 0's (0 and 64)
            lo, hi = (5, 69) if nb > 69 else (0, 64)
            tie(b, lo, hi, name.endswith("low_right"))
        elif name.startswith("higher_lane"):  # row 7 in lane 7, row 70 in lane 6; below 71 rows (1, 64), then any two lanes
            lo, hi = (7, 70) if nb > 70 else (1, 64) if nb > 64 else (2, min(40, nb - 1))
            tie(b, lo, hi, name.endswith("low_right"))
        elif name == "all_minus_inf":
            sc[b] = -np.inf
            right(b, 0)
            if nb > 1:
                wrong(b, 1)
                ties[b] = (0, 1)
        elif name == "plus_inf_top" and nb:
            sc[b, nb - 1] = np.inf
            right(b, nb - 1)
        elif name == "plus_inf_tie":
            tie(b, min(3, nb - 1), nb - 1, True, np.inf)
        elif name == "past_count":
            n[b] = nb = max(min(cap, 1), cap - 3)
            if nb < cap:
                sc[b, nb:] = 1e9
                for i in range(nb, cap):
                    right(b, i)
            if nb:
                sc[b, nb // 2] = 0.75
                wrong(b, nb // 2)
        elif name == "no_recall_rows":
            gt[b] = -1 - (ints(seed + 5, (cap,), 2))
        elif name == "no_precision_rows":
            m[b] = np.where(gt[b] == -2, m[b], -1)
        elif name == "no_accuracy_rows":
            gt[b] = -2
    _PR[cap] = (m.astype(np.int64), gt.astype(np.int64), sc, n, names, ties)
    return _PR[cap]


def pr_expected(cap):
    m, gt, sc, n, _, _ = pr_case(cap)
    return np.stack([matcher_metrics(m[b, :n[b]], gt[b, :n[b]], sc[b, :n[b]]) for b in range(len(n))])
