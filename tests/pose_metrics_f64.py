"""The pair metrics under depth + motion (einx_pair_metrics_pose) restated in numpy, and inputs on which fp32 computes
every decision of them exactly.

Not collected by pytest (no test_ prefix).  tests/test_pose_metrics_cpu.py checks this restatement against itself in float32 and
against metrics_f64.Restated under the induced homography; tests/test_pose_metrics_gpu.py compares the kernels of csrc/metrics.hip
with it.

Written from the reference's text with dense [N1,N2] matrices and numpy's arg-min; it shares nothing with the kernels.  The depth
sampler, the projection and the pose inverse are gt_matches_f64's (depth.py:9-69 restated), the symmetric epipolar distance is
gt_matches_ref.epipolar_all, the descriptor records are metrics_f64._desc_records.  Every function takes the dtype it computes in;
the epipolar distance is computed in float64 only, as the kernel does.

Why exact inputs (as gt_matches_f64.projection_case / scene_case): depth maps hold planes d in {1, 2} (and holes), the motion is a
rotation by 0 / 90 / 180 degrees about the optical axis plus a dyadic translation, focal lengths are 32; keypoints lie wholly on
the half-integer grid or wholly on odd quarters.  Every sample, projection, bound test and squared distance is then representable
in fp32, float32 and float64 agree bit for bit (asserted by the CPU test), and the GPU test compares with array_equal."""
import zlib

import numpy as np

from gt_matches_f64 import RZ, invert_pose, project_side, sample_depth
from gt_matches_ref import epipolar_all
from metrics_f64 import _desc_records
from mnn_f64 import exact_unit

F64 = np.float64
SIZE0, SIZE1 = (48, 64), (40, 56)  # (H, W) of image 0 / image 1
FOCAL = 32.0
PLANE = 2.0
EPI_MARGIN = 1e-6


# ------------------------------------------------------------------------------------------------ the restatement
def project_view(xy, depth_s, depth_o, K_s, K_o, T, Tinv, occlusion_th, dt=F64):
    """contract 1 and 2 for the points xy [n,2] (x, y) of one view: -> uv [n,2] in the other view, ok [n] = valid & front (and,
    with occlusion_th > 0, the circle consistency of depth.py:62-67 with the threshold in pixels: the other map sampled at uv,
    back-projected with the inverse motion, valid, in front and |xy - back|^2 < occlusion_th^2), valid [n]"""
    xy = np.asarray(xy, dt).reshape(-1, 2)
    d, valid, _ = sample_depth(xy, depth_s, dt)
    uv, _, side = project_side(xy, d, valid, K_s, K_o, T, dt)
    ok = valid & side["front"]
    if occlusion_th is not None and occlusion_th > 0:
        d2, valid2, _ = sample_depth(uv, depth_o, dt)
        back, _, side2 = project_side(uv, d2, valid2, K_o, K_s, Tinv, dt)
        with np.errstate(invalid="ignore"):
            consistent = ((xy - back) ** 2).sum(1) < dt(occlusion_th) * dt(occlusion_th)
        ok = ok & valid2 & side2["front"] & consistent
    return uv, ok, valid


def inside(uv, size):
    """util.py:43-70 (keep_true_points): 0 <= u < W, 0 <= v < H of the IMAGE; NaN is outside"""
    with np.errstate(invalid="ignore"):
        return (uv[:, 0] >= 0) & (uv[:, 0] < size[1]) & (uv[:, 1] >= 0) & (uv[:, 1] < size[0])


class RestatedPose:
    """One pair.  k0 [n,>=2], k1 [m,>=2] keypoint rows ((y, x, ..) if kp_yx), d0 [n,D], d1 [m,D], mk0 / mk1 [M,2|3], size0 / size1
    the image sizes (H, W), K0 / K1 [3,3], T01 [4,4], T10 [4,4] or None (Pose.inv), depth0 / depth1 [H,W] or both None.

    warped0 [n,2], ok0 / ok1, keep0 / keep1, N1, N2     contract 1 and 2
    near_d / near_j / near_sq / desc_sq / desc_d / angle   per side, as metrics_f64.Restated (contract 3)
    judged [M], mma_sq [M]                               contract 4: squared reprojection error of every match
    epi [M]                                              contract 5, float64"""

    def __init__(self, k0, k1, d0, d1, mk0, mk1, size0, size1, K0, K1, T01, T10=None, depth0=None, depth1=None, occlusion_th=None,
                 kp_yx=True, dt=F64):
        f = lambda a: np.asarray(a, F64)  # noqa: E731
        xy = [1, 0] if kp_yx else [0, 1]
        k0, k1, mk0, mk1 = f(k0), f(k1), f(mk0), f(mk1)
        self.n, self.m, self.M = k0.shape[0], k1.shape[0], mk0.shape[0]
        self.has_depth = depth0 is not None
        assert (depth0 is None) == (depth1 is None)
        p0, p1 = k0[:, xy].astype(dt), k1[:, xy].astype(dt)
        q0, q1 = mk0[:, xy].astype(dt), mk1[:, xy].astype(dt)
        Tinv = invert_pose(T01, dt) if T10 is None else np.asarray(T10, dt)
        counts = (self.n, self.m)
        self.near_d = [np.full((c,), np.inf) for c in counts]
        self.near_j = [np.full((c,), -1, np.int64) for c in counts]
        self.near_sq, self.desc_sq, self.desc_d, self.angle = ([np.full((c,), np.nan) for c in counts] for _ in range(4))
        self.N1 = self.N2 = 0
        self.ties = [0, 0]  # rows / columns of the distance matrix whose minimum is reached more than once
        if self.has_depth:
            self.warped0, self.ok0, self.valid0 = project_view(p0, depth0, depth1, K0, K1, T01, Tinv, occlusion_th, dt)
            w1, self.ok1, self.valid1 = project_view(p1, depth1, depth0, K1, K0, Tinv, T01, occlusion_th, dt)
            self.keep0, self.keep1 = self.ok0 & inside(self.warped0, size1), self.ok1 & inside(w1, size0)
            self.N1, self.N2 = int(self.keep0.sum()), int(self.keep1.sum())
            if self.N1 and self.N2:
                a, b = self.warped0[self.keep0], p1[self.keep1]
                sq = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)  # [N1,N2]
                norm = np.sqrt(sq)
                d0, d1 = f(d0), f(d1)
                orig0, orig1 = np.nonzero(self.keep0)[0], np.nonzero(self.keep1)[0]
                i1, i0 = norm.argmin(1), norm.argmin(0)  # numpy: the first occurrence of the minimum
                rows, cols = np.arange(self.N1), np.arange(self.N2)
                self.near_d[0][orig0], self.near_sq[0][orig0], self.near_j[0][orig0] = norm[rows, i1], sq[rows, i1], orig1[i1]
                self.near_d[1][orig1], self.near_sq[1][orig1], self.near_j[1][orig1] = norm[i0, cols], sq[i0, cols], orig0[i0]
                self.desc_sq[0][orig0], self.desc_d[0][orig0], self.angle[0][orig0] = _desc_records(d0[orig0], d1[orig1[i1]])
                self.desc_sq[1][orig1], self.desc_d[1][orig1], self.angle[1][orig1] = _desc_records(d0[orig0[i0]], d1[orig1])
                self.ties = [int(((sq == sq.min(1, keepdims=True)).sum(1) > 1).sum()), int(((sq == sq.min(0, keepdims=True)).sum(0) > 1).sum())]
            mw, self.judged, _ = project_view(q0, depth0, depth1, K0, K1, T01, Tinv, occlusion_th, dt)
            with np.errstate(invalid="ignore"):
                self.mma_sq = ((mw - q1) ** 2).sum(1)
            self.match_proj = mw
        else:
            self.judged, self.mma_sq = np.zeros(self.M, bool), np.full(self.M, np.nan)
        # the epipolar distance of match r: the diagonal of sym_epipolar_distance_all, float64
        self.epi = np.diagonal(epipolar_all(f(mk0)[:, xy], f(mk1)[:, xy], K0, K1, T01, F64)).copy() if self.M else np.zeros(0)

    def selected(self, t):
        return self.near_d[0] <= t, self.near_d[1] <= t

    def mma_good(self, t):
        """judged matches whose error sqrt(dx^2 + dy^2), rounded to fp32 as the metric computes it, is <= t"""
        with np.errstate(invalid="ignore"):
            return self.judged & (np.sqrt(self.mma_sq.astype(F64)).astype(np.float32) <= np.float32(t))

    def row(self, mma_thr=(1, 3), vdd_thr=(1, 3), epi_thr=()):
        """[MR, MMA@t.., judged_ratio, (Repeatability, ValidDistance, Angle)@t.., EPI@t..] float64.  Quotients of counts are fp32
        quotients; a quotient with an empty denominator is NaN."""
        nan = float("nan")
        q32 = lambda a, b: float(np.float32(a) / np.float32(b)) if b > 0 else nan  # noqa: E731
        out = [self.M / (min(self.n, self.m) + 1e-8)]
        J = int(self.judged.sum())
        for t in mma_thr:
            out.append(q32(self.mma_good(t).sum(), J) if self.has_depth else nan)
        out.append(q32(J, self.M) if self.has_depth else nan)
        for t in vdd_thr:
            rep = vd = ang = nan
            if self.has_depth and self.N1 != 0 and self.N2 != 0:
                s0, s1 = self.selected(t)
                c = F64(s0.sum() + s1.sum())
                rep = float(np.float32(c) / np.float32(self.N1 + self.N2))
                dist = np.concatenate([self.desc_d[0][s0], self.desc_d[1][s1]]).astype(np.float32).astype(F64)
                with np.errstate(invalid="ignore"):
                    vd = float(dist.sum() / c)
                    ang = float(np.concatenate([self.angle[0][s0], self.angle[1][s1]]).sum() / c)
            out += [rep, vd, ang]
        for t in epi_thr:
            assert (np.abs(self.epi - t) > EPI_MARGIN).all(), "an epipolar distance within 1e-6 of a threshold"
            out.append(q32((self.epi <= t).sum(), self.M))
        return np.array(out, F64)


# ------------------------------------------------------------------------------------------------ exact geometries
def _kmat(c):
    return np.array([[FOCAL, 0, c[0]], [0, FOCAL, c[1]], [0, 0, 1.0]])


class Geometry:
    """view 0 -> view 1: rotation by `theta` degrees about the optical axis, then the pixel shift s = t_xy f / d on the plane d.
    On d = 2: proj(x) = Rz (x - c0) + s + c1, exact on the keypoint lattices; `shift` is s for d = 2 (half-integers, so that a
    half-integer keypoint lands on a whole pixel coordinate such as 0 or W1 exactly)."""

    def __init__(self, theta, c0, c1, shift, tz=0.0):
        self.theta, self.c0, self.c1, self.shift = theta, np.array(c0, F64), np.array(c1, F64), np.array(shift, F64)
        self.K0, self.K1 = _kmat(c0), _kmat(c1)
        self.R2 = np.array(RZ[theta], F64)[:2, :2]
        self.T01 = np.eye(4)
        self.T01[:3, :3] = RZ[theta]
        self.T01[:3, 3] = [shift[0] * PLANE / FOCAL, shift[1] * PLANE / FOCAL, tz]
        self.T10 = invert_pose(self.T01)

    def fwd(self, xy, d=PLANE):
        return (np.asarray(xy, F64) - self.c0) @ self.R2.T + self.shift * (PLANE / d) + self.c1

    def inv(self, uv, d=PLANE):
        return (np.asarray(uv, F64) - self.c1 - self.shift * (PLANE / d)) @ self.R2 + self.c0


GEOMETRIES = {
    # u = x - 2.5, v = y - 1.5: u == 0 at x = 2.5 and u == W1 at x = 58.5, both inside image 0
    "shift": Geometry(0, (32, 24), (28, 20), (1.5, 2.5)),
    # u = 45.5 - y, v = x - 14.5
    "rot90": Geometry(90, (32, 24), (28, 20), (-6.5, -2.5)),
    # u = 61.5 - x, v = 44.5 - y
    "rot180": Geometry(180, (32, 24), (28, 20), (1.5, 0.5)),
    # the same camera twice and no motion: F = 0, every match passes EPI
    "identity": Geometry(0, (28, 20), (28, 20), (0.0, 0.0)),
    # q.z = 2 - 6 = -4 for view 0 (behind camera 1: N1 = 0, nothing judged), 2 + 6 = 8 for view 1
    "behind": Geometry(0, (32, 24), (28, 20), (1.5, 2.5), tz=-6.0),
}


def on_lattice(p):
    """wholly on the half-integer grid or wholly on odd quarters"""
    fr = np.mod(np.asarray(p, F64), 1.0)
    return bool((fr == 0.5).all() or np.isin(fr, (0.25, 0.75)).all())


def _lattice(r, k, lo, hi):
    """k points in the box [lo, hi) (x, y): even rows on the half-integer grid, odd rows on odd quarters"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    cell = np.stack([r.integers(lo[0], hi[0], k), r.integers(lo[1], hi[1], k)], 1).astype(F64)
    quarter = 0.25 + 0.5 * r.integers(0, 2, (k, 2))
    return cell + np.where((np.arange(k) % 2 == 0)[:, None], 0.5, quarter)


def off_the_rim(p, size):
    """points (x, y) for a map of `size` (H, W): a coordinate of 1/4 or size - 1/4 has a bilinear footprint with weight 3/4 inside the
    map and 1/4 outside (zero padding), a depth of 3/2 and an inexact quotient; moved half a pixel inwards"""
    p = np.array(p, F64)
    for axis, s in ((0, size[1]), (1, size[0])):
        p[p[:, axis] == 0.25, axis] = 0.75
        p[p[:, axis] == s - 0.25, axis] = s - 0.75
    return p


def holed_plane(seed, size, depth=PLANE, share=20):
    """the plane with one hole in `share` pixels (0, negative, NaN in turn)"""
    r = np.random.default_rng(seed)
    d = np.full(size, depth)
    h = r.integers(0, share, size)
    k = r.integers(0, 3, size)
    d[(h == 0) & (k == 0)], d[(h == 0) & (k == 1)], d[(h == 0) & (k == 2)] = 0.0, -1.0, np.nan
    return d


# offsets (dx, dy) in multiples of 1/2: distance exactly t, and the next lattice distance beyond it (metrics_f64.AT / ABOVE)
AT = {1: (1.0, 0.0), 2.5: (1.5, 2.0), 3: (0.0, 3.0), 5: (3.0, 4.0)}
ABOVE = {1: (0.5, 1.0), 2.5: (0.5, 2.5), 3: (0.5, 3.0), 5: (0.5, 5.0)}
OFFSETS = [(0.0, 0.0)] + list(AT.values()) + list(ABOVE.values())
EDGE_U = (0.0, -0.25, 0.25)  # and W1 + each: exactly on the bound and a quarter pixel either side


def make_pair(seed, n, m, M, D, cols, kp_yx, geom, matches="any", extra=0):
    """One pair under GEOMETRIES[geom]: float32 k0 [n,3], k1 [m,3], d0, d1, mk0 / mk1 [M,cols], depth0 / depth1 (extra pixels
    wider and higher than the images: the bound of `keep` is the image, not the map) and info.
    View 1's keypoints B are drawn in image 1's frame (a margin outside it included), view 0's are preimages of points A drawn in
    the same frame; planted: A on u == 0 / W1 / v == 0 / H1 and a quarter pixel either side, B at A + an offset of OFFSETS (distance
    exactly a threshold, or the next lattice distance), two B equidistant from an A.
    matches: "any", or "holes" (every matched row of view 0 sits on a hole: nothing is judged)."""
    r = np.random.default_rng(seed)
    g = GEOMETRIES[geom]
    (H0, W0), (H1, W1) = SIZE0, SIZE1
    depth0 = holed_plane(seed + 1, (H0 + extra, W0 + extra))
    depth1 = holed_plane(seed + 2, (H1 + extra, W1 + extra))
    # a lattice point plus (1/2, 1/2): every shift of GEOMETRIES is a half-integer, so the preimage is on a lattice again
    p0 = g.inv(_lattice(r, n, (-3, -3), (W1 + 3, H1 + 3)) + 0.5)
    if n and not on_lattice(p0[0]):  # a whole-pixel shift ("identity")
        p0 -= 0.5
    A = g.fwd(off_the_rim(p0, depth0.shape))
    B = off_the_rim(_lattice(r, m, (-3, -3), (W1 + 3, H1 + 3)), depth1.shape)
    info = {"edges": [], "planted": [], "ties": []}
    # edges: view 0's keypoints whose projection is on a bound of image 1, where the preimage is on a lattice inside image 0
    k = 0
    for axis, bound in ((0, 0.0), (0, float(W1)), (1, 0.0), (1, float(H1))):
        for off in EDGE_U:
            if k >= n // 2:
                break
            a = np.array([10.0 + k, 10.0 + k]) + (0.0 if off == 0.0 else 0.25)  # whole numbers are half-integers of view 0
            a[axis] = bound + off
            x = g.inv(a)
            if on_lattice(x) and 0.5 <= x[0] <= W0 - 0.5 and 0.5 <= x[1] <= H0 - 0.5:
                A[k] = a
                x0, y0 = int(np.floor(x[0] - 0.5)), int(np.floor(x[1] - 0.5))
                depth0[y0:y0 + 2, x0:x0 + 2] = PLANE  # no hole under a planted point
                info["edges"].append((k, axis, bound, off))
                k += 1
    # neighbours at planted distances: B[j] = A[i] + offset for quarter-lattice A (odd i), where B stays on a lattice
    j = 0
    for i in range(k | 1, n, 2):
        if j + 2 > m or i % 3 == 0:
            continue
        off = np.array(OFFSETS[(i // 2) % len(OFFSETS)])
        b = A[i] + off
        if not on_lattice(b) or (off_the_rim(b[None], depth1.shape) != b).any() or (off_the_rim((A[i] - off)[None], depth1.shape) != A[i] - off).any():
            continue
        B[j] = b
        info["planted"].append((i, j, tuple(off)))
        j += 1
        if (i // 2) % 4 == 0 and off.any():  # a second candidate at the same distance: the lower index wins
            B[j] = A[i] - off
            info["ties"].append((i, j - 1, j))
            j += 1
    p0 = g.inv(A)
    assert all(on_lattice(p) for p in p0) and all(on_lattice(p) for p in B)
    xy = [1, 0] if kp_yx else [0, 1]
    k0, k1 = np.zeros((n, 3), np.float32), np.zeros((m, 3), np.float32)
    k0[:, xy], k1[:, xy] = p0, B
    k0[:, 2], k1[:, 2] = r.random(n), r.random(m)
    d0, d1 = exact_unit(seed + 3, n, D), exact_unit(seed + 4, m, D)
    for i, jb, _ in info["planted"][::2]:  # identical descriptors on half of the planted neighbours: angle exactly 0
        d1[jb] = d0[i]
    # matches: view 0's row on a lattice inside image 0, view 1's row at its true projection plus an offset
    q0 = off_the_rim(_lattice(r, M, (0, 0), (W0, H0)), depth0.shape)
    if matches == "holes":
        ys, xs = np.nonzero(~(depth0[:H0, :W0] > 0))
        pick = r.integers(0, len(ys), M)
        q0 = np.stack([xs[pick] + 0.5, ys[pick] + 0.5], 1)
    q1 = g.fwd(q0)
    for i in range(M):
        off = np.array(OFFSETS[int(r.integers(len(OFFSETS)))]) if r.random() < 0.6 else r.integers(-12, 13, 2) * 0.5
        q1[i] += -off[::-1] if r.random() < 0.5 else off
    mk0, mk1 = np.zeros((M, cols), np.float32), np.zeros((M, cols), np.float32)
    mk0[:, xy], mk1[:, xy] = q0, q1
    if cols == 3:
        mk0[:, 2], mk1[:, 2] = r.random(M), r.random(M)
    return k0, k1, d0, d1, mk0, mk1, depth0.astype(np.float32), depth1.astype(np.float32), info


# ------------------------------------------------------------------------------------------------ the cases
# name -> B, cap0, cap1, D, [(n, m, nmatch)], kp_yx, cols, reprojection thresholds (MMA and VDD), EPI thresholds, geometry per pair,
# pass T_1to0 (else NULL), extra depth-map pixels, occlusion_th.  The smallest shapes that reach each path (metrics_f64.CASES).
CASES = {
    "ragged": dict(B=3, caps=(65, 130), D=36, counts=[(65, 130, 40), (64, 1, 1), (0, 100, 0)], kp_yx=True, cols=3, thr=(1, 3, 5),
                   epi=(0.5, 2), geoms=("shift", "rot90", "rot180"), t10=False, extra=0, occ=None),
    "trip_edge": dict(B=2, caps=(256, 257), D=64, counts=[(256, 257, 100), (255, 256, 255)], kp_yx=False, cols=2, thr=(1, 2.5, 3, 5),
                      epi=(1,), geoms=("rot180", "shift"), t10=True, extra=4, occ=None),
    "past_1024": dict(B=1, caps=(1030, 1040), D=36, counts=[(1030, 1040, 64)], kp_yx=True, cols=3, thr=(1, 3), epi=(),
                      geoms=("rot90",), t10=False, extra=0, occ=None),
    "matches_beyond_256": dict(B=2, caps=(320, 16), D=36, counts=[(10, 12, 300), (8, 6, 0)], kp_yx=True, cols=2, thr=(1, 2.5, 3, 5),
                               epi=(0.5, 1, 2, 4), geoms=("shift", "rot90"), t10=False, extra=0, occ=None),
    "d4": dict(B=2, caps=(20, 30), D=4, counts=[(20, 30, 10), (7, 5, 3)], kp_yx=False, cols=2, thr=(3,), epi=(1,),
               geoms=("rot90", "shift"), t10=True, extra=0, occ=None),
    "d257": dict(B=2, caps=(30, 40), D=257, counts=[(30, 40, 12), (9, 17, 5)], kp_yx=True, cols=3, thr=(1, 5), epi=(),
                 geoms=("shift", "rot180"), t10=False, extra=0, occ=None),
    # pair 0: every matched row on a hole (MMA NaN, judged_ratio 0); pair 1: behind camera 1 (N1 = 0: NaN triple, MR intact);
    # pair 2: no motion at all (every match passes EPI)
    "unjudged": dict(B=3, caps=(40, 48), D=36, counts=[(40, 48, 20), (30, 40, 16), (36, 36, 24)], kp_yx=True, cols=3, thr=(1, 3),
                     epi=(1, 3), geoms=("shift", "behind", "identity"), t10=False, extra=0, occ=None, matches=("holes", "any", "any")),
    # the occlusion check on a scene it does not change much: every consistent point comes back to itself exactly
    "occlusion_on": dict(B=2, caps=(65, 70), D=36, counts=[(65, 70, 40), (33, 70, 20)], kp_yx=True, cols=3, thr=(1, 3), epi=(1,),
                         geoms=("rot90", "shift"), t10=False, extra=4, occ=1.0),
}
CASE_NAMES = list(CASES)


class Case:
    """Padded float32 arrays of one case (NaN in every row past a pair's count) and pairs[b], the restatement of pair b.  `family`
    keeps the (name, family, pair) keys of test_metrics_f64_gpu's angle-bound cache apart from metrics_f64's cases."""

    def row(self, b):
        return self.pairs[b].row(self.thr, self.thr, self.epi)

    def restate(self, b, dt=F64, depth=True, occ="case"):
        n, m, M = self.n[b], self.m[b], self.nm[b]
        return RestatedPose(self.k0[b, :n], self.k1[b, :m], self.d0[b, :n], self.d1[b, :m], self.mk0[b, :M], self.mk1[b, :M], self.size0,
                            self.size1, self.K0[b], self.K1[b], self.T01[b], None if self.T10 is None else self.T10[b],
                            self.depth0[b] if depth else None, self.depth1[b] if depth else None, self.occ if occ == "case" else occ,
                            self.kp_yx, dt)


_CACHE = {}


def build_case(name):
    if name in _CACHE:
        return _CACHE[name]
    s = CASES[name]
    c = Case()
    c.name, c.family, c.B, (c.cap0, c.cap1), c.D = name, "pose", s["B"], s["caps"], s["D"]
    c.kp_yx, c.cols, c.thr, c.epi, c.occ = s["kp_yx"], s["cols"], s["thr"], s["epi"], s["occ"]
    c.size0, c.size1 = SIZE0, SIZE1
    B, e = c.B, s["extra"]
    seed = zlib.crc32(name.encode()) % 100000 * 1000
    c.k0, c.k1 = np.full((B, c.cap0, 3), np.nan, np.float32), np.full((B, c.cap1, 3), np.nan, np.float32)
    c.d0, c.d1 = np.full((B, c.cap0, c.D), np.nan, np.float32), np.full((B, c.cap1, c.D), np.nan, np.float32)
    c.mk0, c.mk1 = (np.full((B, c.cap0, c.cols), np.nan, np.float32) for _ in range(2))
    c.depth0 = np.zeros((B, SIZE0[0] + e, SIZE0[1] + e), np.float32)
    c.depth1 = np.zeros((B, SIZE1[0] + e, SIZE1[1] + e), np.float32)
    c.n, c.m, c.nm = ([v[i] for v in s["counts"]] for i in range(3))
    gs = [GEOMETRIES[g] for g in s["geoms"]]
    c.K0, c.K1 = np.stack([g.K0 for g in gs]).astype(np.float32), np.stack([g.K1 for g in gs]).astype(np.float32)
    c.T01 = np.stack([g.T01 for g in gs]).astype(np.float32)
    c.T10 = np.stack([g.T10 for g in gs]).astype(np.float32) if s["t10"] else None
    c.info, c.pairs = [], []
    for b, (n, m, M) in enumerate(s["counts"]):
        k0, k1, d0, d1, mk0, mk1, c.depth0[b], c.depth1[b], info = make_pair(seed + 10 * b, n, m, M, c.D, c.cols, c.kp_yx, s["geoms"][b],
                                                                             s.get("matches", ("any",) * B)[b], e)
        c.k0[b, :n], c.k1[b, :m], c.d0[b, :n], c.d1[b, :m], c.mk0[b, :M], c.mk1[b, :M] = k0, k1, d0, d1, mk0, mk1
        c.info.append(info)
    c.pairs = [c.restate(b) for b in range(B)]
    _CACHE[name] = c
    return c


# ------------------------------------------------------------------------------------------------ a two-layer scene
_LAYERS = None


def two_layer_case():
    """One pair, no rotation, cameras alike, t = (3/32, 0, 0): a point of the background (d = 2) moves 1.5 px to the right, one of
    the foreground (d = 1) 3 px.  View 0 sees only background.  View 1's map holds a foreground strip in columns 20..29: a
    background keypoint of view 0 that projects into the strip is hidden behind it there.  Sampled at its projection the strip says
    d = 1, the way back is 3 px instead of 1.5 px, and the point returns 1.5 px from where it started: occlusion_th = 1 drops it,
    occlusion_th = 0 (off) keeps it.  View 1's keypoints on the strip project with d = 1 to 3 px left of themselves, where view 0's
    map says d = 2: they come back 1.5 px off and are dropped as well.  No holes, so that nothing else changes."""
    global _LAYERS
    if _LAYERS is not None:
        return _LAYERS
    c = Case()
    c.name, c.family, c.B, c.cap0, c.cap1, c.D = "two_layer", "pose", 1, 70, 66, 36
    # the motion is along x: a match's epipolar distance is |dy|, a multiple of 1/2 -- the EPI threshold keeps 1/4 away from those
    c.kp_yx, c.cols, c.thr, c.epi, c.occ = True, 3, (1, 3), (0.75,), 1.0
    c.size0 = c.size1 = SIZE1
    H, W = SIZE1
    g = Geometry(0, (28, 20), (28, 20), (1.5, 0.0))
    r = np.random.default_rng(424242)
    n, m, M = 64, 60, 30
    c.n, c.m, c.nm = [n], [m], [M]
    d0, d1 = np.full((H, W), PLANE), np.full((H, W), PLANE)
    d1[:, 20:30] = 1.0
    def clear(p, dx):  # no bilinear footprint of view 1's map at x + dx across a border of the strip: a mixed depth is no power of two
        first = np.floor(p[:, 0] + dx - 0.5)
        p[(p[:, 0] + dx - 0.5 != first) & np.isin(first, (19, 29)), 0] += 3.0
        return p

    def on_strip(p, dx):  # every tap of the footprint at x + dx reads the strip
        first = np.floor(p[:, 0] + dx - 0.5)
        return (first >= 20) & (np.ceil(p[:, 0] + dx - 0.5) <= 29)

    p0 = clear(_lattice(r, n, (2, 2), (W - 8, H - 2)), 1.5)
    p0[:8] = np.stack([19.5 + np.arange(8), 5.5 + 3 * np.arange(8)], 1)  # project to u = 21 .. 28: inside the strip
    p1 = clear(_lattice(r, m, (4, 2), (W - 8, H - 2)), 0.0)
    p1[:6] = np.stack([21.5 + np.arange(6), 8.5 + 4 * np.arange(6)], 1)  # on the strip
    q0 = clear(_lattice(r, M, (2, 2), (W - 8, H - 2)), 1.5)
    q0[:5] = p0[:5]  # matches whose point is hidden in view 1: unjudged under the occlusion check
    q1 = g.fwd(q0) + r.integers(-4, 5, (M, 2)) * 0.5
    c.k0, c.k1 = np.full((1, c.cap0, 3), np.nan, np.float32), np.full((1, c.cap1, 3), np.nan, np.float32)
    c.mk0, c.mk1 = (np.full((1, c.cap0, 3), np.nan, np.float32) for _ in range(2))
    for dst, src in ((c.k0[0, :n], p0), (c.k1[0, :m], p1), (c.mk0[0, :M], q0), (c.mk1[0, :M], q1)):
        dst[:, [1, 0]], dst[:, 2] = src, r.random(len(src))
    c.d0, c.d1 = np.full((1, c.cap0, c.D), np.nan, np.float32), np.full((1, c.cap1, c.D), np.nan, np.float32)
    c.d0[0, :n], c.d1[0, :m] = exact_unit(1, n, c.D), exact_unit(2, m, c.D)
    c.depth0, c.depth1 = d0[None].astype(np.float32), d1[None].astype(np.float32)
    c.K0, c.K1, c.T01, c.T10 = g.K0[None].astype(np.float32), g.K1[None].astype(np.float32), g.T01[None].astype(np.float32), None
    # what the strip hides: the planted rows first, whatever else of the random rows lands there too
    c.hidden0, c.hidden1, c.hidden_matches = on_strip(p0, 1.5), on_strip(p1, 0.0), on_strip(q0, 1.5)
    assert c.hidden0[:8].all() and c.hidden1[:6].all() and c.hidden_matches[:5].all()
    c.pairs = [c.restate(0)]
    c.pairs_off = [c.restate(0, occ=0.0)]
    _LAYERS = c
    return c


# ------------------------------------------------------------------------------------------------ the induced homography
def induced_homography(geom):
    """the homography that view 0 -> view 1 is on the plane d = 2: [[R2, s + c1 - R2 c0], [0, 0, 1]]"""
    g = GEOMETRIES[geom]
    H = np.eye(3)
    H[:2, :2] = g.R2
    H[:2, 2] = g.shift + g.c1 - g.R2 @ g.c0
    return H
