"""core.geometry.depth and the two epipolar distances restated in dense numpy, and inputs on which fp32 computes
them exactly.

Not collected by pytest (no test_ prefix).  tests/test_geometry_cpu.py checks this restatement against itself in float32, and
against the reference's fixture tests/golden/geometry.npz; tests/test_geometry_gpu.py compares the kernels of csrc/geometry.hip
with it.

Written from the reference's text (depth.py:9-89, epipolar.py:32-72, the pinhole Camera / Pose it calls) for ONE pair, with
numpy's own operators; every function takes the dtype it computes in.  The inputs follow the exact-input recipe of
tests/gt_matches_f64.py: keypoints on a lattice of quarter pixels (wholly on the half-integer grid or wholly on odd quarters),
depths that are powers of two on piecewise constant surfaces, f = 32, rotations about the optical axis by multiples of 90
degrees, a translation of (1/4, -1/8, 0) -- a parallax of (4, -2) whole pixels at depth 2, (8, -4) at depth 1 and (2, -1) at depth
4, so a keypoint and its projection are on the same kind of lattice point -- so that the sampler, both projections and the squared
cycle distance are exact in fp32.  A point of the plane at depth 2 whose projection meets a surface at half its depth in the other
map comes back (4, -2) pixels off: a squared cycle distance of exactly 20, which is what lets a test put the bound ON a distance.

Where the reference and the 8e sampler contract part ways -- a NaN tap of weight zero beside taps of non-zero weight, which only a
point on the grid in one coordinate and off it in the other can have -- no case goes: every sampled point is wholly on the
half-integer grid or wholly on odd quarters."""
import numpy as np

import gt_matches_f64 as G
from gt_matches_f64 import EPS_Z, RZ, Case, _kmat, _lattice_points, _pose, ints, invert_pose, project_side  # noqa: F401

F64 = np.float64


# ------------------------------------------------------------------------------------------------ the restatement
def _sample(xy, fm, dt):
    """depth.py:9-17 for one channel fm [H,W] whose holes are NaN: bilinear with zero padding at ix = x - 0.5 (a tap outside the
    map contributes 0), a NaN tap poisons the sum (also at weight zero); a NaN sum is replaced by the nearest pixel (half to even),
    0 outside the map"""
    xy, fm = np.asarray(xy, dt), np.asarray(fm, dt)
    H, W = fm.shape
    with np.errstate(invalid="ignore"):
        ix, iy = xy[:, 0] - dt(0.5), xy[:, 1] - dt(0.5)
        x0, y0 = np.floor(ix), np.floor(iy)

        def pixel(xx, yy):
            inmap = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            return inmap, fm[np.where(inmap, yy, 0).astype(np.int64), np.where(inmap, xx, 0).astype(np.int64)]

        total = np.zeros(len(xy), dt)
        for yy, wy in ((y0, y0 + dt(1) - iy), (y0 + dt(1), iy - y0)):
            for xx, wx in ((x0, x0 + dt(1) - ix), (x0 + dt(1), ix - x0)):
                inmap, tap = pixel(xx, yy)
                total = total + np.where(inmap, tap * (wx * wy), dt(0))
        inmap, tap = pixel(np.rint(ix), np.rint(iy))
        near = np.where(inmap, tap, dt(0))
        return np.where(np.isnan(total), near, total).astype(dt)


def sample_fmap(xy, fmap, dt=F64):
    """xy [n,2], fmap [C,H,W] -> [n,C]"""
    return np.stack([_sample(xy, ch, dt) for ch in np.asarray(fmap, dt)], 1)


def sample_depth(xy, depth, dt=F64):
    """depth.py:20-25: xy [n,2], depth [H,W] -> d [n], valid [n]"""
    depth = np.asarray(depth, dt)
    with np.errstate(invalid="ignore"):
        d = _sample(xy, np.where(depth > 0, depth, dt(np.nan)), dt)
        return d, ~np.isnan(d) & (d > 0)


def project(xy, d, valid, K_i, K_j, T, depth_j=None, ccth=None, dt=F64, dj=None):
    """depth.py:37-69: -> uv [n,2], visible [n], info.  Without depth_j (or dj = (depths, validity) under the projections) or
    without ccth: no cycle check."""
    xy, d = np.asarray(xy, dt), np.asarray(d, dt)
    uv, vis, fwd = project_side(xy, d, np.asarray(valid, bool), K_i, K_j, T, dt)
    info = {"forward": vis, "front": fwd["front"], "inside": fwd["inside"]}
    if (depth_j is None and dj is None) or ccth is None:
        return uv, vis, info
    dj, validj = sample_depth(uv, depth_j, dt) if dj is None else (np.asarray(dj[0], dt), np.asarray(dj[1], bool))
    back, back_ok, binfo = project_side(uv, dj, np.ones(len(uv), bool), K_j, K_i, invert_pose(T, dt), dt)
    with np.errstate(invalid="ignore", over="ignore"):
        dist = ((xy - back) ** 2).sum(-1)
        consistent = dist < dt(ccth)
    info.update(dj=dj, validj=validj, back_ok=back_ok, back_front=binfo["front"], back_inside=binfo["inside"], dist=dist,
                consistent=consistent)
    return uv, vis & consistent & back_ok & validj, info


def dense_warp(depth_i, depth_j, K_i, K_j, T, ccth=None, dt=F64):
    """depth.py:72-89: every pixel centre of depth_i at the pixel's own value -> warp [Hi,Wi,2], visible [Hi Wi] (the caller shapes
    it like depth_j), counts (valid, visible), info"""
    depth_i = np.asarray(depth_i, dt)
    H, W = depth_i.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=dt), np.arange(W, dtype=dt), indexing="ij")
    xy = np.stack([xx, yy], -1).reshape(-1, 2) + dt(0.5)
    di = depth_i.reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = di > 0
    uv, vis, info = project(xy, di, valid, K_i, K_j, T, depth_j, ccth, dt)
    return uv.reshape(H, W, 2), vis, (int(valid.sum()), int(vis.sum())), info


def _hom(p, dt):
    p = np.asarray(p, dt)
    return p if p.shape[-1] == 3 else np.concatenate([p, np.ones(p.shape[:-1] + (1,), dt)], -1)


def epipolar_all(p0, p1, E, eps=1e-15, dt=F64):
    """epipolar.py:59-72: p0 [n,2|3], p1 [m,2|3], E [3,3] -> [n,m]"""
    p0, p1, E = _hom(p0, dt), _hom(p1, dt), np.asarray(E, dt)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.abs(np.einsum("mi,ij,nj->nm", p1, E, p0))
        l1, l0 = np.einsum("ij,nj->ni", E, p0), np.einsum("ij,mi->mj", E, p1)
        d0 = s / np.sqrt(l1[:, None, 0] ** 2 + l1[:, None, 1] ** 2 + dt(eps))
        d1 = s / np.sqrt(l0[None, :, 0] ** 2 + l0[None, :, 1] ** 2 + dt(eps))
        return ((d0 + d1) / dt(2)).astype(dt)


def epipolar_pairs(p0, p1, E, squared=True, dt=F64):
    """epipolar.py:32-56: paired points [n,2|3] -> [n]"""
    p0, p1, E = _hom(p0, dt), _hom(p1, dt), np.asarray(E, dt)
    s = np.einsum("ni,ij,nj->n", p1, E, p0)
    l1, l0 = np.einsum("ij,nj->ni", E, p0), np.einsum("ij,ni->nj", E, p1)
    d0 = np.maximum(l1[:, 0] ** 2 + l1[:, 1] ** 2, dt(1e-6))
    d1 = np.maximum(l0[:, 0] ** 2 + l0[:, 1] ** 2, dt(1e-6))
    if squared:
        return (s ** 2 * (dt(1) / d0 + dt(1) / d1)).astype(dt)
    return (np.abs(s) * (dt(1) / np.sqrt(d0) + dt(1) / np.sqrt(d1)) / dt(2)).astype(dt)


# ------------------------------------------------------------------------------------------------ the occlusion scene
SIZE = 64           # cameras and depth maps are 64 x 64 (a power of two: the reference's own sampler is exact on it too): f = 32, c = (32, 32)
FAR, NEAR, BEHIND = 2.0, 1.0, 4.0
T_XY = (1 / 4, -1 / 8, 0.0)
BOUND_EQ = 20.0           # the squared cycle distance of a point hidden by a surface at half its depth: |(4, -2)|^2
BOUND_ABOVE = 20.0625     # one step of the quarter-pixel lattice's squared distances (1/16) above it
ROTATIONS = (180, 90, 0)
PROJECT_N = (1, 255, 256, 257)
_SCENES = {}


def _surface(seed):
    """a 64 x 64 map: the plane at depth 2, a rectangle of a nearer surface (depth 1) and one of a farther one (depth 4), 4 % holes
    (0, negative, NaN)"""
    d = np.full((SIZE, SIZE), FAR)
    y0, x0 = 6 + int(ints(seed, (1,), 8)[0]), 6 + int(ints(seed + 1, (1,), 8)[0])
    d[y0:y0 + 16, x0:x0 + 14] = NEAR
    d[y0 + 20:y0 + 28, x0 + 4:x0 + 20] = BEHIND
    r = ints(seed + 2, d.shape, 75)
    d[r == 0], d[r == 1], d[r == 2] = 0.0, -1.0, np.nan
    return d


def _snap_mixed(xy, depth):
    """odd-quarter keypoints whose own sample mixes two surfaces (a depth that is no power of two leaves q.x / q.z inexact) move to
    the centre of their pixel"""
    d, valid = sample_depth(xy, depth)
    mixed = valid & ~np.isin(d, (FAR, NEAR, BEHIND))
    xy = xy.copy()
    xy[mixed] = np.floor(xy[mixed]) + 0.5
    return xy


def occlusion_scene(n):
    """three pairs (rotation by 180, 90 and 0 degrees about the optical axis, t = (1/4, -1/8, 0)) with n keypoints per side,
    ragged counts in pairs 1 and 2.  c.pre[b] = (d0, valid0, d1, valid1): the restatement's own samples, except for the first
    keypoint of each side (n > 1), which sits where its ray meets the other camera's centre at depth -1, valid: behind the other
    camera, q = (0, 0, -1), u = c exactly."""
    if n in _SCENES:
        return _SCENES[n]
    c = Case()
    c.B, c.cap = 3, n
    c.n = [n, max(1, n - 3), max(1, n - 1)]
    c.m = [n, max(1, n - 1), max(1, n - 2)]
    K = _kmat(32, SIZE / 2, SIZE / 2)
    c.K0 = c.K1 = np.stack([K] * 3).astype(np.float32)
    Ts = [_pose(RZ[r], T_XY) for r in ROTATIONS]
    c.T01 = np.stack(Ts).astype(np.float32)
    c.T10 = np.stack([invert_pose(T) for T in Ts]).astype(np.float32)
    c.depth0 = np.stack([_surface(300 + 10 * b + n) for b in range(3)])
    c.depth1 = np.stack([_surface(400 + 10 * b + n) for b in range(3)])
    c.kp0, c.kp1, c.pre = [], [], []
    for b in range(3):
        sides = []
        for side, (cnt, dm, T) in enumerate(((c.n[b], c.depth0[b], Ts[b]), (c.m[b], c.depth1[b], invert_pose(Ts[b])))):
            first = SIZE / 2 + 32.0 * (T[:3, :3].T @ T[:3, 3])[:2]  # R p + t = (0, 0, -1) for p = (x - c) / f * d with d = -1: x = c + f R^T t
            if n > 1:  # an integer point: its four taps read one surface
                dm[int(first[1]) - 1:int(first[1]) + 1, int(first[0]) - 1:int(first[0]) + 1] = FAR
            xy = _snap_mixed(_lattice_points(500 + 20 * b + side + 7 * n, cnt, SIZE, SIZE), dm)
            if n > 1:
                xy[0] = first
            d, valid = sample_depth(xy, dm)
            if n > 1:
                d[0], valid[0] = -1.0, True
            sides.append((xy.astype(np.float32), d.astype(np.float32), valid))
        c.kp0.append(sides[0][0])
        c.kp1.append(sides[1][0])
        c.pre.append((sides[0][1], sides[0][2], sides[1][1], sides[1][2]))
    # holes under the projections of three valid, forward-visible keypoints per side of pair 0: 0, NaN, negative
    if n >= 255:
        for side, (kp, dm_self, dm_other, K_, T) in enumerate(((c.kp0[0], c.depth0[0], c.depth1[0], K, Ts[0]),
                                                                (c.kp1[0], c.depth1[0], c.depth0[0], K, invert_pose(Ts[0])))):
            d, valid = sample_depth(kp, dm_self)
            uv, vis, _ = project(kp, d, valid, K_, K_, T)
            on_grid = vis & (np.mod(uv, 1.0) == 0.5).all(1)
            on_grid[0] = False
            for k, hole in zip(np.nonzero(on_grid)[0][:3], (0.0, np.nan, -2.0)):
                dm_other[int(uv[k, 1] - 0.5), int(uv[k, 0] - 0.5)] = hole
            # a nearer surface under the projection of a consistent keypoint close to its own image's border: the way back ends outside
            _, _, info = project(kp, d, valid, K_, K_, T, dm_other, BOUND_ABOVE)
            for k in np.nonzero(on_grid & info["validj"] & (info["dist"] == 0) & (d == FAR) & ((kp < 4).any(1) | (kp > SIZE - 4).any(1)))[0]:
                y, x = int(uv[k, 1] - 0.5), int(uv[k, 0] - 0.5)
                dm_other[y, x] = NEAR
                if not project(kp[k:k + 1], d[k:k + 1], valid[k:k + 1], K_, K_, T, dm_other, BOUND_ABOVE)[2]["back_ok"][0]:
                    break
                dm_other[y, x] = FAR
        # the planted pixels sit in maps the other side samples its own depths from: off-grid keypoints that now mix two surfaces move
        # to their pixel's centre, and the samples are taken again
        for b in (0,):
            c.kp0[b][1:] = _snap_mixed(c.kp0[b][1:], c.depth0[b]).astype(np.float32)
            c.kp1[b][1:] = _snap_mixed(c.kp1[b][1:], c.depth1[b]).astype(np.float32)
            d0, v0 = sample_depth(c.kp0[b], c.depth0[b])
            d1, v1 = sample_depth(c.kp1[b], c.depth1[b])
            d0[0], v0[0], d1[0], v1[0] = -1.0, True, -1.0, True
            c.pre[b] = (d0.astype(np.float32), v0, d1.astype(np.float32), v1)
    c.depth0, c.depth1 = c.depth0.astype(np.float32), c.depth1.astype(np.float32)
    _SCENES[n] = c
    return c


_EXPECT = {}


def occlusion_expected(n, ccth, T10_given, precomputed, dt=F64):
    """the restatement of both directions of every pair: a list of dicts with gt_matches_f64.STAGE_A_KEYS plus side0 / side1 info"""
    key = (n, ccth, T10_given, precomputed, np.dtype(dt).name)
    if key in _EXPECT:
        return _EXPECT[key]
    c, out = occlusion_scene(n), []
    for b in range(c.B):
        T01 = np.asarray(c.T01[b], dt)
        T10 = np.asarray(c.T10[b], dt) if T10_given else invert_pose(T01, dt)
        if precomputed:
            d0, v0, d1, v1 = c.pre[b]
        else:
            (d0, v0), (d1, v1) = sample_depth(c.kp0[b], c.depth0[b], dt), sample_depth(c.kp1[b], c.depth1[b], dt)
        p01, vis0, i0 = project(c.kp0[b], d0, v0, c.K0[b], c.K1[b], T01, c.depth1[b], ccth, dt)
        p10, vis1, i1 = project(c.kp1[b], d1, v1, c.K1[b], c.K0[b], T10, c.depth0[b], ccth, dt)
        out.append({"depth_keypoints0": np.asarray(d0, dt), "depth_keypoints1": np.asarray(d1, dt), "valid0": np.asarray(v0, bool),
                    "valid1": np.asarray(v1, bool), "proj_0to1": p01, "proj_1to0": p10, "visible0": vis0, "visible1": vis1, "side0": i0,
                    "side1": i1})
    _EXPECT[key] = out
    return out


# ------------------------------------------------------------------------------------------------ dense warp cases
DENSE_SHAPES = {"5x7": ((5, 7), (5, 7)), "16x16": ((16, 16), (16, 16)), "33x45": ((33, 45), (33, 45)), "12x20_to_15x16": ((12, 20), (15, 16))}
_DENSE = {}


def dense_case(name):
    """two pairs with different cameras: f = 32 and c = (W // 2, H // 2) in pair 0, c = (W // 2 + 1, H // 2 - 1) in pair 1 (integers:
    a pixel centre projects onto a pixel centre); rotation by 180 and 0 degrees, t = (1/4, -1/8, 0) and (1/16, 1/16, 0): whole-pixel
    parallax at depths 2 and 1; the maps hold the plane at depth 2, a nearer rectangle and holes"""
    if name in _DENSE:
        return _DENSE[name]
    (Hi, Wi), (Hj, Wj) = DENSE_SHAPES[name]
    c = Case()
    c.B, c.size_i, c.size_j = 2, (Hi, Wi), (Hj, Wj)
    seed = 900 + 13 * Hi + Wj

    def surface(s, H, W):
        d = np.full((H, W), FAR)
        d[H // 4:H // 4 + max(2, H // 3), W // 5:W // 5 + max(2, W // 3)] = NEAR
        r = ints(s, d.shape, 40)
        d[r == 0], d[r == 1], d[r == 2] = 0.0, -1.0, np.nan
        return d
    c.depth_i = np.stack([surface(seed + b, Hi, Wi) for b in range(2)]).astype(np.float32)
    c.depth_j = np.stack([surface(seed + 5 + b, Hj, Wj) for b in range(2)]).astype(np.float32)
    c.K_i = np.stack([_kmat(32, Wi // 2, Hi // 2), _kmat(32, Wi // 2 + 1, Hi // 2 - 1)]).astype(np.float32)
    c.K_j = np.stack([_kmat(32, Wj // 2, Hj // 2), _kmat(32, Wj // 2 + 1, Hj // 2 - 1)]).astype(np.float32)
    c.T = np.stack([_pose(RZ[180], T_XY), _pose(RZ[0], (1 / 16, 1 / 16, 0.0))]).astype(np.float32)
    _DENSE[name] = c
    return c


# ------------------------------------------------------------------------------------------------ sampler cases
def sample_case(C):
    """two maps [C,9,11] of values k/64 with NaN holes, and points (x, y) wholly on the half-integer grid or wholly on odd quarters:
    the planted NaNs sit under a tap of weight zero (an on-grid point's neighbours: the sample is its own pixel), under a weighted
    tap with a good nearest pixel, with a NaN nearest pixel, and on the border"""
    H, W = 9, 11
    fm = (ints(1200 + C, (2, C, H, W), 257) - 128) / 64.0
    fm[ints(1300 + C, fm.shape, 12) == 0] = np.nan
    fm[:, :, 4, 5], fm[:, :, 4, 6], fm[:, :, 5, 5] = 0.75, np.nan, np.nan  # (5.5, 4.5) on the grid: NaN neighbours at weight zero
    fm[:, :, 2, 2], fm[:, :, 2, 3], fm[:, :, 3, 2], fm[:, :, 3, 3] = 1.5, np.nan, -0.25, 0.5  # (3.25, 3.25): NaN at weight 3/16, nearest (3, 3) good
    fm[:, :, 6, 8], fm[:, :, 6, 7] = np.nan, 0.25  # (8.75, 6.75): nearest pixel (6, 8) a NaN -> NaN
    fm[:, :, 0, 0] = np.nan  # (0.25, 0.25): three taps outside, the one inside a NaN
    pts = [(5.5, 4.5), (3.25, 3.25), (8.75, 6.75), (0.25, 0.25), (0.5, 0.5), (W - 0.5, H - 0.5), (W - 0.25, 3.25), (-1.5, 2.5), (4.5, H + 2.5),
           (np.nan, 2.5), (np.inf, 2.5), (1e10, -1e10)]
    k = 30
    on = np.stack([ints(1400 + C, (k,), W) + 0.5, ints(1401 + C, (k,), H) + 0.5], 1)
    off = np.stack([ints(1402 + C, (k,), W - 1) + 0.75 + 0.5 * ints(1403 + C, (k,), 2), ints(1404 + C, (k,), H - 1) + 0.75 + 0.5 * ints(1405 + C, (k,), 2)], 1)
    pts = np.concatenate([np.array(pts), on, off]).astype(np.float32)
    return fm.astype(np.float32), np.stack([pts, pts[::-1]])


# ------------------------------------------------------------------------------------------------ epipolar cases
EPI_SHAPES = ((1, 1), (3, 1025), (257, 260))
EPI_GATE = 2.0 ** -21  # relative; four roundings of 2^-24 (root, quotient, twice; one sum), doubled


def epipolar_case(n, m, cols=(2, 2)):
    """B = 2: F with entries k/4, |k| <= 4, points on the half-integer lattice below 16 (a third column: w in {0.5, 1, 2}): p1^T F p0
    and the squared norms are exact in fp32"""
    seed = 2000 + 7 * n + m
    E = (ints(seed, (2, 3, 3), 9) - 4) / 4.0
    pts = lambda s, k, c: np.concatenate([ints(s, (2, k, 2), 32) / 2.0] + ([0.5 * 2.0 ** ints(s + 1, (2, k, 1), 3)] if c == 3 else []), -1)  # noqa: E731
    return pts(seed + 1, n, cols[0]).astype(np.float32), pts(seed + 3, m, cols[1]).astype(np.float32), E.astype(np.float32)


def general_epipolar_case():
    """one pair in general position (non-dyadic pose and cameras): n = 70, m = 90 pixel keypoints and F = K1^-T [t]x R K0^-1"""
    a = 0.3
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, np.cos(0.1), -np.sin(0.1)],
                                                                                                  [0, np.sin(0.1), np.cos(0.1)]])
    t = np.array([0.31, -0.12, 0.07])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    K0, K1 = _kmat(223.7, 171.3, 129.1), _kmat(231.2, 168.9, 131.4)
    Fm = np.linalg.inv(K1).T @ tx @ R @ np.linalg.inv(K0)
    p0 = np.stack([ints(2500, (70,), 3460) / 10.0, ints(2501, (70,), 2600) / 10.0], 1)
    p1 = np.stack([ints(2502, (90,), 3460) / 10.0, ints(2503, (90,), 2600) / 10.0], 1)
    return p0.astype(np.float32)[None], p1.astype(np.float32)[None], Fm.astype(np.float32)[None]


# ------------------------------------------------------------------------------------------------ pose error cases
def pose_error_case():
    """a ground-truth pose and two estimates: rotations about the optical axis, translations in the image plane"""
    rot = lambda a: np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])  # noqa: E731
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(0.5), [0.6, 0.8, 0.0]
    return T.astype(np.float32), [(rot(0.25).astype(np.float32), np.array([0.8, 0.6, 0.0], np.float32)),
                                  (rot(0.5).astype(np.float32), np.array([-0.6, -0.8, 0.1], np.float32))]
