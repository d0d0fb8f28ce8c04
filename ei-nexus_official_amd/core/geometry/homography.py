"""Random homographies for homographic pairs: drop-in for the sampler and the point warps of the reference's
core/geometry/homography.py (flat2mat :10, sample_homography_corners :40-107, compute_homography :110-128, warp_points :134-158,
warp_points_torch :161-180), which the reference ships and never calls.  Host numpy float64, restated from what the functions
compute.  `sample_homography_corners` issues the SAME draws from `rng` in the SAME order as the reference (as Matchers.py does for
its random padding), so a seeded run picks the same homographies: one uniform (4, 2) block per try of the convexity loop, two
shuffles of the angle grid, one uniform pair for the translation.  The line utilities and the error functions of that file are
not restated: the package measures homography errors on the device (csrc/homography.hip, csrc/metrics.hip).

All coordinates are continuous image coordinates, (x, y) with the pixel (r, c) centred at (c + 0.5, r + 0.5): the convention of
`sparse_positions`, of gt_matches(..., homography=) and of datasets.warp.warp_perspective."""
import math

import numpy as np
import torch


def flat2mat(H):
    """[N,8] -> the 3x3 matrix whose ninth entry is 1 (N = 1)"""
    H = np.asarray(H)
    return np.concatenate([H, np.ones_like(H[:, :1])], axis=1).reshape(3, 3)


def _center_patch(shape, patch_shape=None):
    """corners (left-bottom, left-top, right-top, right-bottom) of a patch centred in `shape` = (width, height), cut to integers"""
    w, h = shape
    pw, ph = shape if patch_shape is None else patch_shape
    x0, x1 = int((w - pw) / 2), int((w + pw) / 2)
    y0, y1 = int((h - ph) / 2), int((h + ph) / 2)
    return np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]])


def _convex(quad, min_convexity):
    """every turn of the polygon [N,2] is clockwise by more than `min_convexity` (cross product of consecutive edges)"""
    n = quad.shape[0]
    for i in range(n):
        (xa, ya), (xb, yb), (xc, yc) = quad[(i - 1) % n], quad[i], quad[(i + 1) % n]
        if (xb - xa) * (yc - yb) - (xc - xb) * (yb - ya) > -min_convexity:
            return False
    return True


def sample_homography_corners(shape, patch_shape, difficulty=1.0, translation=0.4, n_angles=10, max_angle=90, min_convexity=0.05,
                              rng=np.random):
    """A random convex quadrilateral of the image `shape` = (width, height) and the homography that takes it to the centred patch
    `patch_shape`.  Returns (H [3,3] float64 with H[2,2] = 1, the image's corners [4,2], their images under H [4,2], patch_shape).
    difficulty in [0, 1] scales how far the corners move inwards, the rotation range and the translation; 0 gives the map from the
    whole image to the patch."""
    max_angle = max_angle / 180.0 * math.pi
    w, h = shape
    inner = _center_patch(shape, (w * (1 - difficulty), h * (1 - difficulty)))  # the quadrilateral's corners never leave [full, inner]
    full = _center_patch(shape)
    target = _center_patch(patch_shape)
    reach = inner - full
    size = np.array(shape)
    while True:  # one (4, 2) block of draws per try
        quad = full + rng.uniform(0.0, 1.0, size=(4, 2)) * reach
        if _convex(quad / size, min_convexity):
            break
    quad = quad - np.mean(quad, axis=0, keepdims=True)
    quad = quad + np.mean(inner, axis=0, keepdims=True)

    if n_angles > 0 and difficulty > 0:
        angles = np.linspace(-max_angle * difficulty, max_angle * difficulty, n_angles)
        rng.shuffle(angles)
        rng.shuffle(angles)
        angles = np.concatenate([[0.0], angles], axis=0)
        centre = np.mean(quad, axis=0, keepdims=True)
        c, s = np.cos(angles), np.sin(angles)
        rot = np.stack([c, -s, s, c], axis=1).reshape(-1, 2, 2)
        turned = np.matmul(np.tile((quad - centre)[None], [n_angles + 1, 1, 1]), rot) + centre
        for k in range(1, n_angles):  # the first shuffled angle that keeps every corner inside the image
            rel = turned[k] / size
            if np.all((rel >= 0.0) & (rel < 1.0)):
                quad = turned[k]
                break

    if translation > 0:
        lo = -np.min(quad, axis=0)
        hi = shape - np.max(quad, axis=0)
        quad += rng.uniform(lo, hi)[None] * translation * difficulty

    H = compute_homography(quad, target, [1.0, 1.0])
    return H, full, warp_points(full, H, inverse=False), patch_shape


def compute_homography(pts1_, pts2_, shape):
    """the homography [3,3] (ninth entry 1) that takes the four points pts1_ to pts2_, both [4,2] and scaled by shape[::-1]:
    the eight linear equations of the direct linear transform, solved exactly"""
    scale = np.array(shape[::-1], dtype=np.float32)[None]
    src, dst = pts1_ * scale, pts2_ * scale
    rows, rhs = [], []
    for (x, y), (u, v) in zip(src, dst):
        rows.append([x, y, 1, 0, 0, 0, -x * u, -y * u])
        rows.append([0, 0, 0, x, y, 1, -x * v, -y * v])
        rhs += [[u], [v]]
    return flat2mat(np.linalg.solve(np.stack(rows, axis=0), np.array(rhs)).T)


def warp_points(points, homography, inverse=True):
    """points [N,2] through the INVERSE of `homography` ([3,3] or [B,3,3]; inverse=False: through the homography itself) ->
    [N,2] or [B,N,2].  A third coordinate closer to 0 than 1e-8 is replaced by 1e-8."""
    H = homography[None] if homography.ndim == 2 else homography
    pts = np.concatenate([points, np.ones([points.shape[0], 1], dtype=np.float32)], -1)
    M = np.transpose(np.linalg.inv(H) if inverse else H)  # [3,3,B]: M[j,i,b] = H_b[i,j]
    out = np.transpose(np.tensordot(pts, M, axes=[[1], [0]]), [2, 0, 1])  # [B,N,3]
    out[np.abs(out[:, :, 2]) < 1e-8, 2] = 1e-8
    out = out[:, :, :2] / out[:, :, 2:]
    return out[0] if homography.ndim == 2 else out


def warp_points_torch(points, H, inverse=True):
    """points [B,N,2] through the INVERSE of H ([3,3] or [B,3,3]; inverse=False: through H) -> [B,N,2]; the third coordinate
    is offset by 1e-5 before the division"""
    pts = torch.cat([points, points.new_ones(points.shape[:-1] + (1,))], dim=-1)
    M = (torch.inverse(H) if inverse else H).transpose(-2, -1)
    out = torch.einsum("...nj,...ji->...ni", pts, M)
    return out[..., :-1] / (out[..., -1:] + 1e-5)


def sample_homographies(B, shape, patch_shape=None, *, rng, **kw):
    """B successive sample_homography_corners calls on ONE rng -> H [B,3,3] float64 (source -> destination).  shape = (width,
    height); patch_shape None: the image itself.  kw: difficulty, translation, n_angles, max_angle, min_convexity."""
    if int(B) < 0:
        raise ValueError(f"einx: sample_homographies: B must not be negative, got {B}")
    patch = tuple(shape) if patch_shape is None else patch_shape
    out = np.empty((int(B), 3, 3), np.float64)
    for b in range(int(B)):
        out[b] = sample_homography_corners(tuple(shape), patch, rng=rng, **kw)[0]
    return out
