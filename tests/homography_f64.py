"""Homography of ONE pair, written from the contract of DESIGN.md section 8c in float64 numpy (the answer csrc/homography.hip is
measured against).  Not collected by pytest (no test_ prefix).  The DLT takes its eigenvector from numpy.linalg.eigh and the
polish its steps from numpy.linalg.solve (cyclic Jacobi and Gauss-Jordan on the device), so that the two do not share a solver;
everything else (generator, checkSubset, inlier rule, selection scan, damping rule, corner rows) is the contract itself."""
import math

import numpy as np

from pose_f64 import DEFAULT_SEED, MASK64, splitmix64  # the generator of 8b

RETRIES = 64    # tries of one draw for an index not drawn before
ATTEMPTS = 16   # samples drawn for one iteration until one passes checkSubset
LM_ITERS = 10
FLT_EPS = float(np.finfo(np.float32).eps)
DBL_EPS = float(np.finfo(np.float64).eps)
TRIPLETS = ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3))
GT_BOUND = 3.0  # px: the smallest correctness threshold of the script; held by every pair with N >= 50, <= 50 % outliers, <= 0.5 px


def draw(seed, it, att, n):
    """four distinct indices of [0, n) for attempt `att` of RANSAC iteration `it`: draw d, retry r ->
    splitmix64(seed ^ (att << 32 | it << 16 | d << 8 | r)) % n; None when a draw finds no new index within RETRIES tries"""
    out = []
    for d in range(4):
        for r in range(RETRIES):
            v = splitmix64((seed ^ ((att << 32) | (it << 16) | (d << 8) | r)) & MASK64) % n
            if v not in out:
                out.append(v)
                break
        else:
            return None
    return out


def _collinear(a, b, c):
    """haveCollinearPoints' test of the triplet a < b < c, based at c"""
    d1x, d1y, d2x, d2y = b[0] - c[0], b[1] - c[1], a[0] - c[0], a[1] - c[1]
    return abs(d2x * d1y - d1x * d2y) <= FLT_EPS * (abs(d1x) + abs(d1y) + abs(d2x) + abs(d2y))


def _det3(p0, p1, p2):
    return p0[0] * (p1[1] - p2[1]) - p0[1] * (p1[0] - p2[0]) + (p1[0] * p2[1] - p2[0] * p1[1])


def check_subset(m1, m2):
    """four points [4,2] float64 of each image: no collinear triplet in either, and every triplet keeps its orientation (a
    sample whose four triplets all flip, a reflection, is rejected too: 8c)"""
    negative = 0
    for i, j, k in TRIPLETS:
        if _collinear(m1[i], m1[j], m1[k]) or _collinear(m2[i], m2[j], m2[k]):
            return False
        negative += _det3(m1[i], m1[j], m1[k]) * _det3(m2[i], m2[j], m2[k]) < 0.0
    return negative == 0


def dlt(m1, m2):
    """OpenCV's normalised DLT (HomographyEstimatorCallback::runKernel) over points [n,2] float64 -> H [3,3] with H[2,2] = 1, or
    None (a degenerate axis, a non-finite result, |H[2,2]| <= 1e-12 max|H|)"""
    n = len(m1)
    if n < 4:
        return None
    cM, cm = m1.sum(0) / n, m2.sum(0) / n
    dM, dm = np.abs(m1 - cM).sum(0), np.abs(m2 - cm).sum(0)
    if not (np.all(np.abs(dM) >= DBL_EPS) and np.all(np.abs(dm) >= DBL_EPS)):
        return None
    sM, sm = n / dM, n / dm
    X, Y = (m1[:, 0] - cM[0]) * sM[0], (m1[:, 1] - cM[1]) * sM[1]
    x, y = (m2[:, 0] - cm[0]) * sm[0], (m2[:, 1] - cm[1]) * sm[1]
    one, zero = np.ones(n), np.zeros(n)
    Lx = np.stack([X, Y, one, zero, zero, zero, -x * X, -x * Y, -x], 1)
    Ly = np.stack([zero, zero, zero, X, Y, one, -y * X, -y * Y, -y], 1)
    LtL = Lx.T @ Lx + Ly.T @ Ly
    w, V = np.linalg.eigh(LtL)
    H0 = V[:, 0].reshape(3, 3)
    inv_norm = np.array([[1.0 / sm[0], 0, cm[0]], [0, 1.0 / sm[1], cm[1]], [0, 0, 1.0]])
    norm2 = np.array([[sM[0], 0, -cM[0] * sM[0]], [0, sM[1], -cM[1] * sM[1]], [0, 0, 1.0]])
    with np.errstate(all="ignore"):
        H = inv_norm @ H0 @ norm2
        if not np.all(np.isfinite(H)) or not abs(H[2, 2]) > 1e-12 * np.abs(H).max():
            return None
        H = H * (1.0 / H[2, 2])
    H[2, 2] = 1.0
    return H if np.all(np.isfinite(H)) else None


def reproj_f32(H, m1, m2):
    """OpenCV's computeError: H rounded to float32, float32 arithmetic in its operation order; m1 / m2 [n,2] float32"""
    h = H.astype(np.float32).ravel()
    X, Y, x, y = m1[:, 0], m1[:, 1], m2[:, 0], m2[:, 1]
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        ww = one / ((h[6] * X + h[7] * Y) + one)
        dx = ((h[0] * X + h[1] * Y) + h[2]) * ww - x
        dy = ((h[3] * X + h[4] * Y) + h[5]) * ww - y
        return dx * dx + dy * dy


def update_iters(conf, ep, bound, model_points=4):
    """RANSACUpdateNumIters with (1 - ep)^m as m - 1 products and 8b's guards"""
    p = min(max(conf, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, 2.2250738585072014e-308)
    q = 1.0 - ep
    pw = q
    for _ in range(model_points - 1):
        pw = pw * q
    denom = 1.0 - pw
    if denom < 2.2250738585072014e-308:
        return 0
    num, denom = math.log(num), math.log(denom)
    return bound if denom >= 0 or -num >= bound * (-denom) else int(math.floor(num / denom + 0.5))


def _residuals(h, M, m, jac):
    """HomographyRefineCallback: residuals [2n] (and the Jacobian [2n,8]) of the 8 free entries h"""
    Mx, My = M[:, 0], M[:, 1]
    ww = (h[6] * Mx + h[7] * My) + 1.0
    with np.errstate(all="ignore"):
        ww = np.where(np.abs(ww) > DBL_EPS, 1.0 / ww, 0.0)
    xi = ((h[0] * Mx + h[1] * My) + h[2]) * ww
    yi = ((h[3] * Mx + h[4] * My) + h[5]) * ww
    r = np.stack([xi - m[:, 0], yi - m[:, 1]], 1).ravel()
    if not jac:
        return r, None
    z = np.zeros_like(Mx)
    J0 = np.stack([Mx * ww, My * ww, ww, z, z, z, -Mx * ww * xi, -My * ww * xi], 1)
    J1 = np.stack([z, z, z, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi], 1)
    J = np.empty((2 * len(Mx), 8))
    J[0::2], J[1::2] = J0, J1
    return r, J


def polish(H, M, m):
    """at most LM_ITERS Levenberg-Marquardt iterations over H's first 8 entries (8c's damping rule)"""
    h = H.ravel()[:8].copy()
    r, J = _residuals(h, M, m, True)
    A, v, S = J.T @ J, J.T @ r, float(r @ r)
    lam = 1e-3
    for _ in range(LM_ITERS):
        Ap = A + lam * np.diag(np.diag(A))
        try:
            with np.errstate(all="ignore"):
                d = np.linalg.solve(Ap, v)
        except np.linalg.LinAlgError:
            break
        if not np.all(np.isfinite(d)):
            break
        hd = h - d
        rd, Jd = _residuals(hd, M, m, True)
        Sd = float(rd @ rd)
        if Sd < S:
            h, S, A, v = hd, Sd, Jd.T @ Jd, Jd.T @ rd
            lam = lam / 10.0
        else:
            lam = lam * 10.0
        if np.abs(d).max() < FLT_EPS:
            break
    return np.append(h, 1.0).reshape(3, 3)


def corner_rows(H_true, H, img_shape, he_thr=(3, 5, 10)):
    """update_one's epilogue (matching_metrics.py:265-297) in float32, the 4x3 by 3x3 products as explicit sums left to right
    -> ([error <= t ...], mean corner distance as float32)"""
    f = np.float32
    Hh, Ww = img_shape
    corners = [(f(0), f(0)), (f(Ww - 1), f(0)), (f(0), f(Hh - 1)), (f(Ww - 1), f(Hh - 1))]
    total = f(0)
    with np.errstate(all="ignore"):
        for cx, cy in corners:
            pts = []
            for mat in (np.asarray(H_true).astype(f), np.asarray(H).astype(f)):
                u = (cx * mat[0, 0] + cy * mat[0, 1]) + mat[0, 2]
                v = (cx * mat[1, 0] + cy * mat[1, 1]) + mat[1, 2]
                z = (cx * mat[2, 0] + cy * mat[2, 1]) + mat[2, 2]
                pts.append((u / z, v / z))
            dx, dy = pts[0][0] - pts[1][0], pts[0][1] - pts[1][1]
            total = total + np.sqrt(dx * dx + dy * dy)
        mean = f(total / f(4))
    return [float(mean <= f(t)) for t in he_thr], mean


def homography(kp0, kp1, thresh=3.0, conf=0.995, ordering="yx", max_iters=2000, seed=DEFAULT_SEED, stages=False):
    """kp0 / kp1 [N, 2|3] float32 -> dict(status = "ok" | "few" | "noH", it, H [3,3] float64, mask [N] bool).  With stages=True
    also the RANSAC model (H_ransac) and the refit (H_refit) before the polish."""
    kp0, kp1 = np.asarray(kp0, np.float32)[:, :2], np.asarray(kp1, np.float32)[:, :2]
    if ordering == "yx":
        kp0, kp1 = kp0[:, ::-1], kp1[:, ::-1]
    kp0, kp1 = np.ascontiguousarray(kp0), np.ascontiguousarray(kp1)
    n = len(kp0)
    M, m = kp0.astype(np.float64), kp1.astype(np.float64)
    if n < 4:
        return {"status": "few"}
    if n == 4:
        H = dlt(M, m)
        if H is None:
            return {"status": "noH"}
        return {"status": "ok", "it": 0, "H": H, "mask": np.ones(4, bool)}
    thr2 = np.float32(thresh * thresh)
    best, best_cnt, best_H, best_mask, bound = -1, 0, None, None, max_iters
    it = 0
    while it < bound:
        H = None
        for att in range(ATTEMPTS):
            idx = draw(seed, it, att, n)
            if idx is not None and check_subset(M[idx], m[idx]):
                H = dlt(M[idx], m[idx])
                break
        if H is not None:
            mask = reproj_f32(H, kp0, kp1) <= thr2
            c = int(mask.sum())
            if c > max(best_cnt, 3):
                best, best_cnt, best_H, best_mask = it, c, H, mask
                bound = update_iters(conf, (n - c) / n, bound)
        it += 1
    if best < 0:
        return {"status": "noH"}
    H1 = dlt(M[best_mask], m[best_mask])
    if H1 is None:
        return {"status": "noH"}
    H2 = polish(H1, M[best_mask], m[best_mask])
    out = {"status": "ok", "it": best, "H": H2, "mask": best_mask}
    if stages:
        out.update(H_ransac=best_H, H_refit=H1)
    return out


def rows(res, H_true, img_shape, he_thr=(3, 5, 10)):
    """the device's per-pair row: ratios, error, inlier ratio (0.., inf, 0 without a homography)"""
    if res["status"] != "ok":
        return [0.0] * len(he_thr) + [np.inf, 0.0]
    ratios, err = corner_rows(H_true, res["H"], img_shape, he_thr)
    return ratios + [float(err), float(res["mask"].mean())]


# ------------------------------------------------------------------ synthetic scenes
def random_homography(rng, W=346, H=260, shift=40.0):
    """the homography that moves the four frame corners by up to +-shift px each (exact 4-point DLT in float64)"""
    src = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.float64)
    dst = src + rng.uniform(-shift, shift, (4, 2))
    A, b = [], []
    for (X, Y), (x, y) in zip(src, dst):
        A.append([X, Y, 1, 0, 0, 0, -x * X, -x * Y])
        A.append([0, 0, 0, X, Y, 1, -y * X, -y * Y])
        b += [x, y]
    h = np.linalg.solve(np.array(A), np.array(b))
    return np.append(h, 1.0).reshape(3, 3)


def warp(Hm, pts):
    q = np.c_[pts, np.ones(len(pts))] @ Hm.T
    return q[:, :2] / q[:, 2:]


def scene(rng, n, noise=0.0, outliers=0.0, W=346, H=260, shift=40.0, cols=3, ordering="yx"):
    """n uniformly placed points of a W x H frame and their images under a random homography, noise px of Gaussian noise on both
    sides, a fraction of uniformly re-drawn outliers; float32 storage in `ordering` with a score column when cols == 3.
    -> (kp0, kp1, H_true [3,3] float64)"""
    Ht = random_homography(rng, W, H, shift)
    p0 = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], 1)
    p1 = warp(Ht, p0)
    if noise:
        p0 = p0 + rng.normal(scale=noise, size=p0.shape)
        p1 = p1 + rng.normal(scale=noise, size=p1.shape)
    n_out = int(round(outliers * n))
    if n_out:
        sel = rng.choice(n, n_out, replace=False)
        p1[sel] = np.stack([rng.uniform(0, W - 1, n_out), rng.uniform(0, H - 1, n_out)], 1)
    if ordering == "yx":
        p0, p1 = p0[:, ::-1], p1[:, ::-1]
    if cols == 3:
        score = rng.uniform(0, 1, (n, 1))
        p0, p1 = np.hstack([p0, score]), np.hstack([p1, score])
    return p0.astype(np.float32), p1.astype(np.float32), Ht


IMG_SHAPE = (260, 346)  # (H, W) of the scenes
# (N, noise px, outlier fraction) of the generated pairs of `batch()`
BATCH_SPEC = [(4, 0.0, 0.0), (5, 0.0, 0.0), (8, 0.0, 0.0), (8, 0.3, 0.25), (50, 0.0, 0.0), (50, 0.5, 0.2), (50, 0.5, 0.5), (50, 1.0, 0.3),
              (300, 0.0, 0.0), (300, 0.5, 0.3), (300, 0.5, 0.6), (300, 1.0, 0.5), (1024, 0.0, 0.0), (1024, 0.5, 0.3), (1024, 1.0, 0.6),
              (1024, 0.2, 0.1)]
BATCH_GT = [b for b, (n, nz, o) in enumerate(BATCH_SPEC) if n >= 50 and nz <= 0.5 and o <= 0.5]  # pairs held to GT_BOUND
BATCH_FAIL = {16: "noH", 17: "noH", 18: "few", 19: "few", 20: "noH"}


def batch():
    """the ragged batch of the kernel tests, (kp0, kp1, H_true) per pair in (y, x, score) float32: BATCH_SPEC's scenes, then
    16: every point identical, 17: collinear points, 18: N = 3, 19: N = 0, 20: a mirrored pair (every sample fails the
    orientation test)"""
    rng = np.random.default_rng(2025)
    pairs = [scene(rng, n, noise=nz, outliers=o) for n, nz, o in BATCH_SPEC]
    k0, k1, Ht = scene(rng, 40)
    same = np.repeat(k0[:1], 40, 0)
    pairs.append((same, same.copy(), Ht))
    line = np.stack([20.0 + 6 * np.arange(30), 30.0 + 4 * np.arange(30), np.ones(30)], 1).astype(np.float32)  # exact in float32
    pairs.append((line, line[::-1].copy(), Ht))
    pairs.append((k0[:3], k1[:3], Ht))
    pairs.append((k0[:0], k1[:0], Ht))
    mirrored = k1.copy()
    mirrored[:, 1] = np.float32(345.0) - mirrored[:, 1]  # x -> W - 1 - x in the second image
    pairs.append((k0, mirrored, Ht))
    return pairs
