"""Absolute pose of ONE pair from matches and the depth of view 0, written from the contract of DESIGN.md section 8u in float64
numpy (the answer csrc/abs_pose.hip is measured against).  Not collected by pytest (no test_ prefix).  Where a second route
exists it is taken, so that the two do not share a mistake: numpy.roots for Grunert's quartic (the kernel brackets between the
derivative's roots), a Kabsch/SVD alignment for the pose of a root (the kernel builds two orthonormal frames; `frames_pose` here
restates that and `p3p` cross-checks the two), numpy.linalg.solve for the damped normal equations (the kernel eliminates).  The
generator, the lift, the inlier rule, the selection scan and the damping rule are the contract itself."""
import math

import numpy as np

from pose_f64 import DEFAULT_SEED, MASK64, rotation, splitmix64

FLT_EPS = 1.1920928955078125e-07
COLLINEAR_TOL = 1e-6   # |(P2 - P1) x (P3 - P1)| <= tol |P2 - P1| |P3 - P1|: no model
BEARING_TOL = 1e-6     # |f_i x f_j| <= tol for a pair of unit bearings: no model
LEAD_TOL = 1e-12       # a leading coefficient of the quartic at or below this fraction of the largest one lowers the degree
LM_ITERS = 10


# ------------------------------------------------------------------ draws and the scan's bound
def draw3(seed, it, n, retries=64):
    """three distinct indices of [0, n) for iteration `it`: draw d, retry r -> splitmix64(seed ^ (it << 16 | d << 8 | r)) % n"""
    out = []
    for d in range(3):
        for r in range(retries):
            v = splitmix64((seed ^ ((it << 16) | (d << 8) | r)) & MASK64) % n
            if v not in out:
                out.append(v)
                break
        else:
            return None
    return out


def update_iters(conf, ep, bound):
    """RANSACUpdateNumIters with (1 - ep)^3 as two products"""
    p = min(max(conf, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, 2.2250738585072014e-308)
    q = 1.0 - ep
    denom = 1.0 - q * q * q
    if denom < 2.2250738585072014e-308:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= bound * (-denom):
        return bound
    return int(math.floor(num / denom + 0.5))


# ------------------------------------------------------------------ the lift
def sample_depth(dm, x, y):
    """csrc/gt_project.h:gt_sample_depth in float32: bilinear with zero padding at x - 0.5; a hole (<= 0 or NaN) under a tap of
    non-zero weight sends the sample to the nearest pixel (half to even), NaN when that is a hole, 0 outside the map"""
    f = np.float32
    H, W = dm.shape
    x, y = f(x), f(y)
    ix, iy = f(x - f(0.5)), f(y - f(0.5))
    fx0, fy0 = f(np.floor(ix)), f(np.floor(iy))
    tx, ty = f(ix - fx0), f(iy - fy0)
    x0 = int(fx0) if -2.0 <= fx0 <= W else -2
    y0 = int(fy0) if -2.0 <= fy0 <= H else -2
    wx = (f(f(fx0 + f(1)) - ix), tx)
    wy = (f(f(fy0 + f(1)) - iy), ty)
    acc, hole = f(0), False
    for dy in range(2):
        for dx in range(2):
            xx, yy = x0 + dx, y0 + dy
            if xx < 0 or xx >= W or yy < 0 or yy >= H:
                continue
            w = f(wx[dx] * wy[dy])
            v = f(dm[yy, xx])
            if not v > 0:
                if w != 0:
                    hole = True
                continue
            acc = f(acc + f(v * w))
    if not hole and ix == ix and iy == iy:
        return acc
    nx, ny = f(np.rint(ix)), f(np.rint(iy))
    if not (0 <= nx < W and 0 <= ny < H):
        return f(0)
    v = f(dm[int(ny), int(nx)])
    return v if v > 0 else f(np.nan)


def lift(kp0, K0, depth0=None, d0=None, valid0=None):
    """-> (usable indices in order, X [nu,3] float64): X = d ((x - cx) / fx, (y - cy) / fy, 1), kp0 [n,2] (x, y) float32"""
    n = len(kp0)
    if depth0 is not None:
        d = np.array([sample_depth(depth0, kp0[j, 0], kp0[j, 1]) for j in range(n)], np.float32).reshape(n)
        valid = (d == d) & (d > 0)
    else:
        d, valid = np.asarray(d0, np.float32)[:n], np.asarray(valid0)[:n] != 0
    idx = np.nonzero(valid)[0]
    K = np.asarray(K0, np.float32).astype(np.float64)
    x, y, dd = kp0[idx, 0].astype(np.float64), kp0[idx, 1].astype(np.float64), d[idx].astype(np.float64)
    X = np.stack([dd * ((x - K[0, 2]) / K[0, 0]), dd * ((y - K[1, 2]) / K[1, 1]), dd], 1)
    return idx, X


def bearings(px, K1):
    """unit bearings of pixels [n,2] (x, y) float64 under K1"""
    K = np.asarray(K1, np.float32).astype(np.float64)
    v = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0], (px[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(px))], 1)
    return v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + 1.0)[:, None]


# ------------------------------------------------------------------ P3P (Grunert)
def grunert_quartic(P, f):
    """(coefficients A0..A4 ascending in v = s3 / s1, the terms u(v) needs) or None under the guards"""
    d21, d31 = P[1] - P[0], P[2] - P[0]
    cr = np.cross(d21, d31)
    if not np.dot(cr, cr) > COLLINEAR_TOL ** 2 * np.dot(d21, d21) * np.dot(d31, d31):
        return None
    for i, j in ((0, 1), (0, 2), (1, 2)):
        c = np.cross(f[i], f[j])
        if not np.dot(c, c) > BEARING_TOL ** 2:
            return None
    a2, b2, c2 = np.dot(P[1] - P[2], P[1] - P[2]), np.dot(d31, d31), np.dot(d21, d21)
    ca, cb, cg = np.dot(f[1], f[2]), np.dot(f[0], f[2]), np.dot(f[0], f[1])
    q = (a2 - c2) / b2     # (a^2 - c^2) / b^2
    p = (a2 + c2) / b2
    A4 = (q - 1.0) ** 2 - 4.0 * c2 / b2 * ca * ca
    A3 = 4.0 * (q * (1.0 - q) * cb - (1.0 - p) * ca * cg + 2.0 * c2 / b2 * ca * ca * cb)
    A2 = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb * cb + 2.0 * (b2 - c2) / b2 * ca * ca - 4.0 * p * ca * cb * cg + 2.0 * (b2 - a2) / b2 * cg * cg)
    A1 = 4.0 * (-q * (1.0 + q) * cb + 2.0 * a2 / b2 * cg * cg * cb - (1.0 - p) * ca * cg)
    A0 = (1.0 + q) ** 2 - 4.0 * a2 / b2 * cg * cg
    return np.array([A0, A1, A2, A3, A4]), (q, ca, cb, cg, b2)


def frames_pose(P, Q):
    """the kernel's closed form: R = F_Q F_P^T from the orthonormal frames of the two triples, t = Q1 - R P1"""
    def frame(T):
        e1 = T[1] - T[0]
        e1 = e1 / np.linalg.norm(e1)
        e3 = np.cross(e1, T[2] - T[0])
        e3 = e3 / np.linalg.norm(e3)
        return np.stack([e1, np.cross(e3, e1), e3], 1)
    R = frame(Q) @ frame(P).T
    return R, Q[0] - R @ P[0]


def kabsch_pose(P, Q):
    """least-squares rigid alignment Q ~ R P + t by SVD (exact for congruent triangles)"""
    cp, cq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - cq).T @ (P - cp))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, cq - R @ cp


def p3p(P, f, check=True):
    """every pose (R, t) with s_i f_i = R P_i + t, s_i > 0, ordered by ascending v = s3 / s1: P [3,3] points, f [3,3] unit bearings"""
    g = grunert_quartic(P, f)
    if g is None:
        return []
    A, (q, ca, cb, cg, b2) = g
    n, amax = 4, np.abs(A).max()
    while n > 0 and not abs(A[n]) > LEAD_TOL * amax:
        n -= 1
    if n == 0 or not np.all(np.isfinite(A)):
        return []
    vs = []
    for r in np.roots(A[n::-1]):
        if abs(r.imag) > 1e-8 * max(1.0, abs(r.real)):
            continue
        v = r.real
        for _ in range(3):  # Newton on the quartic
            pv = (((A[4] * v + A[3]) * v + A[2]) * v + A[1]) * v + A[0]
            dv = ((4.0 * A[4] * v + 3.0 * A[3]) * v + 2.0 * A[2]) * v + A[1]
            step = pv / dv
            if not np.isfinite(step):
                break
            v = v - step
        vs.append(v)
    vs.sort()
    out, last = [], None
    for v in vs:
        if last is not None and abs(v - last) <= 1e-9 * max(1.0, abs(v)):
            continue  # a double root shows up twice: the kernel finds distinct roots
        last = v
        with np.errstate(all="ignore"):
            u = ((q - 1.0) * v * v - 2.0 * q * cb * v + 1.0 + q) / (2.0 * (cg - v * ca))
            s1 = np.sqrt(b2 / (1.0 + v * v - 2.0 * v * cb))
        s = np.array([s1, u * s1, v * s1])
        if not (np.all(np.isfinite(s)) and np.all(s > 0)):
            continue
        Q = s[:, None] * f
        R, t = kabsch_pose(P, Q)
        if check:
            R2, t2 = frames_pose(P, Q)
            assert np.abs(R - R2).max() < 1e-6 and np.abs(t - t2).max() < 1e-6 * max(1.0, np.abs(t).max()), "frames and Kabsch disagree"
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
            out.append((R, t))
    return out


# ------------------------------------------------------------------ score, RANSAC, refit
def project(R, t, X, K1):
    Y = X @ R.T + t
    with np.errstate(all="ignore"):
        u = K1[0, 0] * (Y[:, 0] / Y[:, 2]) + K1[0, 2]
        v = K1[1, 1] * (Y[:, 1] / Y[:, 2]) + K1[1, 2]
    return Y, u, v


def inliers(R, t, X, px, K1, thresh):
    Y, u, v = project(R, t, X, K1)
    with np.errstate(invalid="ignore"):
        e = (u - px[:, 0]) * (u - px[:, 0]) + (v - px[:, 1]) * (v - px[:, 1])
        return (Y[:, 2] > 0) & (e <= thresh * thresh)


def ransac(X, px, K1, thresh, conf, max_iters, seed):
    """-> ((iteration, solution, R, t) or None, inlier mask over the usable list)"""
    n = len(X)
    f = bearings(px, K1)
    best, best_cnt, bound = None, 0, max_iters
    for it in range(max_iters):
        if it >= bound:
            break
        idx = draw3(seed, it, n)
        if idx is None:
            continue
        for k, (R, t) in enumerate(p3p(X[idx], f[idx])):
            cnt = int(np.count_nonzero(inliers(R, t, X, px, K1, thresh)))
            if cnt > max(best_cnt, 2):
                best, best_cnt = (it, k, R, t), cnt
                bound = update_iters(conf, (n - cnt) / n, bound)
    if best is None:
        return None, np.zeros(n, bool)
    return best, inliers(best[2], best[3], X, px, K1, thresh)


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def expm_so3(w):
    """exp([w]x) = I + A [w]x + B [w]x^2, A = sin(th) / th, B = 2 (sin(th / 2) / th)^2; A = 1, B = 1/2 at th = 0"""
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    A, B = 1.0, 0.5
    if th > 0:
        A = math.sin(th) / th
        h = math.sin(0.5 * th) / th
        B = 2.0 * h * h
    W = skew(w)
    return np.eye(3) + A * W + B * (W @ W)


def _normal(R, t, X, px, K1, reverse=False):
    """J^T J, J^T r and |r|^2 of the pixel residuals over the points; |r|^2 = inf when a point has Y_z <= 0"""
    Y, u, v = project(R, t, X, K1)
    if not np.all(Y[:, 2] > 0):
        return None, None, np.inf
    a = Y - t
    iz = 1.0 / Y[:, 2]
    n = len(X)
    J = np.zeros((n, 2, 6))
    for r, fk, num in ((0, K1[0, 0], Y[:, 0]), (1, K1[1, 1], Y[:, 1])):
        g = np.zeros((n, 3))          # d(pixel) / dY
        g[:, r] = fk * iz
        g[:, 2] = -fk * num * iz * iz
        J[:, r, :3] = np.cross(a, g)   # g . (w x a) = w . (a x g)
        J[:, r, 3:] = g
    res = np.stack([u - px[:, 0], v - px[:, 1]], 1)
    if reverse:
        J, res = J[::-1], res[::-1]
    Jf, rf = J.reshape(-1, 6), res.reshape(-1)
    return Jf.T @ Jf, Jf.T @ rf, float(np.sum(rf * rf))


def refit(R, t, X, px, K1, reverse=False):
    """at most LM_ITERS Levenberg-Marquardt iterations over (w, dt): R <- exp([w]x) R, t <- t + dt, 8c's damping rule"""
    A, g, S = _normal(R, t, X, px, K1, reverse)
    lam = 1e-3
    for _ in range(LM_ITERS):
        M = A + lam * np.diag(np.diag(A))
        try:
            d = np.linalg.solve(M, g)
        except np.linalg.LinAlgError:
            break
        if not np.all(np.isfinite(d)):
            break
        Rn, tn = expm_so3(-d[:3]) @ R, t - d[3:]
        An, gn, Sn = _normal(Rn, tn, X, px, K1, reverse)
        if Sn < S:
            R, t, A, g, S = Rn, tn, An, gn, Sn
            lam /= 10.0
        else:
            lam *= 10.0
        if np.abs(d).max() < FLT_EPS:
            break
    return R, t


def pose_rows(T_0to1, R, t):
    """(R_err degrees, |t - t_gt|, angle of t against t_gt in degrees folded to [0, 90]; NaN for a zero t_gt)"""
    T = np.asarray(T_0to1, np.float64)
    tg = T[:3, 3]
    cos = np.clip((np.trace(R.T @ T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    R_err = float(np.rad2deg(abs(math.acos(cos))))
    with np.errstate(all="ignore"):
        c = np.dot(t, tg) / (np.linalg.norm(t) * np.linalg.norm(tg))
        ang = np.rad2deg(np.arccos(np.clip(c, -1.0, 1.0)))
    ang = float(np.minimum(ang, 180.0 - ang))
    return R_err, float(np.linalg.norm(t - tg)), ang


def absolute_pose(kp0, kp1, K0, K1, depth0=None, d0=None, valid0=None, T_0to1=None, thresh=8.0, conf=0.99, ordering="yx",
                  max_iters=100, seed=DEFAULT_SEED, refine=True, reverse=False):
    """one pair end to end: kp [n, 2|3] float32, K [3,3] -> dict(status, R, t, mask [n], it = (iteration, solution), rows [5],
    R0 / t0 the RANSAC model); status 'ok', 'few' (fewer than 4 usable matches), 'none' (no model)"""
    kp0, kp1 = np.asarray(kp0, np.float32)[:, :2], np.asarray(kp1, np.float32)[:, :2]
    n = len(kp0)
    if ordering == "yx":
        kp0, kp1 = kp0[:, ::-1], kp1[:, ::-1]
    K1d = np.asarray(K1, np.float32).astype(np.float64)
    idx, X = lift(kp0, K0, depth0, d0, valid0)
    nu = len(idx)
    px = kp1[idx].astype(np.float64)
    usable = nu / n if n else float("nan")
    out = {"mask": np.zeros(n, bool), "nu": nu, "rows": [np.inf, np.inf, np.inf, 0.0, usable]}
    if nu < 4:
        return dict(out, status="few")
    best, inl = ransac(X, px, K1d, thresh, conf, max_iters, seed)
    if best is None:
        return dict(out, status="none")
    it, k, R0, t0 = best
    R, t = (refit(R0, t0, X[inl], px[inl], K1d, reverse) if refine else (R0, t0))
    out["mask"][idx[inl]] = True
    errs = list(pose_rows(T_0to1, R, t)) if T_0to1 is not None else [np.nan] * 3
    return dict(out, status="ok", R=R, t=t, R0=R0, t0=t0, it=(it, k), rows=errs + [int(inl.sum()) / nu, usable])


# ------------------------------------------------------------------ synthetic scenes
def scene(rng, n, noise=0.0, outliers=0.0, W=346, H=260, holes=None, max_deg=15.0):
    """ransac_cases.scene2 for the absolute pose: two different cameras over a W x H image (f ~ 0.65 W and ~ 0.9 W; view 0's depth
    map has the image's size), depth 2-10, float32 keypoints (y, x, score).  holes None: exact per-match depths d0 (float32) and valid0 of ones;
    a fraction: a depth map [H,W] float32 of a fronto-parallel-free smooth surface with that share of -1 holes, the keypoints'
    3-D points lying on it.  -> dict(kp0, kp1, K0, K1, T, depth0 | d0 + valid0)"""
    def intrinsics(f, dcx, dcy):
        f = f * W
        return np.array([[f * rng.uniform(1.01, 1.03), 0, W * (0.5 + dcx) + rng.uniform(-0.5, 0.5)],
                         [0, f * rng.uniform(0.97, 0.99), H * (0.5 + dcy) + rng.uniform(-0.5, 0.5)], [0, 0, 1]], np.float64).astype(np.float32)

    K0, K1 = intrinsics(0.65, -0.02, 0.02), intrinsics(0.9, 0.025, -0.025)
    R = rotation(rng.normal(size=3), rng.uniform(1.0, max_deg))
    t = rng.normal(size=3)
    t = t / np.linalg.norm(t) * rng.uniform(0.3, 1.0)
    K0d, K1d = K0.astype(np.float64), K1.astype(np.float64)
    dm = None
    if holes is not None:
        yy, xx = np.mgrid[0:H, 0:W]
        dm = (6.0 + 2.5 * np.sin(xx / 9.0 + rng.uniform(0, 3)) + 1.5 * np.cos(yy / 7.0 + rng.uniform(0, 3))).astype(np.float32)
        dm[rng.uniform(size=dm.shape) < holes] = -1.0
    pts0, pts1, ds = [], [], []
    while len(pts0) < n:
        u, v = float(np.float32(rng.uniform(1, W - 1))), float(np.float32(rng.uniform(1, H - 1)))
        if dm is None:
            z = float(np.float32(rng.uniform(2, 10)))
        else:
            z = float(sample_depth(dm, np.float32(u), np.float32(v)))
            if not z > 0:
                z = 5.0  # a hole: the match is not usable, any point will do
        X1 = R @ (np.linalg.solve(K0d, np.array([u, v, 1.0])) * z) + t
        if X1[2] <= 0.5:
            continue
        p = K1d @ (X1 / X1[2])
        if not (0 <= p[0] < W and 0 <= p[1] < H):
            continue
        pts0.append([u, v])
        pts1.append(p[:2])
        ds.append(z)
    pts0, pts1 = np.array(pts0).reshape(n, 2), np.array(pts1).reshape(n, 2)
    if noise:
        pts1 = pts1 + rng.normal(scale=noise, size=pts1.shape)  # view 0's keypoints stay where their depth was taken
    n_out = int(round(outliers * n))
    if n_out:
        sel = rng.choice(n, n_out, replace=False)
        pts1[sel] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)], 1)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    score = rng.uniform(0, 1, (n, 1))
    out = {"kp0": np.hstack([pts0[:, ::-1], score]).astype(np.float32), "kp1": np.hstack([pts1[:, ::-1], score]).astype(np.float32),
           "K0": K0, "K1": K1, "T": T}
    if dm is None:
        out["d0"], out["valid0"] = np.array(ds, np.float32), np.ones(n, np.uint8)
    else:
        out["depth0"] = dm
    return out
