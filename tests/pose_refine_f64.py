"""Refinement of ONE pair's relative pose on its Sampson inliers, written from the contract of DESIGN.md section 8w in float64 numpy
(the answer csrc/pose.hip's pose_refine_kernel is measured against).  Not collected by pytest (no test_ prefix).  The points, the
threshold, the inlier rule, the cheirality rule and the error rows are 8b's and come from tests/pose_f64.py; the sums run over
the set in index order, or in reverse with reverse=True (the kernel's order is a third one: the difference is REFINE_FLOOR)."""
import math

import numpy as np

import pose_f64 as P

FLT_EPS = 1.1920928955078125e-07
MIN_SET = 6  # a round needs at least this many Sampson inliers: five parameters and one to spare


def essential(R, t):
    return P.skew(t) @ R


def rot_step(w, R):
    """exp([w]x) R with exp = I + A [w]x + B [w]x^2, A = sin(th) / th, B = 2 (sin(th / 2) / th)^2; A = 1, B = 1/2 at th = 0"""
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    A, B = 1.0, 0.5
    if th > 0:
        A = math.sin(th) / th
        h = math.sin(0.5 * th) / th
        B = 2.0 * h * h
    W = P.skew(w)
    return (np.eye(3) + A * W + B * (W @ W)) @ R


def basis(t):
    """the tangent plane of the unit sphere at t: k = the smallest |t_i| (the first on ties), b1 = e_k x t normalised, b2 = t x b1"""
    k = 0
    for i in (1, 2):
        if abs(t[i]) < abs(t[k]):
            k = i
    e = np.zeros(3)
    e[k] = 1.0
    b1 = np.cross(e, t)
    b1 = b1 / math.sqrt(float(b1 @ b1))
    return b1, np.cross(t, b1)


def apply_step(R, t, d):
    """R <- exp([w]x) R with w = d[:3]; t <- (t + d[3] b1 + d[4] b2) normalised, the basis taken at t"""
    b1, b2 = basis(t)
    tn = t + d[3] * b1 + d[4] * b2
    return rot_step(d[:3], R), tn / math.sqrt(float(tn @ tn))


def directions(R, t):
    """the five directions of E = [t]x R: [t]x [e_k]x R for the rotation, [b1]x R and [b2]x R for the translation"""
    b1, b2 = basis(t)
    St = P.skew(t)
    return [St @ P.skew(e) @ R for e in np.eye(3)] + [P.skew(b1) @ R, P.skew(b2) @ R]


def _forms(E, x1, x2):
    """per match: (a, b) of E x1, (p, q) of E^T x2 and d = x2^T E x1"""
    h1 = np.column_stack([x1, np.ones(len(x1))])
    h2 = np.column_stack([x2, np.ones(len(x2))])
    l = h1 @ E.T
    m = h2 @ E
    return l[:, 0], l[:, 1], m[:, 0], m[:, 1], np.sum(h2 * l, 1)


def residuals(R, t, x1, x2):
    """r = d / sqrt(s), s = a^2 + b^2 + p^2 + q^2: the signed Sampson distance, unrounded"""
    a, b, p, q, d = _forms(essential(R, t), x1, x2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return d / np.sqrt(a * a + b * b + p * p + q * q)


def jacobian(R, t, x1, x2):
    """(r [m], J [m,5]) analytic: dr = dd / sqrt(s) - d ds / (2 s^(3/2)) per direction"""
    a, b, p, q, d = _forms(essential(R, t), x1, x2)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = a * a + b * b + p * p + q * q
        rs = np.sqrt(s)
        J = np.empty((len(x1), 5))
        for k, G in enumerate(directions(R, t)):
            da, db, dp, dq, dd = _forms(G, x1, x2)
            ds = 2.0 * (a * da + b * db + p * dp + q * dq)
            J[:, k] = dd / rs - d * ds / (2.0 * s * rs)
        return d / rs, J


def normal(R, t, x1, x2, reverse=False):
    """J^T J, J^T r and |r|^2 over the given matches"""
    r, J = jacobian(R, t, x1, x2)
    if reverse:
        r, J = r[::-1], J[::-1]
    A, g, S = np.zeros((5, 5)), np.zeros(5), 0.0
    for j in range(len(r)):  # a plain running sum: one order, not numpy's pairwise one
        A += np.outer(J[j], J[j])
        g += J[j] * r[j]
        S += r[j] * r[j]
    return A, g, float(S)


def gauss_jordan(M):
    """ransac.h's elimination with partial pivoting on the 5 x 6 system, tolerance 0: the solution column, or None"""
    M = M.copy()
    n = M.shape[0]
    for c in range(n):
        p = c
        for r in range(c + 1, n):
            if abs(M[r, c]) > abs(M[p, c]):
                p = r
        if not abs(M[p, c]) > 0.0:
            return None
        M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, n]


def sampson_inliers(R, t, x1, x2, thr2, trace=None, tag=None):
    e32, e64 = P.sampson_f32(essential(R, t), x1, x2)
    if trace is not None:
        trace.append(("sampson", tag, e64, float(thr2)))
    return e32 <= thr2  # a NaN is never an inlier


def cheirality(R, t, x1, x2):
    """(pose_f64.triangulate_ok's verdict, the three quantities it takes signs of: X_2 X_3, the depth in view 0, the depth in view 1)"""
    ok = P.triangulate_ok(R, t, x1, x2)
    P1 = np.hstack([R, t[:, None]])
    q = np.empty((len(x1), 3))
    for i in range(len(x1)):
        A = np.stack([[-1.0, 0.0, x1[i, 0], 0.0], [0.0, -1.0, x1[i, 1], 0.0], x2[i, 0] * P1[2] - P1[0], x2[i, 1] * P1[2] - P1[1]])
        X = np.linalg.svd(A)[2][3]
        with np.errstate(invalid="ignore", divide="ignore"):
            q[i] = X[2] * X[3], X[2] / X[3], P1[2] @ (X / X[3])
    return ok, q


def lm(R, t, x1, x2, lm_iters, reverse=False):
    """Levenberg-Marquardt on the matches given, 8c's damping rule.  -> (R, t, steps accepted, cost at the start, cost at the end)"""
    A, g, S = normal(R, t, x1, x2, reverse)
    S0, lam, acc = S, 1e-3, 0
    for _ in range(lm_iters):
        d = gauss_jordan(np.column_stack([A + lam * np.diag(np.diag(A)), g]))
        if d is None:
            break
        d = -d
        if not np.all(np.isfinite(d)):
            break
        Rn, tn = apply_step(R, t, d)
        An, gn, Sn = normal(Rn, tn, x1, x2, reverse)
        if Sn < S:  # a non-finite trial cost is a rejection
            R, t, A, g, S = Rn, tn, An, gn, Sn
            lam /= 10.0
            acc += 1
        else:
            lam *= 10.0
        if np.abs(d).max() < FLT_EPS:
            break
    return R, t, acc, S0, S


def rows_of(T_0to1, R, t, mask, n):
    """8b's four values: R_err, t_err, pose_err (NaN without a true pose), the mask count over n"""
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.float64(np.count_nonzero(mask)) / np.float64(n))
    if T_0to1 is None:
        return (math.nan, math.nan, math.nan, ratio)
    return P.pose_errors(T_0to1, R, t) + (ratio,)


def refine(kp0, kp1, K0, K1, R_in, t_in, mask_in, status_in, T_0to1=None, thresh=1.0, ordering="yx", rounds=2, lm_iters=10, reverse=False,
           trace=None):
    """one pair: kp [n, 2|3] float32 (the n matches), the pose, mask [n] and status einx_relative_pose returned for it.
    -> dict(R, t, mask, rows, info = (kept, rounds run, steps accepted, |S| of the last round run), cost = (before, after), c_in, c_ref)"""
    kp0, kp1 = np.asarray(kp0)[:, :2], np.asarray(kp1)[:, :2]
    n = len(kp0)
    if status_in < 0:
        return {"R": np.zeros((3, 3)), "t": np.zeros(3), "mask": np.zeros(n, bool), "rows": (math.inf, math.inf, math.inf, 0.0),
                "info": (-1, 0, 0, 0), "cost": (math.nan, math.nan), "c_in": 0, "c_ref": 0}
    if ordering == "yx":
        kp0, kp1 = kp0[:, ::-1], kp1[:, ::-1]
    x1, x2 = P.normalize(kp0, K0), P.normalize(kp1, K1)
    thr = P.ransac_threshold(thresh, K0, K1)
    thr2 = np.float32(thr * thr)
    R_in, t_in = np.asarray(R_in, np.float64), np.asarray(t_in, np.float64)
    c_in = int(np.count_nonzero(sampson_inliers(R_in, t_in, x1, x2, thr2, trace, "c_in")))
    R, t, acc, ran, last, cost = R_in, t_in, 0, 0, 0, (math.nan, math.nan)
    for r in range(rounds):
        S = sampson_inliers(R, t, x1, x2, thr2, trace, f"S_{r}")
        if np.count_nonzero(S) < MIN_SET:
            break
        R, t, a, c0, c1 = lm(R, t, x1[S], x2[S], lm_iters, reverse)
        ran, last, acc = ran + 1, int(np.count_nonzero(S)), acc + a
        cost = (c0 / last, c1 / last)
    inl = sampson_inliers(R, t, x1, x2, thr2, trace, "c_ref")
    c_ref = int(np.count_nonzero(inl))
    if acc > 0 and c_ref >= c_in:
        mask = np.zeros(n, bool)
        sel = np.nonzero(inl)[0]
        ok, depth = cheirality(R, t, x1[sel], x2[sel])
        if trace is not None:
            trace.append(("cheirality", "mask", depth, ok))
        mask[sel] = ok
        kept = 1
    else:
        R, t, mask, kept = R_in, t_in, np.asarray(mask_in, bool).copy(), 0
    return {"R": R, "t": t, "mask": mask, "rows": rows_of(T_0to1, R, t, mask, n), "info": (kept, ran, acc, last), "cost": cost,
            "c_in": c_in, "c_ref": c_ref}
