"""Relative pose of ONE pair, written from the contract of DESIGN.md section 8b in float64 numpy (the answer csrc/pose.hip is
measured against).  Not collected by pytest (no test_ prefix).  The minimal solver takes a different route from the kernel's
(action matrix + numpy.linalg.eig here, Nister's degree-10 polynomial + bisection there), so that the two do not share a
mistake; everything else (generator, normalisation, inlier rule, selection scan, candidate order) is the contract itself."""
import math

import numpy as np

MASK64 = (1 << 64) - 1
# ground-truth pose-error bounds (degrees) shared by the CPU test of this restatement and the GPU test of the kernels: the worst
# of their fixed seeds with margin.  MVSEC-like float32 keypoints, the default ~1 px threshold.
GT_BOUNDS = {"noise_free": 0.02, "outliers_30": 6.0, "outliers_60": 8.0}
FORWARD = (0.02, 0.01, 1.0)  # forward driving (MVSEC outdoor_day): the parametrisation's E[1,2], E[2,0], E[2,1], E[2,2] are all small
DEFAULT_SEED = 0x5EED0F5E


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed, it, n, retries=64):
    """five distinct indices of [0, n) for RANSAC iteration `it`: draw d, retry r -> splitmix64(seed ^ (it << 16 | d << 8 | r)) % n;
    None when a draw finds no new index within `retries` tries"""
    out = []
    for d in range(5):
        for r in range(retries):
            v = splitmix64((seed ^ ((it << 16) | (d << 8) | r)) & MASK64) % n
            if v not in out:
                out.append(v)
                break
        else:
            return None
    return out


def ransac_threshold(thresh, K0, K1):
    """thresh / mean([K0[0,0], K1[1,1], K0[0,0], K1[1,1]]) as numpy evaluates it: K's dtype, left to right"""
    dt = np.result_type(K0.dtype, K1.dtype)
    a, b = dt.type(K0[0, 0]), dt.type(K1[1, 1])
    m = dt.type(dt.type(dt.type(dt.type(a + b) + a) + b) / dt.type(4))
    return float(dt.type(dt.type(thresh) / m))


def normalize(kp, K):
    """(x - cx) / fx, (y - cy) / fy in numpy's dtype for float32 keypoints and K, then widened to float64"""
    dt = np.result_type(np.float32, K.dtype)
    kp = kp.astype(dt)
    c = np.array([K[0, 2], K[1, 2]], dtype=dt)
    f = np.array([K[0, 0], K[1, 1]], dtype=dt)
    return ((kp - c) / f).astype(np.float64)


# ------------------------------------------------------------------ five-point solver (action matrix)
def null_basis(x1, x2):
    """rows x2 (x) x1 of the 5x9 system, reduced by Gauss-Jordan with partial pivoting over the first five columns (the same
    elimination as the kernel: a canonical basis with e5..e8 = x, y, z, 1).  Returns the 9x4 coefficient matrix of E(x, y, z)
    or None when a pivot falls below 1e-9 of the largest entry (a singular sample)."""
    A = np.empty((5, 9))
    for r in range(5):
        u1, v1 = x1[r]
        u2, v2 = x2[r]
        A[r] = [u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0]
    tol = 1e-9 * np.abs(A).max()
    for c in range(5):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if not abs(A[p, c]) > tol:
            return None
        A[[c, p]] = A[[p, c]]
        A[c] = A[c] / A[c, c]
        for r in range(5):
            if r != c:
                A[r] = A[r] - A[r, c] * A[c]
    Ec = np.zeros((9, 4))
    Ec[:5] = -A[:, 5:]
    Ec[5:] = np.eye(4)
    return Ec


# monomials x^i y^j z^k as exponent tuples; GRevLex degree-3 block first, then the ten of degree <= 2 (the quotient basis)
DEG3 = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
ALL = DEG3 + BASIS
LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _cubic_map():
    """64 x 20: the product of three linear forms over (x, y, z, 1), indexed (a, b, c), onto the monomials ALL"""
    P = np.zeros((64, 20))
    for a in range(4):
        for b in range(4):
            for c in range(4):
                e = tuple(LIN[a][v] + LIN[b][v] + LIN[c][v] for v in range(3))
                P[16 * a + 4 * b + c, ALL.index(e)] = 1.0
    return P


_P64 = _cubic_map()
_EPS = np.zeros((3, 3, 3))
for _i, _j, _k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
    _EPS[_i, _j, _k], _EPS[_i, _k, _j] = 1.0, -1.0


def constraints(Ec):
    """the 10 cubic constraints det E = 0 and 2 E E^T E - tr(E E^T) E = 0 as a 10x20 matrix over ALL"""
    E = Ec.reshape(3, 3, 4)
    det = np.einsum("pqr,pa,qb,rc->abc", _EPS, E[0], E[1], E[2])
    t1 = np.einsum("ila,klb,kjc->ijabc", E, E, E)
    t2 = np.einsum("mla,mlb,ijc->ijabc", E, E, E)
    T = np.concatenate([det[None], (2.0 * t1 - t2).reshape(9, 4, 4, 4)], 0)
    return T.reshape(10, 64) @ _P64


def _polish(Ec, p, steps=6):
    """Gauss-Newton on det E = 0 and 2 E E^T E - tr(E E^T) E = 0 from an eigenpair's (x, y, z), evaluated on E(x, y, z) itself:
    eigenvectors alone lose digits on ill-conditioned samples, and the cubics expanded over the monomials (`constraints`) carry
    coefficients of |Ec|^3 that cancel, which leaves E 1e-8 off the essential variety there"""
    B = Ec.reshape(3, 3, 4)
    for _ in range(steps):
        E = B @ np.array([p[0], p[1], p[2], 1.0])
        EEt = E @ E.T
        tr = np.trace(EEt)
        r = np.concatenate([[np.linalg.det(E)], (2.0 * EEt @ E - tr * E).ravel()])
        C = cofactor(E)
        J = np.zeros((10, 3))
        for v in range(3):
            D = B[:, :, v]
            J[0, v] = np.sum(C * D)
            J[1:, v] = (2.0 * (D @ E.T @ E + E @ D.T @ E + EEt @ D) - 2.0 * np.sum(E * D) * E - tr * D).ravel()
        step = np.linalg.lstsq(J, -r, rcond=None)[0]
        if not np.all(np.isfinite(step)):
            break
        p = p + step
    return p


def solve5(x1, x2):
    """every real essential matrix of five normalised correspondences, ordered by ascending z = E[2,1] / E[2,2]; each scaled so
    that E[2,2] = 1 (the parametrisation).  [] for a singular sample."""
    Ec = null_basis(x1, x2)
    if Ec is None:
        return []
    M = constraints(Ec)
    if np.linalg.cond(M[:, :10]) > 1e13:
        return []
    Bm = np.linalg.solve(M[:, :10], M[:, 10:])  # deg3 monomial = -Bm . basis
    At = np.zeros((10, 10))  # multiplication by x on the quotient basis
    for i, e in enumerate(BASIS[:6]):
        At[i] = -Bm[DEG3.index((e[0] + 1, e[1], e[2]))]
    for i, e in ((6, 0), (7, 1), (8, 2), (9, 6)):
        At[i, e] = 1.0
    w, V = np.linalg.eig(At)
    sols = []
    for k in range(10):
        if abs(w[k].imag) > 1e-8 * max(1.0, abs(w[k].real)):
            continue
        v = V[:, k].real
        if not abs(v[9]) > 0:
            continue
        xyz = _polish(Ec, np.array([w[k].real, v[7] / v[9], v[8] / v[9]]))
        E = Ec @ np.array([xyz[0], xyz[1], xyz[2], 1.0])
        if not np.all(np.isfinite(E)):
            continue
        # the kernel's guard against a root lost to cancellation: det E below 1e-6 |E|^3
        if abs(np.linalg.det(E.reshape(3, 3))) <= 1e-6 * np.linalg.norm(E) ** 3:
            sols.append(E.reshape(3, 3))
    sols.sort(key=lambda E: E[2, 1])
    # a double root shows up twice in eig: keep distinct roots only (the kernel finds distinct roots)
    out = []
    for E in sols:
        if not out or abs(E[2, 1] - out[-1][2, 1]) > 1e-9 * max(1.0, abs(E[2, 1])):
            out.append(E)
    return out


# ------------------------------------------------------------------ RANSAC
def sampson_f32(E, x1, x2):
    """OpenCV EMEstimatorCallback::computeError's operation order, rounded to float"""
    e = E.reshape(9)
    u1, v1, u2, v2 = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    a = e[0] * u1 + e[1] * v1 + e[2]
    b = e[3] * u1 + e[4] * v1 + e[5]
    c = e[6] * u1 + e[7] * v1 + e[8]
    s2 = e[0] * u2 + e[3] * v2 + e[6]
    s1 = e[1] * u2 + e[4] * v2 + e[7]
    d1 = u2 * a + v2 * b + c
    with np.errstate(invalid="ignore", divide="ignore"):
        return (d1 * d1 / (a * a + b * b + s2 * s2 + s1 * s1)).astype(np.float32), (d1 * d1 / (a * a + b * b + s2 * s2 + s1 * s1))


def update_iters(conf, ep, bound):
    """RANSACUpdateNumIters with (1 - ep)^5 as four products"""
    p = min(max(conf, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, 2.2250738585072014e-308)
    q = 1.0 - ep
    denom = 1.0 - q * q * q * q * q
    if denom < 2.2250738585072014e-308:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= bound * (-denom):
        return bound
    return int(math.floor(num / denom + 0.5))


def ransac(x1, x2, thr, conf=0.999, max_iters=1000, seed=DEFAULT_SEED):
    """-> (E or None, inlier mask, chosen (iteration, solution) or None, candidate list for the 5-match case)"""
    n = len(x1)
    thr2 = np.float32(thr * thr)
    if n == 5:
        sols = solve5(x1, x2)
        return sols, np.ones(n, bool), None
    best, best_cnt, bound = None, 0, max_iters
    for it in range(max_iters):
        if it >= bound:
            break
        idx = draw(seed, it, n)
        if idx is None:
            continue
        for s, E in enumerate(solve5(x1[idx], x2[idx])):
            err, _ = sampson_f32(E, x1, x2)
            cnt = int(np.count_nonzero(err <= thr2))
            if cnt > max(best_cnt, 4):
                best, best_cnt = (it, s, E), cnt
                bound = update_iters(conf, (n - cnt) / n, bound)
    if best is None:
        return [], np.zeros(n, bool), None
    err, _ = sampson_f32(best[2], x1, x2)
    return [best[2]], err <= thr2, best[:2]


# ------------------------------------------------------------------ recover pose
def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def cofactor(E):
    return np.stack([np.cross(E[1], E[2]), np.cross(E[2], E[0]), np.cross(E[0], E[1])])


def decompose(E):
    """(R1, R2, t) of E scaled to Frobenius norm sqrt(2): t = the unit left null vector from the largest cross product of two
    columns (first of (0,1), (0,2), (1,2) on ties), R1 = cof(E) - [t]x E, R2 = cof(E) + [t]x E"""
    E = E * (math.sqrt(2.0) / np.linalg.norm(E))
    best, t = -1.0, None
    for i, j in ((0, 1), (0, 2), (1, 2)):
        c = np.cross(E[:, i], E[:, j])
        nc = float(np.dot(c, c))
        if nc > best:
            best, t = nc, c
    t = t / math.sqrt(best)
    C, S = cofactor(E), skew(t) @ E
    return C - S, C + S, t


def triangulate_ok(R, t, x1, x2, dist=1e9):
    """DLT against [I|0] and [R|t] by SVD; OpenCV recoverPose's depth tests"""
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    P1 = np.hstack([R, t[:, None]])
    ok = np.zeros(len(x1), bool)
    for i in range(len(x1)):
        A = np.stack([x1[i, 0] * P0[2] - P0[0], x1[i, 1] * P0[2] - P0[1], x2[i, 0] * P1[2] - P1[0], x2[i, 1] * P1[2] - P1[1]])
        X = np.linalg.svd(A)[2][3]
        if not X[2] * X[3] > 0:
            continue
        Xh = X / X[3]
        z2 = P1[2] @ Xh
        ok[i] = Xh[2] < dist and z2 > 0 and z2 < dist
    return ok


def recover_pose(E, x1, x2, mask):
    R1, R2, t = decompose(E)
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    goods = []
    for R, tt in cands:
        ok = np.zeros(len(x1), bool)
        sel = np.nonzero(mask)[0]
        ok[sel] = triangulate_ok(R, tt, x1[sel], x2[sel])
        goods.append(ok)
    cnt = [int(g.sum()) for g in goods]
    k = int(np.argmax(cnt))  # first maximum: (R1,t), (R2,t), (R1,-t), (R2,-t)
    return cnt[k], cands[k][0], cands[k][1], goods[k]


def relative_pose(kp0, kp1, K0, K1, thresh=1.0, conf=0.999, ordering="yx", max_iters=1000, seed=DEFAULT_SEED):
    """one pair end to end: kp [N, 2|3] float32, K [3,3].  -> dict(status, R, t, mask, it)
    status: 'ok', 'few' (fewer than 5 matches), 'noE' (no essential matrix), 'cheir' (no point passes)"""
    kp0, kp1 = np.asarray(kp0)[:, :2], np.asarray(kp1)[:, :2]
    n = len(kp0)
    if n < 5:
        return {"status": "few", "mask": np.zeros(n, bool)}
    if ordering == "yx":
        kp0, kp1 = kp0[:, ::-1], kp1[:, ::-1]
    x1, x2 = normalize(kp0, K0), normalize(kp1, K1)
    thr = ransac_threshold(thresh, K0, K1)
    Es, mask, chosen = ransac(x1, x2, thr, conf, max_iters, seed)
    if not Es:
        return {"status": "noE", "mask": np.zeros(n, bool)}
    best, ret = 0, None
    for s, E in enumerate(Es):  # the reference's loop over the stacked solutions, one in/out mask (matching_metrics.py:442-450)
        cnt, R, t, ok = recover_pose(E, x1, x2, mask)
        mask = ok
        if cnt > best:
            best, ret = cnt, (R, t, mask.copy(), chosen if chosen is not None else (0, s), E)
    if ret is None:
        return {"status": "cheir", "mask": np.zeros(n, bool)}
    return {"status": "ok", "R": ret[0], "t": ret[1], "mask": ret[2], "it": ret[3], "E": ret[4]}


def pose_errors(T_0to1, R, t):
    """relative_pose_error + update_one's epilogue (matching_metrics.py:452-518) -> (R_err, t_err, pose_err)"""
    T = np.asarray(T_0to1, dtype=np.float64)
    t_gt = T[:3, 3]
    n = np.linalg.norm(t) * np.linalg.norm(t_gt)
    with np.errstate(invalid="ignore", divide="ignore"):
        t_err = np.rad2deg(np.arccos(np.clip(np.dot(t, t_gt) / n, -1.0, 1.0)))
    t_err = np.minimum(t_err, 180 - t_err)
    if not np.isfinite(np.linalg.norm(t_gt)):
        t_err = 0.0
    cos = np.clip((np.trace(np.dot(R.T, T[:3, :3])) - 1) / 2, -1.0, 1.0)
    R_err = np.rad2deg(np.abs(np.arccos(cos)))
    pose_err = max(R_err, t_err) if np.isfinite(t_err) else R_err
    return float(R_err), float(t_err), float(pose_err)


# ------------------------------------------------------------------ synthetic scenes
def rotation(axis, deg):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    a = math.radians(deg)
    K = skew(axis)
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def scene(rng, n, max_deg=15.0, noise=0.0, outliers=0.0, W=346, H=260, f=226.0, t_dir=None, min_deg=1.0):
    """MVSEC-like pair: K float32 (fx ~ fy ~ 226, 346 x 260), depths 2-10 m, rotation of min_deg..max_deg.  t_dir: a fixed
    translation direction (forward driving: (0.02, 0.01, 1)); a random one otherwise.  Keypoints float32 in (y, x) order with a
    score column, like the extractors' matches.  -> (kp0, kp1, K0, K1, T_0to1 [4,4] float32)"""
    K = np.array([[f + rng.uniform(-2, 2), 0, W / 2 + rng.uniform(-3, 3)], [0, f + rng.uniform(-2, 2), H / 2 + rng.uniform(-3, 3)],
                  [0, 0, 1]], np.float32)
    R = rotation(rng.normal(size=3), rng.uniform(min_deg, max_deg))
    t = rng.normal(size=3) if t_dir is None else np.asarray(t_dir, float)
    t = t / np.linalg.norm(t) * rng.uniform(0.3, 1.0)
    pts0, pts1 = [], []
    Kd = K.astype(np.float64)
    while len(pts0) < n:
        u, v, z = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(2, 10)
        X = np.linalg.solve(Kd, np.array([u, v, 1.0])) * z
        X1 = R @ X + t
        if X1[2] <= 0.5:
            continue
        p = Kd @ (X1 / X1[2])
        if not (0 <= p[0] < W and 0 <= p[1] < H):
            continue
        pts0.append([u, v])
        pts1.append(p[:2])
    pts0, pts1 = np.array(pts0), np.array(pts1)
    if noise:
        pts0 = pts0 + rng.normal(scale=noise, size=pts0.shape)
        pts1 = pts1 + rng.normal(scale=noise, size=pts1.shape)
    n_out = int(round(outliers * n))
    if n_out:
        sel = rng.choice(n, n_out, replace=False)
        pts1[sel] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)], 1)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    score = rng.uniform(0, 1, (n, 1))
    kp0 = np.hstack([pts0[:, ::-1], score]).astype(np.float32)
    kp1 = np.hstack([pts1[:, ::-1], score]).astype(np.float32)
    return kp0, kp1, K, K.copy(), T
