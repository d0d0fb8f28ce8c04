"""numpy float64 restatement of the pose-track rules (include/einx.h: einx_pose_interp, einx_pose_relative,
einx_nearest_stamp), written from those rules and from what scipy's Slerp and linear interp1d compute -- without scipy, which is
not among the test dependencies.  tests/golden/gen_poses.py records what the reference's PoseInterpolator (scipy) gives on the
same tracks; tests/test_poses_cpu.py holds this file to those records, the GPU tests hold the kernels to this file.

Every function is vectorised over the queries and evaluates each expression in the order the kernel does."""
import numpy as np

LERP_BELOW = 1e-12  # rad: below this angle between two knots the slerp is a normalised lerp


# ---- knots ------------------------------------------------------------------------------------------------------------------
def nearest_rotation(M):
    """[N,3,3] -> the rotation nearest to each matrix: the polar factor U V^T of its SVD, with the last column of U negated where
    that product is a reflection"""
    U, _, Vt = np.linalg.svd(np.asarray(M, np.float64))
    R = U @ Vt
    flip = np.linalg.det(R) < 0
    U[flip, :, 2] *= -1.0
    R[flip] = U[flip] @ Vt[flip]
    return R


def quat_from_matrix(R):
    """[N,3,3] rotations -> [N,4] unit quaternions (x, y, z, w) by the largest of (m00, m11, m22, trace)"""
    R = np.asarray(R, np.float64)
    q = np.empty((R.shape[0], 4))
    for n, m in enumerate(R):
        dec = (m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2])
        c = int(np.argmax(dec))
        if c != 3:
            i, j, k = c, (c + 1) % 3, (c + 2) % 3
            q[n, i] = 1.0 - dec[3] + 2.0 * m[i, i]
            q[n, j] = m[j, i] + m[i, j]
            q[n, k] = m[k, i] + m[i, k]
            q[n, 3] = m[k, j] - m[j, k]
        else:
            q[n] = (m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1.0 + dec[3])
    return q / np.sqrt((q * q).sum(1, keepdims=True))


def knots(R, quat_R=False):
    """the track's unit quaternions [N,4] (x, y, z, w) from PoseInterpolator's `R` argument"""
    R = np.asarray(R, np.float64)
    if quat_R:
        return R / np.sqrt((R * R).sum(1, keepdims=True))
    return quat_from_matrix(nearest_rotation(R))


def matrix_from_quat(q):
    """[Q,4] unit quaternions (x, y, z, w) -> [Q,3,3]"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = x2 - y2 - z2 + w2
    R[:, 1, 0] = 2.0 * (xy + zw)
    R[:, 2, 0] = 2.0 * (xz - yw)
    R[:, 0, 1] = 2.0 * (xy - zw)
    R[:, 1, 1] = -x2 + y2 - z2 + w2
    R[:, 2, 1] = 2.0 * (yz + xw)
    R[:, 0, 2] = 2.0 * (xz + yw)
    R[:, 1, 2] = 2.0 * (yz - xw)
    R[:, 2, 2] = -x2 - y2 + z2 + w2
    return R


# ---- interpolation ---------------------------------------------------------------------------------------------------------
def world_from_camera(stamps, trans, quats, queries):
    """(R [Q,3,3], p [Q,3], bad [Q]) of T_W_j at every query; rows of `bad` queries (outside the track or NaN) are NaN"""
    ts, p, qk = np.asarray(stamps, np.float64), np.asarray(trans, np.float64), np.asarray(quats, np.float64)
    q = np.atleast_1d(np.asarray(queries, np.float64))
    N = ts.shape[0]
    with np.errstate(invalid="ignore"):
        bad = ~((q >= ts[0]) & (q <= ts[-1]))
    qs = np.where(bad, ts[0], q)
    i = np.clip(np.searchsorted(ts, qs, side="left") - 1, 0, N - 2)
    dt, dq = ts[i + 1] - ts[i], qs - ts[i]
    alpha = dq / dt
    pos = (p[i + 1] - p[i]) / dt[:, None] * dq[:, None] + p[i]
    q0, q1 = qk[i], qk[i + 1].copy()
    d = ((q0[:, 0] * q1[:, 0] + q0[:, 1] * q1[:, 1]) + q0[:, 2] * q1[:, 2]) + q0[:, 3] * q1[:, 3]
    neg = d < 0.0
    q1[neg] = -q1[neg]
    d = np.where(neg, -d, d)
    r = q1 - d[:, None] * q0
    s = np.sqrt(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) + r[:, 3] * r[:, 3])
    theta = np.arctan2(s, d)
    lerp = theta < LERP_BELOW
    th = np.where(lerp, 1.0, theta)
    w0 = np.where(lerp, 1.0 - alpha, np.sin((1.0 - alpha) * th) / np.sin(th))
    w1 = np.where(lerp, alpha, np.sin(alpha * th) / np.sin(th))
    qi = w0[:, None] * q0 + w1[:, None] * q1
    qi = qi / np.sqrt(((qi[:, 0] * qi[:, 0] + qi[:, 1] * qi[:, 1]) + qi[:, 2] * qi[:, 2]) + qi[:, 3] * qi[:, 3])[:, None]
    R = matrix_from_quat(qi)
    R[bad], pos[bad] = np.nan, np.nan
    return R, pos, bad


def rigid(R, p):
    T = np.zeros((R.shape[0], 4, 4))
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, p, 1.0
    return T


def rigid_inverse(R, p):
    """[R^T | -R^T p], each entry of the translation summed left to right"""
    Rt = np.swapaxes(R, 1, 2)
    t = -((Rt[:, :, 0] * p[:, None, 0] + Rt[:, :, 1] * p[:, None, 1]) + Rt[:, :, 2] * p[:, None, 2])
    return Rt, t


def interpolate(stamps, trans, quats, queries, inverse=True):
    """[Q,4,4] float64: T_j_W (inverse, what PoseInterpolator.interpolate returns) or T_W_j; all-NaN rows for queries outside the
    track.  Second value: the number of such queries."""
    R, p, bad = world_from_camera(stamps, trans, quats, queries)
    T = rigid(*rigid_inverse(R, p)) if inverse else rigid(R, p)
    T[bad] = np.nan
    return T, int(bad.sum())


def compose(Ra, ta, Rb, tb):
    """(Ra | ta) (Rb | tb), every entry summed left to right"""
    R = (Ra[:, :, 0, None] * Rb[:, None, 0, :] + Ra[:, :, 1, None] * Rb[:, None, 1, :]) + Ra[:, :, 2, None] * Rb[:, None, 2, :]
    t = ((Ra[:, :, 0] * tb[:, None, 0] + Ra[:, :, 1] * tb[:, None, 1]) + Ra[:, :, 2] * tb[:, None, 2]) + ta
    return R, t


def relative(stamps, trans, quats, q0, q1):
    """(T_0to1, T_1to0) [P,4,4] float64 with T_0to1 = T_1_W T_W_0 and T_1to0 = T_0_W T_W_1; a pair with a query outside the track has
    NaN rows in both.  Third value: the number of such QUERIES (a pair can count twice)."""
    R0, p0, bad0 = world_from_camera(stamps, trans, quats, q0)
    R1, p1, bad1 = world_from_camera(stamps, trans, quats, q1)
    T01 = rigid(*compose(*rigid_inverse(R1, p1), R0, p0))
    T10 = rigid(*compose(*rigid_inverse(R0, p0), R1, p1))
    bad = bad0 | bad1
    T01[bad], T10[bad] = np.nan, np.nan
    return T01, T10, int(bad0.sum()) + int(bad1.sum())


# ---- pairing ----------------------------------------------------------------------------------------------------------------
def nearest_index(stamps, queries):
    """np.abs(np.subtract.outer(stamps, q)).argmin(axis=0) for sorted stamps without the F x Q matrix: the first index whose
    |stamps[i] - q|, rounded to float64, is minimal.  The rounded distance does not increase up to the last stamp below q and does
    not decrease from the first stamp >= q on, so the minimum lies at one of those two and its first occurrence is found by
    bisection on the side it lies on."""
    s = np.asarray(stamps, np.float64)
    out = np.zeros(len(queries), np.int64)
    for k, q in enumerate(np.asarray(queries, np.float64)):
        j = int(np.searchsorted(s, q, side="left")) if not np.isnan(q) else 0
        dist = lambda i: abs(s[i] - q)  # noqa: E731
        if j == 0 or (j < len(s) and dist(j) < dist(j - 1)):
            out[k] = j if j < len(s) else 0
            continue
        m, lo, hi = dist(j - 1), 0, j - 1  # first i in [0, j - 1] with dist(i) <= m
        while lo < hi:
            mid = (lo + hi) // 2
            if dist(mid) <= m:
                hi = mid
            else:
                lo = mid + 1
        out[k] = lo
    return out


def nearest_index_dense(stamps, queries):
    """the reference's expression itself (datasets/MVSEC.py:364-366)"""
    with np.errstate(invalid="ignore"):
        return np.abs(np.subtract.outer(np.asarray(stamps, np.float64), np.asarray(queries, np.float64))).argmin(axis=0).astype(np.int64)


# ---- tracks of the fixture and the GPU tests ---------------------------------------------------------------------------------------
def rotvec_matrix(v):
    """Rodrigues: rotation vector [3] -> [3,3]"""
    v = np.asarray(v, np.float64)
    th = np.sqrt((v * v).sum())
    if th == 0.0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def make_track(seed, N=24, t0=1.5e9, perturb=0.0, identical=(7, 8), near=(15, 16)):
    """(stamps [N], t [N,3], R [N,3,3]): epoch-scale stamps 5..20 ms apart; rotations that mix small steps (<= 0.05 rad) with jumps
    (up to 2.5 rad), one pair of identical neighbours and one pair 1e-9 rad apart; every matrix entry perturbed by up to
    `perturb`"""
    rng = np.random.default_rng(seed)
    stamps = t0 + np.cumsum(rng.uniform(0.005, 0.020, N))
    t = np.cumsum(rng.normal(size=(N, 3)) * 0.3, 0) + rng.normal(size=3) * 3.0
    R = np.empty((N, 3, 3))
    cur = rotvec_matrix(rng.normal(size=3))
    for n in range(N):
        axis = rng.normal(size=3)
        axis /= np.sqrt((axis * axis).sum())
        ang = rng.uniform(0.8, 2.5) if n % 5 == 4 else rng.uniform(0.0, 0.05)
        if N > 2 and n == identical[1]:
            ang = 0.0
        if N > 2 and n == near[1]:
            ang = 1e-9
        if n:
            cur = cur @ rotvec_matrix(axis * ang)
        R[n] = cur
    if perturb:
        delta = rng.uniform(-perturb, perturb, R.shape)
        if N > 2:
            delta[near[1]] = delta[near[0]]  # the same error on both: their nearest rotations stay about 1e-9 rad apart
        R = R + delta
    if N > 2:
        R[identical[1]] = R[identical[0]]
    return stamps, t, R


def make_queries(seed, stamps, near=(15, 16)):
    """200 uniform queries over the track, every knot, and 50 inside the stretch between the two near-identical knots"""
    rng = np.random.default_rng(seed)
    q = [rng.uniform(stamps[0], stamps[-1], 200), stamps]
    if len(stamps) > near[1]:
        q.append(rng.uniform(stamps[near[0]], stamps[near[1]], 50))
    return np.concatenate(q)


def neighbour_angles(R):
    """[N-1] rotation angle between neighbouring knots (of their nearest rotations)"""
    Rn = nearest_rotation(R)
    rel = np.swapaxes(Rn[:-1], 1, 2) @ Rn[1:]
    return np.arccos(np.clip((np.trace(rel, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0))


TRACK_CASES = [  # name, make_track arguments, quaternion input
    ("exact", dict(seed=1), False),
    ("p1e-7", dict(seed=2, perturb=1e-7), False),
    ("p1e-4", dict(seed=3, perturb=1e-4), False),
    ("p1e-2", dict(seed=4, perturb=1e-2), False),
    ("n2", dict(seed=5, N=2), False),
    ("quat", dict(seed=6), True),
]


def track_case(name):
    """(stamps, t, R or quaternions, quat_R, queries) of a fixture case; the quaternion case hands over UN-normalised quaternions"""
    kw, quat = next((k, q) for n, k, q in TRACK_CASES if n == name)
    stamps, t, R = make_track(**kw)
    if quat:
        R = quat_from_matrix(R) * np.random.default_rng(kw["seed"] + 100).uniform(0.5, 2.0, (R.shape[0], 1))
    return stamps, t, R, quat, make_queries(kw["seed"] + 50, stamps)


PAIRING_CASES = {
    "tie": ([0.0, 1.0, 1.0, 2.0, 4.0], [-1.0, 0.5, 1.0, 3.0, 9.0]),
    "dup_run": ([1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 3.0, 3.0, 5.0], [2.0, 2.4, 2.5, 2.6, 3.0, 4.0, 4.5, 0.0, 7.0]),
    # stamps of mixed magnitude: 1e16 - 1, 1e16 - 1.5 and 1e16 - 1.75 all round to 1e16, so DIFFERENT stamps tie after rounding
    # (the answer is the first of them, not the last stamp below the query); 1.5e16 ties across the query as well
    "mixed": ([1.0, 1.5, 1.75, 3e16], [1e16, 2e16, 1.6, -1e16, 1.5e16, 1.74, 3e16]),
    "nan": ([1.0, 2.0, 3.0], [float("nan"), 2.2, float("nan"), float("inf"), -float("inf")]),
}
