"""numpy restatement of DESIGN.md 8e (ground-truth matches from depth + pose or a homography, matcher precision / recall) and the
integer-built scenes its fixture (tests/golden/gt_matches.npz, generator gen_gt_matches.py) and tests share.  Not collected.

Stage A (`project`, `warp`) runs in the dtype it is given: float32 follows the kernel's operation order (every product and sum
rounded separately), float64 is the exact-arithmetic yardstick the reference's own float noise is measured against.  Stage B
(`label`) and stage C (`match_pr`) are the written algorithm; `label` works on given projections and is bit-exact in float32."""
import numpy as np

IGNORE, UNMATCHED = -2, -1


# ------------------------------------------------------------------------------------------------ integer-built inputs
def _mix(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def ints(seed, shape, mod):
    """uniform integers in [0, mod) from a 64-bit integer hash of (seed, index): the same on every platform"""
    n = int(np.prod(shape)) if len(shape) else 1
    with np.errstate(over="ignore"):
        x = _mix(_mix(np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x100000001B3)))
    return (x % np.uint64(mod)).astype(np.int64).reshape(shape)


def _pose(seed, b, kind):
    """small-integer-ratio motions: rotation about the optical axis by a Pythagorean angle, translation in 1/16 steps"""
    c, s = [(24, 7), (40, 9), (60, 11), (12, 5)][int(ints(seed + 11, (8,), 4)[b % 8])]
    h = float(np.hypot(c, s))  # 25, 41, 61, 13: exact
    c, s = c / h, s / h
    if ints(seed + 12, (8,), 2)[b % 8]:
        s = -s
    t = (ints(seed + 13, (8, 3), 9)[b % 8] - 4) / 16.0
    if kind == "behind":
        t[2] = -5.0
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = t
    return T


def invert_pose_f32(T):
    """(R^T, -R^T t) in float32 with the kernel's operation order: what passing T_1to0 = NULL computes"""
    T = np.asarray(T, np.float32)
    out = np.zeros_like(T)
    R = np.swapaxes(T[..., :3, :3], -1, -2)
    t = T[..., :3, 3]
    out[..., :3, :3] = R
    out[..., :3, 3] = -((R[..., 0] * t[..., None, 0] + R[..., 1] * t[..., None, 1]) + R[..., 2] * t[..., None, 2])
    out[..., 3, 3] = 1
    return out


def scene(seed, B, n, m, size0, size1, counts0=None, counts1=None, f0=64.0, f1=64.0, n_corr=40, n_dup=5, behind=(), hole_pct=3):
    """B pairs, n x m keypoints (x, y) on depth maps of size0 / size1 = (H, W): depths k/64 around a fronto-parallel plane (so the two
    views are consistent up to the k/64 relief), holes (0, a negative value, NaN) at hole_pct % of the pixels and under the first
    keypoints, half-integer keypoints (the extractors' grid) mixed with quarter-offset ones, the first n_corr keypoints of side 1 the
    projections of side-0 keypoints plus a triangular noise of sigma 1.5 px in quarter-pixel steps, n_dup exact duplicates of
    corresponding columns, pairs listed in `behind` moved so that side 0's points fall behind camera 1.
    Returns float32 arrays: kp0 [B,n,2], kp1 [B,m,2], depth0 [B,H0,W0], depth1, K0, K1 [B,3,3], T01, T10 [B,4,4], and int32 counts."""
    (H0, W0), (H1, W1) = size0, size1
    out = {k: [] for k in ("kp0", "kp1", "depth0", "depth1", "K0", "K1", "T01", "T10")}
    for b in range(B):
        sd = seed * 1000 + b * 37
        K0 = np.array([[f0, 0, W0 / 2], [0, f0, H0 / 2], [0, 0, 1]])
        K1 = np.array([[f1, 0, W1 / 2], [0, f1, H1 / 2], [0, 0, 1]])
        T = _pose(sd, b, "behind" if b in behind else "")
        Ti = np.eye(4)
        Ti[:3, :3] = T[:3, :3].T
        Ti[:3, 3] = -T[:3, :3].T @ T[:3, 3]
        z0 = 4.0
        z1 = z0 + (T[2, 3] if b not in behind else 0.0)
        d0 = (z0 * 64 + ints(sd + 1, (H0, W0), 17) - 8) / 64.0
        d1 = (z1 * 64 + ints(sd + 2, (H1, W1), 17) - 8) / 64.0
        for d, s in ((d0, sd + 3), (d1, sd + 4)):
            r = ints(s, d.shape, 300)
            d[r < hole_pct] = 0.0
            d[r == hole_pct] = -1.0
            d[r == hole_pct + 1] = np.nan
        # odd quarters (fractions .25 / .75): a keypoint is either wholly on the half-integer grid or wholly off it.  (With ONE
        # coordinate on the grid, a hole under the zero-weight tap is seen or not by the reference depending on how its own
        # x / W * 2 - 1 round trip rounds: DESIGN.md 8e.)
        kp0 = np.stack([2 * ints(sd + 5, (n,), 2 * W0 - 4) + 5, 2 * ints(sd + 6, (n,), 2 * H0 - 4) + 5], 1) / 4.0
        kp1 = np.stack([2 * ints(sd + 7, (m,), 2 * W1 - 4) + 5, 2 * ints(sd + 8, (m,), 2 * H1 - 4) + 5], 1) / 4.0
        half0, half1 = ints(sd + 9, (n,), 3) > 0, ints(sd + 10, (m,), 3) > 0  # two thirds on the extractors' half-integer grid
        kp0[half0] = np.floor(kp0[half0]) + 0.5
        kp1[half1] = np.floor(kp1[half1]) + 0.5
        nc = min(n_corr, n, m)
        if nc:
            src = np.argsort(ints(sd + 14, (n,), 1 << 30), kind="stable")[:nc]
            p = np.stack([(kp0[src, 0] - K0[0, 2]) / f0, (kp0[src, 1] - K0[1, 2]) / f0, np.ones(nc)], 1) * z0
            q = p @ T[:3, :3].T + T[:3, 3]
            if b not in behind:
                uv = q[:, :2] / q[:, 2:] * f1 + K1[:2, 2]
                noise = (ints(sd + 15, (nc, 2, 3), 12).sum(-1) * 2 - 33) / 8.0  # odd eighths: never an exact integer pixel offset
                kp1[:nc] = np.rint(uv * 4) / 4.0 + noise
            for k in range(min(n_dup, nc, m - nc)):
                kp1[m - 1 - k] = kp1[k]
        # holes under the first keypoints of side 0: under a half-integer keypoint (its one tap), under one tap of four
        for i in range(min(6, n)):
            x0, y0 = int(np.floor(kp0[i, 0] - 0.5)), int(np.floor(kp0[i, 1] - 0.5))
            if 0 <= x0 < W0 - 1 and 0 <= y0 < H0 - 1:
                d0[y0 + (i % 2), x0 + ((i // 2) % 2)] = [0.0, np.nan, -2.0][i % 3]
        out["kp0"].append(kp0), out["kp1"].append(kp1), out["depth0"].append(d0), out["depth1"].append(d1)
        out["K0"].append(K0), out["K1"].append(K1), out["T01"].append(T), out["T10"].append(Ti)
    res = {k: np.ascontiguousarray(np.stack(v).astype(np.float32)) for k, v in out.items()}
    res["n"] = np.asarray(counts0 if counts0 is not None else [n] * B, np.int32)
    res["m"] = np.asarray(counts1 if counts1 is not None else [m] * B, np.int32)
    return res


def homography_scene(seed, B, n, m, size=(200, 260)):
    """kp0 / kp1 (x, y) on quarter pixels, H = a small integer-ratio affinity plus a perspective row; half of the smaller side corresponds"""
    H_, W_ = size
    kp0s, kp1s, Hs = [], [], []
    for b in range(B):
        sd = seed * 1000 + b * 41
        a = (ints(sd, (9,), 17) - 8)
        Hm = np.array([[1 + a[0] / 64, a[1] / 64, a[2] / 2], [a[3] / 64, 1 + a[4] / 64, a[5] / 2], [a[6] / 16384, a[7] / 16384, 1.0]])
        kp0 = np.stack([ints(sd + 1, (n,), 4 * W_), ints(sd + 2, (n,), 4 * H_)], 1) / 4.0
        kp1 = np.stack([ints(sd + 3, (m,), 4 * W_), ints(sd + 4, (m,), 4 * H_)], 1) / 4.0
        nc = min(n, m) // 2
        w = np.concatenate([kp0[:nc], np.ones((nc, 1))], 1) @ Hm.T
        noise = (ints(sd + 5, (nc, 2, 3), 20).sum(-1) * 2 - 57) / 8.0
        kp1[:nc] = np.rint(w[:, :2] / w[:, 2:] * 4) / 4.0 + noise
        for k in range(min(4, nc)):
            kp1[m - 1 - k] = kp1[k]
        kp0s.append(kp0), kp1s.append(kp1), Hs.append(Hm)
    return {"kp0": np.stack(kp0s).astype(np.float32), "kp1": np.stack(kp1s).astype(np.float32), "H": np.stack(Hs).astype(np.float32)}


# ------------------------------------------------------------------------------------------------ stage A
def sample_depth(xy, depth, dt=np.float32):
    """one view: xy [n,2] (x, y), depth [H,W] -> (d [n], valid [n])"""
    H, W = depth.shape
    dm = np.asarray(depth, dt)
    x, y = np.asarray(xy[:, 0], dt), np.asarray(xy[:, 1], dt)
    ix, iy = x - dt(0.5), y - dt(0.5)
    fx0, fy0 = np.floor(ix), np.floor(iy)
    wx = [(fx0 + dt(1)) - ix, ix - fx0]
    wy = [(fy0 + dt(1)) - iy, iy - fy0]
    acc = np.zeros(len(x), dt)
    hole = np.zeros(len(x), bool)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = fx0.astype(np.int64) + dx, fy0.astype(np.int64) + dy
            inmap = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            v = dm[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            w = wx[dx] * wy[dy]
            good = inmap & (v > 0)
            hole |= inmap & ~(v > 0) & (w != 0)
            acc = np.where(good, acc + np.where(good, v, 0) * w, acc)
    nx, ny = np.rint(ix), np.rint(iy)  # half to even
    inmap = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
    v = dm[np.clip(ny.astype(np.int64), 0, H - 1), np.clip(nx.astype(np.int64), 0, W - 1)]
    near = np.where(inmap, np.where(v > 0, v, dt(np.nan)), dt(0))
    d = np.where(hole, near, acc).astype(dt)
    return d, ~np.isnan(d) & (d > 0)


def project_side(xy, d, valid, Ks, Ko, T, dt=np.float32):
    """one view: -> dict(proj [n,2], visible [n], qz, u, v, wmax, hmax) (the latter for the margins of the discrete decisions)"""
    Ks, Ko, T = np.asarray(Ks, dt), np.asarray(Ko, dt), np.asarray(T, dt)
    x, y, d = np.asarray(xy[:, 0], dt), np.asarray(xy[:, 1], dt), np.asarray(d, dt)
    eps = dt(np.float32(1e-4))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        px, py, pz = ((x - Ks[0, 2]) / Ks[0, 0]) * d, ((y - Ks[1, 2]) / Ks[1, 1]) * d, d
        q = [((px * T[r, 0] + py * T[r, 1]) + pz * T[r, 2]) + T[r, 3] for r in range(3)]
        front = q[2] > eps
        z = np.where(q[2] < eps, eps, q[2])
        u = (q[0] / z) * Ko[0, 0] + Ko[0, 2]
        v = (q[1] / z) * Ko[1, 1] + Ko[1, 2]
        wmax, hmax = dt(2) * Ko[0, 2] - dt(1), dt(2) * Ko[1, 2] - dt(1)
        inside = (u >= 0) & (u <= wmax) & (v >= 0) & (v <= hmax)
    return {"proj": np.stack([u, v], 1).astype(dt), "visible": valid & front & inside, "qz": q[2], "wmax": wmax, "hmax": hmax, "front": front}


def project(sc, b, dt=np.float32, n=None, m=None, depths=None):
    """stage A of pair b of a scene (keypoints (x, y)); depths = (d0, valid0, d1, valid1): the precomputed-depth keyword path"""
    n = int(sc["n"][b]) if n is None else n
    m = int(sc["m"][b]) if m is None else m
    kp0, kp1 = sc["kp0"][b, :n], sc["kp1"][b, :m]
    if depths is None:
        d0, v0 = sample_depth(kp0, sc["depth0"][b], dt)
        d1, v1 = sample_depth(kp1, sc["depth1"][b], dt)
    else:
        d0, v0, d1, v1 = depths
    s0 = project_side(kp0, d0, v0, sc["K0"][b], sc["K1"][b], sc["T01"][b], dt)
    s1 = project_side(kp1, d1, v1, sc["K1"][b], sc["K0"][b], sc["T10"][b], dt)
    return {"d0": d0, "d1": d1, "valid0": v0, "valid1": v1, "proj01": s0["proj"], "proj10": s1["proj"], "visible0": s0["visible"],
            "visible1": s1["visible"], "side0": s0, "side1": s1}


def adjugate_inverse(H):
    g = np.asarray(H, np.float64).reshape(9)
    c00, c01, c02 = g[4] * g[8] - g[5] * g[7], g[5] * g[6] - g[3] * g[8], g[3] * g[7] - g[4] * g[6]
    det = g[0] * c00 + g[1] * c01 + g[2] * c02
    return np.array([c00, g[2] * g[7] - g[1] * g[8], g[1] * g[5] - g[2] * g[4], c01, g[0] * g[8] - g[2] * g[6], g[2] * g[3] - g[0] * g[5],
                     c02, g[1] * g[6] - g[0] * g[7], g[0] * g[4] - g[1] * g[3]]).reshape(3, 3) / det


def warp(xy, H, dt=np.float32, inverse=False):
    """H fp32 [3,3]; the inverse comes from the adjugate in float64 and is rounded to `dt`"""
    h = (adjugate_inverse(H) if inverse else np.asarray(H, np.float64)).astype(dt)
    x, y = np.asarray(xy[:, 0], dt), np.asarray(xy[:, 1], dt)
    w = [(x * h[r, 0] + y * h[r, 1]) + h[r, 2] for r in range(3)]
    ww = w[2] + dt(np.float32(1e-5))
    return np.stack([w[0] / ww, w[1] / ww], 1).astype(dt)


# ------------------------------------------------------------------------------------------------ stage B
def dist_matrices(kp0, kp1, p01, p10, vis0=None, vis1=None):
    """float32, unfused: dist0, dist1, dist = max(dist0, dist1) where both are visible, else +inf"""
    f = np.float32
    kp0, kp1, p01, p10 = (np.asarray(a, f) for a in (kp0, kp1, p01, p10))
    with np.errstate(invalid="ignore", over="ignore"):
        ax, ay = p01[:, None, 0] - kp1[None, :, 0], p01[:, None, 1] - kp1[None, :, 1]
        cx, cy = kp0[:, None, 0] - p10[None, :, 0], kp0[:, None, 1] - p10[None, :, 1]
        dist0 = ax * ax + ay * ay
        dist1 = cx * cx + cy * cy
        dist = np.fmax(dist0, dist1)
    if vis0 is not None:
        dist = np.where(vis0[:, None] & vis1[None, :], dist, f(np.inf))
    return dist0, dist1, dist


def _nanmin_strict(a, axis):
    """running minimum with strict <: NaN entries never win (inf when nothing does)"""
    return np.where(np.isnan(a), np.float32(np.inf), a).min(axis)


def label(kp0, kp1, p01, p10, vis0, vis1, valid0, valid1, pos_th, neg_th):
    """one pair, keypoints (x, y) -> (matches0, matches1, pos0); vis / valid None: the homography form"""
    n, m = len(kp0), len(kp1)
    if n == 0 or m == 0:
        return np.full(n, UNMATCHED, np.int64), np.full(m, UNMATCHED, np.int64), np.full(n, -1, np.int64)
    dist0, dist1, dist = dist_matrices(kp0, kp1, p01, p10, vis0, vis1)
    pos_sq, neg_sq = np.float32(pos_th ** 2), np.float32(neg_th ** 2)
    key = np.where(np.isnan(dist), np.float32(np.inf), dist)
    min0, min1 = key.argmin(1), key.argmin(0)  # lowest index on ties; an all-inf row gives 0
    dmin0, dmin1 = key[np.arange(n), min0], key[min1, np.arange(m)]
    pos0 = np.where((min1[min0] == np.arange(n)) & (dmin0 < pos_sq), min0, -1)
    pos1 = np.where((min0[min1] == np.arange(m)) & (dmin1 < pos_sq), min1, -1)
    neg0 = (_nanmin_strict(dist0, 1) > neg_sq) & (True if valid0 is None else valid0)
    neg1 = (_nanmin_strict(dist1, 0) > neg_sq) & (True if valid1 is None else valid1)
    m0 = np.where(neg0, UNMATCHED, np.where(pos0 >= 0, pos0, IGNORE)).astype(np.int64)
    m1 = np.where(neg1, UNMATCHED, np.where(pos1 >= 0, pos1, IGNORE)).astype(np.int64)
    return m0, m1, pos0.astype(np.int64)


def assignment_from_pos0(pos0, m):
    a = np.zeros((len(pos0), m), bool)
    rows = np.nonzero(pos0 >= 0)[0]
    a[rows, pos0[rows]] = True
    return a


def epipolar_all(kp0, kp1, K0, K1, T01, dt=np.float64):
    """sym_epipolar_distance_all with F = K1^-T [t]x R K0^-1 (pinhole K inverted in closed form), eps 1e-15"""
    K0, K1, T = np.asarray(K0, dt), np.asarray(K1, dt), np.asarray(T01, dt)

    def kinv(K):
        return np.array([[1 / K[0, 0], 0, -K[0, 2] / K[0, 0]], [0, 1 / K[1, 1], -K[1, 2] / K[1, 1]], [0, 0, 1]], dt)
    t = T[:3, 3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], dt)
    F = kinv(K1).T @ (tx @ T[:3, :3]) @ kinv(K0)
    p0 = np.concatenate([np.asarray(kp0, dt), np.ones((len(kp0), 1), dt)], 1)
    p1 = np.concatenate([np.asarray(kp1, dt), np.ones((len(kp1), 1), dt)], 1)
    Fp0, Ftp1 = p0 @ F.T, p1 @ F
    e = np.abs(Fp0 @ p1.T)
    d0 = e / np.sqrt(Fp0[:, None, 0] ** 2 + Fp0[:, None, 1] ** 2 + dt(1e-15))
    d1 = e / np.sqrt(Ftp1[None, :, 0] ** 2 + Ftp1[None, :, 1] ** 2 + dt(1e-15))
    return (d0 + d1) / 2


# ------------------------------------------------------------------------------------------------ stage C
def match_pr(m, gt, scores):
    """one pair over all its rows -> [recall, precision, accuracy, average_precision] (float64); NaN without rows"""
    m, gt = np.asarray(m, np.int64), np.asarray(gt, np.int64)
    if len(m) == 0:
        return np.full(4, np.nan)
    eq = m == gt
    c_r, c_a, c_p = (gt > -1).sum(), (gt >= -1).sum(), ((m > -1) & (gt >= -1)).sum()
    recall = (eq & (gt > -1)).sum() / (1e-8 + c_r)
    precision = (eq & (m > -1) & (gt >= -1)).sum() / (1e-8 + c_p)
    accuracy = (eq & (gt >= -1)).sum() / (1e-8 + c_a)
    top = int(np.argmax(np.asarray(scores, np.float32)))  # the lowest index on ties
    r_first = float(eq[top] and gt[top] > -1) / (1e-8 + c_r)
    return np.array([recall, precision, accuracy, precision * (recall - r_first)])


# ------------------------------------------------------------------------------------------------ the fixture's cases
def scene_a(seed):
    """ragged batch: 70 x 90 keypoints on 60 x 80 maps, side 1 on a 48 x 100 map with other intrinsics; pair 1 has one row and a
    motion that puts it behind camera 1 (every row invisible), pair 2 has no row at all"""
    return scene(seed, 3, 70, 90, (60, 80), (48, 100), counts0=(70, 1, 0), counts1=(90, 37, 5), f0=64.0, f1=80.0, behind=(1,))


def scene_b(seed):
    """ordering "xy" and the depth_keypoints* keyword path"""
    return scene(seed + 500, 2, 70, 90, (60, 80), (48, 100), f0=64.0, f1=80.0)


def scene_d(seed):
    """full size: one 1024 x 1023 pair at 260 x 346"""
    return scene(seed + 900, 1, 1024, 1023, (260, 346), (260, 346), f0=256.0, f1=256.0, n_corr=512, n_dup=5)


def precomputed_depths(sc, b):
    """case (b)'s depth_keypoints* / valid_depth_keypoints*: the float64 restatement's samples rounded to float32"""
    n, m = int(sc["n"][b]), int(sc["m"][b])
    d0, v0 = sample_depth(sc["kp0"][b, :n], sc["depth0"][b], np.float64)
    d1, v1 = sample_depth(sc["kp1"][b, :m], sc["depth1"][b], np.float64)
    return d0.astype(np.float32), v0, d1.astype(np.float32), v1


def pr_cases():
    """matcher_metrics inputs {name: (matches0 [B,N] int64, gt_matches0, scores0 float32)}: the top score has a strict gap, so the
    reference's argsort has no choice at the one place its order reaches the result"""
    cases = {}
    for name, seed, B, N in (("mixed", 3, 4, 300), ("full", 4, 2, 1024), ("tiny", 5, 3, 2)):
        gt = ints(seed, (B, N), N + 2) - 2          # -2 .. N-1
        gt[gt >= N // 2] = -1
        m = np.where(ints(seed + 1, (B, N), 3) == 0, ints(seed + 2, (B, N), N // 2 + 1) - 1, gt)  # a third wrong or unmatched
        sc = ints(seed + 3, (B, N), 64).astype(np.float32) / np.float32(128.0)                     # many tied scores below the top
        top = ints(seed + 4, (B,), N)
        sc[np.arange(B), top] = 0.75
        m[0, top[0]] = gt[0, top[0]] = 7  # a true positive at the top of pair 0: r_first != 0
        cases[name] = (m.astype(np.int64), gt.astype(np.int64), sc)
    B, N = 2, 50
    gt = np.full((B, N), -2, np.int64)
    m = ints(9, (B, N), 12) - 2
    sc = ints(10, (B, N), 64).astype(np.float32) / np.float32(128.0)
    sc[:, 3] = 0.75
    cases["all_ignored"] = (m.astype(np.int64), gt, sc)                                           # all gt < -1
    gt = ints(11, (B, N), 12) - 2
    cases["no_prediction"] = (np.full((B, N), -1, np.int64), gt.astype(np.int64), sc.copy())     # no predicted match
    return cases


# ------------------------------------------------------------------------------------------------ reading the fixture
POSE_CASES = {"a": scene_a, "b": scene_b, "d": scene_d}


def fixture_pair(G, tag, n, m):
    """the reference's outputs of one pair as stored by gen_gt_matches.py (None for a pair that took the early return)"""
    if f"{tag}.matches0" not in G:
        return None
    r = {k: G[f"{tag}.{k}"] for k in ("proj_0to1", "proj_1to0", "depth_keypoints0", "depth_keypoints1", "visible0", "visible1", "reward_unsure")
         if f"{tag}.{k}" in G}
    r["matches0"], r["matches1"] = G[f"{tag}.matches0"].astype(np.int64), G[f"{tag}.matches1"].astype(np.int64)
    r["assignment"] = np.unpackbits(G[f"{tag}.assignment"])[:n * m].reshape(n, m).astype(bool)
    r["reward"] = G[f"{tag}.reward"].astype(np.float32).reshape(n, m)
    return r


def reward_pose(kp0, kp1, p01, p10, vis0, vis1, K0, K1, T01, pos_th, neg_th):
    """the dense `reward` of the pose form from float32 inputs (epi_dist in float64: its threshold margins are in the fixture)"""
    _, _, dist = dist_matrices(kp0, kp1, p01, p10, vis0, vis1)
    epi = epipolar_all(kp0, kp1, K0, K1, T01)
    return (dist < np.float32(pos_th ** 2)).astype(np.float32) - (epi > neg_th).astype(np.float32)


def reward_homography(kp0, kp1, p01, p10, pos_th, neg_th):
    _, _, dist = dist_matrices(kp0, kp1, p01, p10)
    return (dist < np.float32(pos_th ** 2)).astype(np.float32) - (dist > np.float32(neg_th ** 2)).astype(np.float32)
