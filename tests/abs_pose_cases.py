"""Fixed inputs of the absolute-pose tests (test_abs_pose_cpu.py, test_abs_pose_gpu.py): the CPU file establishes on the float64
restatement tests/abs_pose_f64.py what the GPU file relies on, and both read the cases from here, so that both see the same bytes.
Not collected by pytest (no test_ prefix)."""
from functools import lru_cache

import numpy as np

import abs_pose_f64 as A
from pose_f64 import rotation

CAP = 520
KW = {}  # the batch runs under the defaults: thresh 8, conf 0.99, max_iters 100
# (scene seed, n, noise px, outlier fraction) of abs_pose_f64.scene with exact per-match depths, or a named special pair
PAIRS = [
    (700, 0, 0.0, 0.0),      # 0  no match
    (701, 3, 0.0, 0.0),      # 1  three matches: "few"
    (702, 4, 0.0, 0.0),      # 2  the smallest pair with a pose
    (703, 5, 0.0, 0.0),      # 3
    (704, 64, 0.0, 0.0),     # 4  one wave of points, noise free
    (705, 65, 0.5, 0.3),     # 5  one point past a wave
    (706, 257, 0.0, 0.3),    # 6  one point past the score kernel's 256-point trip
    (707, 513, 0.5, 0.3),    # 7  one point past two trips
    (708, 64, 1.0, 0.6),     # 8
    (709, 257, 1.0, 0.5),    # 9
    (710, 65, 0.2, 0.2),     # 10
    (711, 513, 0.0, 0.0),    # 11
    "collinear",             # 12 every 3-D point on one line: no sample has a model
    "identical",             # 13 one match forty times
    "holes",                 # 14 no match has a valid depth
    "four_of_40",            # 15 exactly 4 usable matches of 40
    (716, 64, 0.5, 0.5),     # 16
    (717, 5, 0.3, 0.2),      # 17 one outlier of five
]
SPECIAL_SEED = {"collinear": 712, "identical": 713, "holes": 714, "four_of_40": 715}
STATUS = {0: "few", 1: "few", 12: "none", 13: "none", 14: "few"}  # the restatement's status where it is not "ok"

# ---- what test_abs_pose_cpu.py measures on the restatement and prints; the GPU gates derive from them
GT_BOUND = {"R_err": 0.5, "t_err": 0.05}  # degrees, depth units: cases with n >= 50, <= 50 % outliers, <= 0.5 px noise, exact depth
GT_WORST = {"R_err": 0.0849, "t_err": 0.00526}  # the restatement's worst: pair 16 (64 matches, 0.5 px, 50 % outliers), pair 5
P3P_WORST = 2.01e-9       # worst reprojection (unit-bearing distance) of a returned pose over the 24 problems: problem 19, four poses
P3P_CEILING = 1e-6
REFIT_FLOOR = 8.3e-10     # largest change of an entry of R or t (t relative to max(1, |t|)) with the LM sums taken in reverse order
CLEAN_WORST = 3.0e-7     # the restatement's own distance from the true pose on the noise-free, outlier-free cases (same measure)


def _special(kind):
    rng = np.random.default_rng(SPECIAL_SEED[kind])
    s = A.scene(rng, 40, noise=0.0, outliers=0.0)
    if kind == "collinear":
        # y = cy0 and one depth: X = d ((x - cx) / fx, 0, 1), the differences of two points have one non-zero component
        K0 = s["K0"].astype(np.float64)
        s["kp0"][:, 0] = s["K0"][1, 2]
        s["d0"][:] = np.float32(4.0)
        R, t = s["T"][:3, :3], s["T"][:3, 3]
        x = s["kp0"][:, 1].astype(np.float64)
        X = np.stack([4.0 * (x - K0[0, 2]) / K0[0, 0], np.zeros(40), np.full(40, 4.0)], 1) @ R.T + t
        p = X[:, :2] / X[:, 2:] * np.array([s["K1"][0, 0], s["K1"][1, 1]], np.float64) + np.array([s["K1"][0, 2], s["K1"][1, 2]], np.float64)
        s["kp1"][:, 1], s["kp1"][:, 0] = p[:, 0], p[:, 1]
    elif kind == "identical":
        for k in ("kp0", "kp1", "d0"):
            s[k] = np.repeat(s[k][:1], 40, 0)
    elif kind == "holes":
        s["d0"][:] = -1.0
        s["valid0"][:] = 0
    elif kind == "four_of_40":
        s["valid0"][:] = 0
        s["valid0"][[3, 11, 26, 38]] = 1
        s["d0"][s["valid0"] == 0] = np.nan
    return s


@lru_cache(maxsize=None)
def pair(i):
    """the scene dict of PAIRS[i] (read only)"""
    spec = PAIRS[i]
    if isinstance(spec, str):
        return _special(spec)
    seed, n, noise, outliers = spec
    return A.scene(np.random.default_rng(seed), n, noise=noise, outliers=outliers)


def run(s, **kw):
    """the restatement on a scene dict"""
    depth = {"depth0": s["depth0"]} if "depth0" in s else {"d0": s["d0"], "valid0": s["valid0"]}
    return A.absolute_pose(s["kp0"], s["kp1"], s["K0"], s["K1"], T_0to1=s["T"], **depth, **kw)


@lru_cache(maxsize=None)
def ref(i, refine=True, max_iters=100):
    """the restatement's result of PAIRS[i]; computed once per process, read only"""
    return run(pair(i), refine=refine, max_iters=max_iters, **KW)


def gt_case(i):
    spec = PAIRS[i]
    return not isinstance(spec, str) and spec[1] >= 50 and spec[3] <= 0.5 and spec[2] <= 0.5


def clean_case(i):
    spec = PAIRS[i]
    return not isinstance(spec, str) and spec[1] >= 4 and spec[2] == 0.0 and spec[3] == 0.0


def pose_distance(R, t, R2, t2):
    """largest entry of |R - R2| and of |t - t2| / max(1, |t2|_inf)"""
    return max(float(np.abs(R - R2).max()), float(np.abs(t - t2).max() / max(1.0, np.abs(t2).max())))


# ---- the lift: small depth maps with holes
LIFT_KW = {"thresh": 1.0}
LIFT_PAIRS = [(750, 64, 0.0, 0.0), (751, 90, 0.2, 0.3), (752, 33, 0.0, 0.2), "all_holes"]
LIFT_HW = (40, 48)


@lru_cache(maxsize=None)
def lift_pair(i):
    spec = LIFT_PAIRS[i]
    if spec == "all_holes":
        s = dict(A.scene(np.random.default_rng(753), 40, W=LIFT_HW[1], H=LIFT_HW[0], holes=0.2))
        s["depth0"] = np.full(LIFT_HW, -1.0, np.float32)
        return s
    seed, n, noise, outliers = spec
    return A.scene(np.random.default_rng(seed), n, noise=noise, outliers=outliers, W=LIFT_HW[1], H=LIFT_HW[0], holes=0.2)


@lru_cache(maxsize=None)
def lift_ref(i):
    return run(lift_pair(i), **LIFT_KW)


# ---- P3P problems
def p3p_problems(n=24, seed=760):
    """(X [n,3,3], f [n,3,3], R [n,3,3], t [n,3]): three points 3-10 in front of view 1 under a random pose"""
    rng = np.random.default_rng(seed)
    Xs, fs, Rs, ts = [], [], [], []
    for _ in range(n):
        R = rotation(rng.normal(size=3), rng.uniform(1, 40))
        t = rng.normal(size=3) * 0.5
        Q = np.stack([rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3), rng.uniform(3, 10, 3)], 1)
        Xs.append((Q - t) @ R)
        fs.append(Q / np.linalg.norm(Q, axis=1)[:, None])
        Rs.append(R)
        ts.append(t)
    return np.array(Xs), np.array(fs), np.array(Rs), np.array(ts)


def p3p_residual(X, f, R, t):
    """the certificate of a pose of a three-point problem: the largest distance between a unit bearing and the direction of its
    transformed point, which must lie in front"""
    Y = X @ R.T + t
    d = np.linalg.norm(Y, axis=1)
    return float(np.abs(Y / d[:, None] - f).max())


# ---- batches over 64 pairs and round boundaries
TILE_B, TILE_CAP, TILE_KW = 130, 64, {"max_iters": 33}
TILE = [0, 1, 2, 3, 4, 8, 12, 13, 14, 15, 16, 17]  # slot b holds PAIRS[TILE[b % 12]]: slots 63, 64, 65 -> 3, 4, 8; 127, 128, 129 -> 13, 14, 15

BOUNDARY_ITERS = (31, 32, 63, 64)
BOUNDARY_KW = {"max_iters": 300, "thresh": 2.0}
BOUNDARY_SCENE = (770, 24, 0.3, 0.65)
BOUNDARY_SEEDS = {31: 9, 32: 123, 63: 71, 64: 87}  # chosen iteration -> RANSAC seed (search_boundary_seeds; verified by test_abs_pose_cpu.py)


@lru_cache(maxsize=None)
def boundary_pair():
    seed, n, noise, outliers = BOUNDARY_SCENE
    return A.scene(np.random.default_rng(seed), n, noise=noise, outliers=outliers)


@lru_cache(maxsize=None)
def boundary_ref(seed):
    return run(boundary_pair(), seed=seed, **BOUNDARY_KW)


def search_boundary_seeds(wanted=BOUNDARY_ITERS, seeds=range(1, 4000)):
    """the search that produced BOUNDARY_SEEDS: RANSAC seeds upward until every wanted iteration has one"""
    found = {}
    for s in seeds:
        r = boundary_ref(s)
        it = r["it"][0] if r["status"] == "ok" else None
        if it in wanted and it not in found:
            found[it] = s
            if len(found) == len(wanted):
                break
    return found
