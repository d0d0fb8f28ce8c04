"""Fixed inputs of the RANSAC contract tests (test_ransac_contract_cpu.py, test_pose_contract_gpu.py,
test_homography_contract_gpu.py): the CPU file establishes on the float64 restatements what the GPU files rely on, and both read
the cases from here, so that both see the same bytes.  Not collected by pytest (no test_ prefix)."""
from functools import lru_cache

import numpy as np

import homography_f64 as Hm
import pose_f64 as P


# ------------------------------------------------------------------ pose scenes with two different cameras
def scene2(rng, n, noise=0.0, outliers=0.0, kdt=np.float32, W=346, H=260, max_deg=15.0):
    """pose_f64.scene with distinct intrinsics: camera 0 has f ~ 226, camera 1 f ~ 310, fx != fy in each and all of fx, fy, cx, cy
    differ between the two.  Image 0 is projected through K0, image 1 through K1 (the matrices as stored, in float64).  kdt
    float64: no entry of fx, fy, cx, cy is representable in float32, so that the promotion of the float32 keypoints matters.
    -> (kp0, kp1, K0, K1, T_0to1 [4,4] float32), keypoints float32 in (y, x, score)"""
    def intrinsics(f, dcx, dcy):
        K = np.array([[f + rng.uniform(2, 6), 0, W / 2 + dcx + rng.uniform(-3, 3)],
                      [0, f - rng.uniform(2, 6), H / 2 + dcy + rng.uniform(-3, 3)], [0, 0, 1]], np.float64)
        K = K.astype(kdt)
        if kdt == np.float64:
            assert all(float(np.float32(v)) != v for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
        return K

    K0, K1 = intrinsics(226.0, -8.0, 5.0), intrinsics(310.0, 9.0, -7.0)
    R = P.rotation(rng.normal(size=3), rng.uniform(1.0, max_deg))
    t = rng.normal(size=3)
    t = t / np.linalg.norm(t) * rng.uniform(0.3, 1.0)
    K0d, K1d = K0.astype(np.float64), K1.astype(np.float64)
    pts0, pts1 = [], []
    while len(pts0) < n:
        u, v, z = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(2, 10)
        X1 = R @ (np.linalg.solve(K0d, np.array([u, v, 1.0])) * z) + t
        if X1[2] <= 0.5:
            continue
        p = K1d @ (X1 / X1[2])
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
    return kp0, kp1, K0, K1, T


# the certificate of a pose (sample_residual): the largest residual of the restatement's own (R, t) over every pose input, as
# test_ransac_contract_cpu.py::test_certificate_bound prints it; the device is held to 10 x that, under a ceiling of 1e-6
CERT_WORST = 3.6e-14  # measured: case 1 (n = 257, noise free, 30 % outliers) 3.58e-14
CERT_GATE = 10 * CERT_WORST
CERT_CEILING = 1e-6
HE_THR = (3, 5, 10)
HE_ERR_GATE = 0.0  # test_homography_gpu.py's ERR_GATE: both sides round H to the same float32

F32, F64 = np.float32, np.float64
IT300 = {"max_iters": 300}
# (scene seed, n, noise px, outlier fraction, K's dtype, keyword arguments of relative_pose); every scene is scene2, K0 != K1
# The scene seeds are ones at which the restatement alone meets test_ransac_contract_cpu.py's rules (decisive, within the
# ground-truth bound, off by more than 10 degrees with the cameras swapped).
POSE_CASES = [
    (101, 60, 0.0, 0.0, F32, IT300),                                  # 0  float32 K0 != K1, noise free
    (102, 257, 0.0, 0.3, F32, IT300),                                 # 1  one point past the score kernel's 256-point trip
    (103, 513, 0.0, 0.3, F32, IT300),                                 # 2  one point past two trips
    (104, 60, 0.0, 0.0, F64, IT300),                                  # 3  float64 K: norm_pair<double>
    (446, 60, 0.5, 0.3, F64, IT300),                                  # 4  float64 K with outliers
    (106, 60, 0.1, 0.2, F32, {"thresh": 0.25, "max_iters": 300}),     # 5
    (107, 60, 0.5, 0.2, F32, {"thresh": 2.0, "max_iters": 300}),      # 6
    (473, 60, 0.5, 0.3, F32, {"conf": 0.5, "max_iters": 300}),        # 7
    (109, 60, 0.5, 0.3, F32, {"conf": 0.99, "max_iters": 300}),       # 8
    (110, 60, 0.5, 0.3, F32, {"seed": 0xC0FFEE, "max_iters": 300}),   # 9
    (111, 40, 0.0, 0.0, F32, {"max_iters": 1}),                       # 10 one iteration: the first round ends after it
    (516, 40, 0.5, 0.3, F32, {"max_iters": 33}),                      # 11 one iteration past the first round
    (524, 40, 0.5, 0.3, F32, {"max_iters": 65}),                      # 12 one iteration past the second round
    (531, 5, 0.0, 0.0, F32, IT300),                                   # 13 n = 5: every solution of the one sample
    (541, 6, 0.0, 0.0, F32, IT300),                                   # 14 n = 6
    (116, 60, 0.5, 0.5, F32, {}),                                     # 15 the default max_iters = 1000
]
POSE_STATUS = {}  # case index -> the restatement's failure status where it is not "ok" (none)
POSE_OUTLIER_BOUND = {0.0: "noise_free", 0.2: "outliers_30", 0.3: "outliers_30", 0.5: "outliers_60"}  # pose_f64.GT_BOUNDS keys


def pose_case(i):
    seed, n, noise, outliers, kdt, kw = POSE_CASES[i]
    return scene2(np.random.default_rng(seed), n, noise=noise, outliers=outliers, kdt=kdt), dict(kw)


@lru_cache(maxsize=None)
def pose_ref(i):
    """(pair, kwargs, the restatement's result) of POSE_CASES[i]; computed once per process, read only"""
    p, kw = pose_case(i)
    return p, kw, P.relative_pose(*p[:4], **kw)


def pose_points(pair):
    """the normalised (x, y) points of both images of a (y, x, score) pair, as the estimator sees them"""
    a0, a1, K0, K1 = pair[:4]
    return P.normalize(a0[:, 1::-1], K0), P.normalize(a1[:, 1::-1], K1)


def sample_residual(pair, R, t, it, seed=P.DEFAULT_SEED):
    """the certificate of a pose: E' = [t]x R at unit Frobenius norm must vanish on the five matches that RANSAC iteration `it`
    drew, whichever solver route found it -> max |x2' E' x1| over the sample"""
    x1, x2 = pose_points(pair)
    E = P.skew(np.asarray(t)) @ np.asarray(R)
    E = E / np.linalg.norm(E)
    idx = P.draw(seed, it, len(x1))
    assert idx is not None
    h1, h2 = np.c_[x1[idx], np.ones(5)], np.c_[x2[idx], np.ones(5)]
    return float(np.abs(np.einsum("ni,ij,nj->n", h2, E, h1)).max())


# (scene seed, n, noise px, outlier fraction, keyword arguments of homography); scenes of homography_f64.scene
HOMOGRAPHY_CASES = [
    (201, 60, 0.3, 0.3, {"thresh": 1.0, "max_iters": 300}),           # 0
    (202, 60, 0.5, 0.3, {"thresh": 6.0, "max_iters": 300}),           # 1
    (203, 60, 0.5, 0.4, {"conf": 0.5, "max_iters": 300}),             # 2
    (204, 60, 0.5, 0.4, {"seed": 0xC0FFEE, "max_iters": 300}),        # 3
    (205, 40, 0.0, 0.0, {"max_iters": 1}),                            # 4
    (206, 40, 0.5, 0.5, {"max_iters": 33}),                           # 5
    (207, 40, 0.5, 0.5, {"max_iters": 65}),                           # 6
    (208, 4, 0.0, 0.0, {"max_iters": 300}),                           # 7  n = 4: the one sample
    (209, 5, 0.0, 0.0, {"max_iters": 300}),                           # 8
    (210, 257, 0.5, 0.3, {"max_iters": 300}),                         # 9  one point past the score kernel's 256-point trip
    (211, 513, 0.5, 0.3, {"max_iters": 300}),                         # 10 one point past two trips
]
HOMOGRAPHY_STATUS = {}  # case index -> the restatement's failure status where it is not "ok" (none)


def homography_case(i):
    seed, n, noise, outliers, kw = HOMOGRAPHY_CASES[i]
    return Hm.scene(np.random.default_rng(seed), n, noise=noise, outliers=outliers), dict(kw)


@lru_cache(maxsize=None)
def homography_ref(i):
    """(pair, kwargs, the restatement's result) of HOMOGRAPHY_CASES[i]; computed once per process, read only"""
    p, kw = homography_case(i)
    return p, kw, Hm.homography(p[0], p[1], **kw)


# ------------------------------------------------------------------ batches over 64 pairs
# eleven small pairs tiled over B = 130 slots (slot b holds entry b % 11), cap 64, max_iters 300: slots 63, 64, 65 hold entries
# 8, 9 ("few"), 10 and slots 127, 128, 129 entries 6, 7 (a failure status), 8
TILE_B, TILE_CAP, TILE_KW = 130, 64, {"max_iters": 300}
TILE_SPEC = [(8, 0.0, 0.0), (60, 0.5, 0.3), (24, 0.3, 0.5), (5, 0.0, 0.0), (33, 0.5, 0.2), (64, 0.0, 0.0), (12, 0.2, 0.25),
             "same", (48, 1.0, 0.4), "few", (6, 0.0, 0.0)]  # (n, noise, outliers) | every point identical | three matches


TILE_SEEDS = {"pose": [3000, 3100, 3200, 3300, 3400, 3500, 3600, 3700, 3800, 3900, 4000],  # one scene seed per entry
              "homography": [5000, 5001, 5002, 5003, 5004, 5005, 5006, 5007, 5108, 5009, 5010]}


def tile_pairs(kind):
    """the eleven pairs of the B = 130 tiling: kind "pose" -> (kp0, kp1, K0, K1, T) float32 K0 != K1, "homography" ->
    (kp0, kp1, H_true)"""
    pairs = []
    for spec, seed in zip(TILE_SPEC, TILE_SEEDS[kind]):
        rng = np.random.default_rng(seed)
        n, nz, o = (40, 0.0, 0.0) if isinstance(spec, str) else spec
        p = scene2(rng, n, noise=nz, outliers=o) if kind == "pose" else Hm.scene(rng, n, noise=nz, outliers=o)
        if spec == "same":
            same = np.repeat(p[0][:1], 40, 0)
            p = (same, same.copy()) + tuple(p[2:])
        elif spec == "few":
            p = (p[0][:3], p[1][:3]) + tuple(p[2:])
        pairs.append(p)
    return pairs


# ------------------------------------------------------------------ round boundaries
# The host enqueues iterations in rounds [0, 32), [32, 64), [64, 128), [128, 256)...; the scan resumes from the previous round's
# state.  Per estimator small scenes of n = 24 with 0.3 px noise and 60-70 % outliers under max_iters = 300 (one for the
# homography, two for the pose), and for each of the first and last iterations of a round a RANSAC seed at which the
# restatement's chosen iteration is exactly that one (found by search_boundary_seeds, verified by test_ransac_contract_cpu.py).
BOUNDARY_ITERS = (31, 32, 63, 64, 127, 128)
BOUNDARY_KW = {"max_iters": 300}
BOUNDARY_SCENES = {"pose": lambda s: P.scene(np.random.default_rng(s), 24, noise=0.3, outliers=0.6),
                   "homography": lambda s: Hm.scene(np.random.default_rng(s), 24, noise=0.3, outliers=0.7)}
BOUNDARY_SEEDS = {  # estimator -> [(scene seed, chosen iteration, RANSAC seed)]
    "pose": [(79, 31, 32), (77, 32, 60), (79, 63, 257), (77, 64, 196), (77, 127, 383), (79, 128, 74)],
    "homography": [(78, 31, 13), (78, 32, 515), (78, 63, 440), (78, 64, 79), (78, 127, 194), (78, 128, 600)],
}


@lru_cache(maxsize=None)
def boundary_ref(kind, scene_seed, seed):
    """(pair, restatement's result) of the boundary scene under RANSAC seed `seed`"""
    p = BOUNDARY_SCENES[kind](scene_seed)
    r = P.relative_pose(*p[:4], seed=seed, **BOUNDARY_KW) if kind == "pose" else Hm.homography(p[0], p[1], seed=seed, **BOUNDARY_KW)
    return p, r


def chosen_iteration(kind, scene_seed, seed):
    """the restatement's chosen iteration of the boundary scene under RANSAC seed `seed`, None without a model"""
    r = boundary_ref(kind, scene_seed, seed)[1]
    if r["status"] != "ok":
        return None
    return r["it"][0] if kind == "pose" else r["it"]


def search_boundary_seeds(kind, scene_seed, wanted=BOUNDARY_ITERS, seeds=range(1, 2000)):
    """the search that produced BOUNDARY_SEEDS: RANSAC seeds upward until every wanted iteration has one -> {iteration: seed}"""
    found = {}
    for s in seeds:
        it = chosen_iteration(kind, scene_seed, s)
        if it in wanted and it not in found:
            found[it] = s
            if len(found) == len(wanted):
                break
    return found
