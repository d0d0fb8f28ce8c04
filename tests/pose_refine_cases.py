"""Fixed inputs of the pose-refinement tests (test_pose_refine_cpu.py, test_pose_refine_gpu.py): the CPU file establishes on the
float64 restatement tests/pose_refine_f64.py what the GPU file relies on, and both read the cases from here, so that both see
the same bytes.  Not collected by pytest (no test_ prefix).

A case is a scene of tests/pose_f64.py (or a special pair) with an initial pose: the true pose perturbed by a fixed rotation and
a tilt of t of the same size, or the result of pose_f64.relative_pose on it, computed once (make_golden) and kept in
tests/golden/pose_refine_init.npz, so that no test spends minutes in the numpy RANSAC."""
import os
from functools import lru_cache

import numpy as np

import pose_f64 as P
import pose_refine_f64 as RF

CAP = 1024
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_refine_init.npz")

# name: (scene seed, n, noise px, outlier fraction, initial pose: degrees of perturbation or "ransac", options)
# options: k64 (float64 intrinsics), cams (a different second camera), forward (P.FORWARD), thresh, rounds, lm_iters
CASES = {
    "n5": (900, 5, 0.0, 0.0, 0.5, {}),                      # five matches: the first set has fewer than 6 members
    "n6_clean": (901, 6, 0.0, 0.0, 0.5, {}),                # the smallest set a round runs on
    "n8_clean": (902, 8, 0.0, 0.0, 0.5, {"k64": True}),
    "n64_clean": (903, 64, 0.0, 0.0, 0.5, {}),              # one wave of matches
    "n255": (904, 255, 0.5, 0.3, 1.0, {"thresh": 3.0}),     # one short of the workgroup; a pose 1 degree off needs a wider threshold
    "n256": (905, 256, 1.0, 0.5, 0.3, {"cams": True}),      # every thread one match
    "n257": (906, 257, 0.5, 0.0, 2.0, {"thresh": 6.0}),     # one thread two matches; 2 degrees off
    "n513_k64": (907, 513, 1.0, 0.3, 1.0, {"k64": True, "cams": True}),
    "n1024": (908, 1024, 0.5, 0.5, 0.5, {}),                # the whole capacity
    "n1024_clean": (909, 1024, 0.0, 0.0, 0.5, {"k64": True}),
    "n64_cams": (910, 64, 1.0, 0.3, 1.0, {"cams": True}),
    "forward": (911, 257, 0.5, 0.3, 0.5, {"forward": True}),
    "rounds4": (912, 255, 1.0, 0.3, 2.0, {"rounds": 4, "lm_iters": 3}),
    "rounds1": (913, 64, 0.5, 0.3, 1.0, {"rounds": 1, "lm_iters": 50}),
    "ransac_64": (920, 64, 0.5, 0.3, "ransac", {}),
    "ransac_255": (921, 255, 1.0, 0.5, "ransac", {}),
    "ransac_257_forward": (922, 257, 0.5, 0.3, "ransac", {"forward": True}),
    "ransac_513": (923, 513, 1.0, 0.3, "ransac", {"cams": True}),
    "ransac_64_clean": (924, 64, 0.0, 0.0, "ransac", {}),
    "few_inliers": (930, 64, 0.5, 0.0, 35.0, {}),           # an initial pose 35 degrees off: fewer than 6 Sampson inliers
    "rejected": (931, 64, 1.0, 0.3, 0.3, {"thresh": 0.75}),  # at this threshold the refined pose has 23 inliers, the input 26: keep rule
}
# special pairs: compared with nothing but themselves (finite or passed through)
DEGENERATE = ("pure_rotation", "identical", "collinear")
DEGENERATE_SEED = {"pure_rotation": 940, "identical": 941, "collinear": 942}
DEGENERATE_DEG = 0.05  # their initial pose: the true one this far off, close enough for a first set of all matches
NEGATIVE = "n64_clean"  # the scene that also goes in with status_in = -2

# ---- what test_pose_refine_cpu.py measures on the restatement and prints; the GPU gates derive from them
# REFINE_FLOOR: the largest change of an entry of R or t (pose_distance) between forward and reversed summation, over the cases
# and over FLOOR_CAMPAIGN.  Where LM has converged, a trial's cost differs from the current one by rounding alone, and whether the
# last step is accepted depends on the order of the sums; the pose then moves by that step.  That happens in about one pair of
# twenty (campaign seeds 976 and 983: 3.6e-9 and 4.2e-9; every other pair stays below 3e-14), and the cases alone happen to hold
# no such pair -- the device, which sums in a third order, meets them at the same rate, so the floor is taken over the campaign too.
REFINE_FLOOR = 4.3e-9
FLOOR_CAMPAIGN = range(950, 990)  # scene seeds: n of (64, 255, 257, 513), noise of (0.5, 1), outliers of (0, 0.3, 0.5), 0.3 degrees off
CLEAN_WORST = 2.6e-6    # the restatement's own distance from the true pose on the noise-free, outlier-free cases: n6_clean
NOT_KEPT = {"n5", "few_inliers", "rejected"}  # the cases whose input pose comes back (kept = 0): the other 18 keep their refinement


def _perturb(T, deg, seed):
    """the true pose turned by `deg` degrees about a fixed axis, its t tilted by `deg` degrees and normalised"""
    rng = np.random.default_rng(seed + 5000)
    U, _, Vt = np.linalg.svd(T[:3, :3].astype(np.float64))  # the float32 entries of T are 1e-8 off a rotation
    R = P.rotation(rng.normal(size=3), deg) @ (U @ Vt)
    t = T[:3, 3].astype(np.float64)
    if not np.linalg.norm(t) > 0:
        t = np.array([1.0, 0.0, 0.0])
    t = P.rotation(rng.normal(size=3), deg) @ (t / np.linalg.norm(t))
    return R, t / np.linalg.norm(t)


def _second_camera(kp1, K1):
    """view 1 through another camera: the pixels of the same rays under K1' (float32, like the extractor's keypoints)"""
    K2 = K1.copy()
    K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2] = K1[0, 0] * 1.31, K1[1, 1] * 1.27, K1[0, 2] + 11.5, K1[1, 2] - 7.25
    out = kp1.copy()
    out[:, 1] = (kp1[:, 1].astype(np.float64) - K1[0, 2]) / K1[0, 0] * K2[0, 0] + K2[0, 2]  # x, the second column of (y, x, score)
    out[:, 0] = (kp1[:, 0].astype(np.float64) - K1[1, 2]) / K1[1, 1] * K2[1, 1] + K2[1, 2]
    return out.astype(np.float32), K2


@lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@lru_cache(maxsize=None)
def scene(name):
    """dict(kp0, kp1 [n,3] float32 (y, x, score), K0, K1, T [4,4] float32) of a case (read only)"""
    if name in DEGENERATE:
        return _degenerate(name)
    seed, n, noise, outliers, _, opt = CASES[name]
    kp0, kp1, K0, K1, T = P.scene(np.random.default_rng(seed), n, noise=noise, outliers=outliers, t_dir=P.FORWARD if opt.get("forward") else None)
    if opt.get("cams"):
        kp1, K1 = _second_camera(kp1, K1)
    if opt.get("k64"):
        K0, K1 = K0.astype(np.float64), K1.astype(np.float64)
    return {"kp0": kp0, "kp1": kp1, "K0": K0, "K1": K1, "T": T}


def _degenerate(kind):
    rng = np.random.default_rng(DEGENERATE_SEED[kind])
    kp0, kp1, K0, K1, T = P.scene(rng, 40, noise=0.0, outliers=0.0)
    Kd = K0.astype(np.float64)
    if kind == "pure_rotation":  # t_gt = 0: view 1 is the homography K R K^-1 of view 0; every t explains it
        T = T.copy()
        T[:3, 3] = 0.0
        h = np.column_stack([kp0[:, 1], kp0[:, 0], np.ones(40)]).astype(np.float64) @ (Kd @ T[:3, :3].astype(np.float64) @ np.linalg.inv(Kd)).T
        kp1 = kp1.copy()
        kp1[:, 1], kp1[:, 0] = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2]
    elif kind == "identical":  # one match forty times
        kp0, kp1 = np.repeat(kp0[:1], 40, 0), np.repeat(kp1[:1], 40, 0)
    elif kind == "collinear":  # both views' points on the image row through the principal point
        kp0, kp1 = kp0.copy(), kp1.copy()
        kp0[:, 0], kp1[:, 0] = K0[1, 2], K1[1, 2]
    return {"kp0": kp0, "kp1": kp1, "K0": K0, "K1": K1, "T": T}


def kwargs(name):
    opt = CASES[name][5] if name in CASES else {}
    return {"thresh": opt.get("thresh", 1.0), "rounds": opt.get("rounds", 2), "lm_iters": opt.get("lm_iters", 10)}


@lru_cache(maxsize=None)
def initial(name):
    """(R [3,3], t [3], mask [n] bool, status) the refinement starts from"""
    s = scene(name)
    n = len(s["kp0"])
    init = CASES[name][4] if name in CASES else DEGENERATE_DEG
    if init == "ransac":
        g = _golden()
        return g[name + "_R"], g[name + "_t"], g[name + "_mask"].astype(bool), int(g[name + "_status"])
    seed = CASES[name][0] if name in CASES else DEGENERATE_SEED[name]
    R, t = _perturb(s["T"], init, seed)
    mask = np.zeros(n, bool)
    mask[::2] = True  # not a mask of this pose: what comes back when the input pose does
    return R, t, mask, 0


def run(name, reverse=False, trace=None, status=None, with_T=True):
    """the restatement on a case"""
    s = scene(name)
    R, t, mask, st = initial(name)
    return RF.refine(s["kp0"], s["kp1"], s["K0"], s["K1"], R, t, mask, st if status is None else status, s["T"] if with_T else None,
                     ordering="yx", reverse=reverse, trace=trace, **kwargs(name))


@lru_cache(maxsize=None)
def ref(name):
    """the restatement's result of a case; computed once per process, read only"""
    return run(name)


def campaign_floor(seed):
    """the restatement's forward-against-reverse distance on one pair of FLOOR_CAMPAIGN, with the two accepted-step counts"""
    n = (64, 255, 257, 513)[seed % 4]
    kp0, kp1, K0, K1, T = P.scene(np.random.default_rng(seed), n, noise=(0.5, 1.0)[seed % 2], outliers=(0.0, 0.3, 0.5)[seed % 3])
    R, t = _perturb(T, 0.3, seed)
    a, b = (RF.refine(kp0, kp1, K0, K1, R, t, np.zeros(n, bool), 0, T, reverse=rev) for rev in (False, True))
    assert a["info"][:2] == b["info"][:2] and a["info"][3] == b["info"][3]
    return pose_distance(a["R"], a["t"], b["R"], b["t"]), a["info"][2], b["info"][2]


def clean_case(name):
    return name in CASES and CASES[name][2] == 0.0 and CASES[name][3] == 0.0 and CASES[name][1] >= 6 and CASES[name][4] != "ransac"


def noisy_case(name):
    """the cases of the improvement check: noise, at least 64 matches, the default threshold"""
    return name in CASES and CASES[name][2] > 0.0 and CASES[name][1] >= 64 and name not in ("few_inliers", "rejected")


def pose_err_before(name):
    s = scene(name)
    R, t, _, _ = initial(name)
    return P.pose_errors(s["T"], R, t)[2]


def pose_distance(R, t, R2, t2):
    """abs_pose_cases.pose_distance's measure: the largest entry of |R - R2| and of |t - t2| / max(1, |t2|_inf)"""
    return max(float(np.abs(R - R2).max()), float(np.abs(t - t2).max() / max(1.0, np.abs(t2).max())))


def truth(name):
    T = scene(name)["T"].astype(np.float64)
    t = T[:3, 3]
    return T[:3, :3], t / np.linalg.norm(t)


def make_golden():
    """the stored initial poses: pose_f64.relative_pose on each "ransac" case (minutes of numpy RANSAC, run once)"""
    out = {}
    for name, spec in CASES.items():
        if spec[4] != "ransac":
            continue
        s = scene(name)
        r = P.relative_pose(s["kp0"], s["kp1"], s["K0"], s["K1"], thresh=1.0, ordering="yx")
        assert r["status"] == "ok", (name, r["status"])
        out[name + "_R"], out[name + "_t"], out[name + "_mask"] = r["R"], r["t"], r["mask"].astype(np.uint8)
        out[name + "_status"] = np.int32(16 * r["it"][0] + r["it"][1])
        print(name, r["it"], int(r["mask"].sum()), P.pose_errors(s["T"], r["R"], r["t"]))
    np.savez(GOLDEN, **out)


if __name__ == "__main__":
    make_golden()
