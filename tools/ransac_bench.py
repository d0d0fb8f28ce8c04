#!/usr/bin/env python3
"""Device time of a batched RANSAC estimator, the relative pose (csrc/pose.hip), the homography (csrc/homography.hip) or the absolute
pose (csrc/abs_pose.hip): B pairs of cap matches with realistic ragged counts (pose and abs_pose: MVSEC-like scenes, abs_pose with
exact per-match depths; homography: 346 x 260 frames; 0.5 px noise, 30 % outliers), timed with device events around the whole
launch sequence.  Only the public relative_pose / homography / absolute_pose functions are used, so EINX_LIB=ab_libs/libeinx_X.so
times an A/B build.  `refine` times the refinement of the relative pose on its inliers on the pose workload: the
refinement alone on the poses relative_pose returned, and relative_pose(refine=True) against refine=False in alternating runs.

    python tools/ransac_bench.py {pose,homography,abs_pose,refine} [--B 32] [--cap 1024] [--iters 20] [--outliers 0.3]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pose_workload(nm, scenes):
    """(the estimator, its arguments after the matches, the estimator's keys of the result line)"""
    import pose_f64 as P
    K0, K1, T = (np.stack(v) for v in zip(*(s[2:] for s in scenes(P.scene))))

    def report(out):
        status = out[3].cpu().numpy()
        return {"posed": int((status >= 0).sum()), "median_pose_err_deg": float(np.median(out[4][:, 2].cpu().numpy()))}
    return nm.relative_pose, (K0, K1, T), report


def homography_workload(nm, scenes):
    import homography_f64 as Hm
    Ht = np.stack([s[2] for s in scenes(Hm.scene)]).astype(np.float32)

    def report(out):
        status, err = out[2].cpu().numpy(), out[3][:, 3].cpu().numpy()
        return {"found": int((status >= 0).sum()), "max_chosen_iteration": int(status.max()), "median_HE_error_px": float(np.median(err)),
                "max_HE_error_px": float(np.max(err))}
    return nm.homography, (np.array([Hm.IMG_SHAPE] * len(Ht), np.int32), Ht), report


def abs_pose_workload(nm, scenes, cap):
    import abs_pose_f64 as A

    def scene(rng, n, noise, outliers):
        s = A.scene(rng, n, noise=noise, outliers=outliers)
        d = np.zeros(cap, np.float32)
        d[:n] = s["d0"]
        return s["kp0"], s["kp1"], s["K0"], s["K1"], s["T"], d
    K0, K1, T, d0 = (np.stack(v) for v in zip(*(s[2:] for s in scenes(scene))))

    def run(mk0, mk1, n, K0, K1, d0, valid0, T):
        return nm.absolute_pose(mk0, mk1, n, K0, K1, d0=d0, valid0=valid0, T_0to1=T)

    def report(out):
        status, rows = out[3].cpu().numpy(), out[4].cpu().numpy()
        return {"posed": int((status >= 0).sum()), "max_chosen_iteration": int(status.max()) // 4, "median_R_err_deg": float(np.median(rows[:, 0])),
                "median_t_err": float(np.median(rows[:, 1]))}
    return run, (K0, K1, d0, np.ones_like(d0, dtype=np.uint8), T), report


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def refine_report(nm, a, cnt, args):
    """the result line of the `refine` mode: the refinement alone, then the estimator with and without it in alternating runs"""
    mk0, mk1, n, K0, K1, T = args
    first = nm.relative_pose(mk0, mk1, n, K0, K1, T)
    alone = lambda: nm.refine_relative_pose(mk0, mk1, n, K0, K1, *first[:4], T)  # noqa: E731
    plain = lambda: nm.relative_pose(mk0, mk1, n, K0, K1, T)  # noqa: E731
    both = lambda: nm.relative_pose(mk0, mk1, n, K0, K1, T, refine=True)  # noqa: E731
    for f in (alone, plain, both) * 3:
        f()
    torch.cuda.synchronize()
    t = {"refine": [], "plain": [], "with_refine": []}
    for _ in range(a.iters):
        for key, f in (("refine", alone), ("plain", plain), ("with_refine", both)):
            ms, out = timed(f)
            t[key].append(ms)
            if key == "refine":
                fine = out
    info, status = fine[3].cpu().numpy(), first[3].cpu().numpy()
    posed = status >= 0
    before, after = first[4][:, 2].cpu().numpy()[posed], fine[4][:, 2].cpu().numpy()[posed]
    line = {"B": a.B, "cap": a.cap, "outliers": a.outliers, "mean_nmatch": float(cnt.mean())}
    for key, v in t.items():
        line.update({f"{key}_ms_median": float(np.median(v)), f"{key}_ms_min": float(np.min(v)), f"{key}_ms_max": float(np.max(v))})
    line.update({"posed": int(posed.sum()), "kept": int((info[:, 0] == 1).sum()), "mean_accepted_steps": float(info[posed, 2].mean()),
                 "mean_last_set": float(info[posed, 3].mean()), "median_pose_err_deg_before": float(np.median(before)),
                 "median_pose_err_deg_after": float(np.median(after)), "mean_pose_err_deg_before": float(before.mean()),
                 "mean_pose_err_deg_after": float(after.mean())})
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("estimator", choices=("pose", "homography", "abs_pose", "refine"))
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--outliers", type=float, default=0.3)
    a = ap.parse_args()
    from helpers import load_pkg
    nm = importlib.import_module(load_pkg().__name__ + ".core.metrics._native_metrics")
    rng = np.random.default_rng(0)
    mk0 = np.zeros((a.B, a.cap, 3), np.float32)
    mk1 = np.zeros((a.B, a.cap, 3), np.float32)
    cnt = np.zeros(a.B, np.int32)

    def scenes(scene):  # fills the matches and yields each pair's scene: (k0, k1, the estimator's ground truth...)
        for b in range(a.B):
            n = int(rng.integers(a.cap // 4, a.cap + 1))  # ragged: MNN keeps a quarter to all of the top-k keypoints
            s = scene(rng, n, noise=0.5, outliers=a.outliers)
            mk0[b, :n], mk1[b, :n], cnt[b] = s[0], s[1], n
            yield s

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
    if a.estimator == "abs_pose":
        run, extra, report = abs_pose_workload(nm, scenes, a.cap)
    else:
        run, extra, report = (homography_workload if a.estimator == "homography" else pose_workload)(nm, scenes)
    args = tuple(t(x) for x in (mk0, mk1, cnt) + extra)
    if a.estimator == "refine":
        return refine_report(nm, a, cnt, args)
    for _ in range(3):
        run(*args)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        ms, out = timed(lambda: run(*args))
        times.append(ms)
    print(json.dumps({"B": a.B, "cap": a.cap, "outliers": a.outliers, "mean_nmatch": float(cnt.mean()), "ms_median": float(np.median(times)),
                      "ms_min": float(np.min(times)), "ms_max": float(np.max(times)), **report(out)}))


if __name__ == "__main__":
    main()
