#!/usr/bin/env python3
"""Device time of the batched relative pose (csrc/pose.hip): B pairs of cap matches with realistic ragged counts (MVSEC-like
scenes, 0.5 px noise, 30 % outliers), timed with device events around the whole launch sequence.

    python tools/pose_bench.py [--B 32] [--cap 1024] [--iters 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--outliers", type=float, default=0.3)
    a = ap.parse_args()
    import importlib
    from helpers import load_pkg
    pkg = load_pkg()
    nm = importlib.import_module(pkg.__name__ + ".core.metrics._native_metrics")
    import pose_f64 as P
    rng = np.random.default_rng(0)
    dev = "cuda:0"
    mk0 = np.zeros((a.B, a.cap, 3), np.float32)
    mk1 = np.zeros((a.B, a.cap, 3), np.float32)
    cnt = np.zeros(a.B, np.int32)
    K0, K1, T = [], [], []
    for b in range(a.B):
        n = int(rng.integers(a.cap // 4, a.cap + 1))  # ragged: MNN keeps a quarter to all of the top-k keypoints
        k0, k1, Ka, Kb, Tb = P.scene(rng, n, noise=0.5, outliers=a.outliers)
        mk0[b, :n], mk1[b, :n], cnt[b] = k0, k1, n
        K0.append(Ka), K1.append(Kb), T.append(Tb)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    args = (t(mk0), t(mk1), t(cnt), t(np.stack(K0)), t(np.stack(K1)), t(np.stack(T)))
    for _ in range(3):
        nm.relative_pose(*args)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = nm.relative_pose(*args)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    status = out[3].cpu().numpy()
    print(json.dumps({"B": a.B, "cap": a.cap, "outliers": a.outliers, "mean_nmatch": float(cnt.mean()), "ms_median": float(np.median(times)),
                      "ms_min": float(np.min(times)), "ms_max": float(np.max(times)), "posed": int((status >= 0).sum()),
                      "median_pose_err_deg": float(np.median(out[4][:, 2].cpu().numpy()))}))


if __name__ == "__main__":
    main()
