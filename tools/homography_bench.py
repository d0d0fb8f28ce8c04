#!/usr/bin/env python3
"""Device time of the batched homography (csrc/homography.hip): B pairs of cap matches with ragged counts (346 x 260 frames,
0.5 px noise, 30 % outliers), timed with device events around the whole launch sequence.

    python tools/homography_bench.py [--B 32] [--cap 1024] [--iters 20] [--outliers 0.3]
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
    import homography_f64 as Hm
    rng = np.random.default_rng(0)
    dev = "cuda:0"
    mk0 = np.zeros((a.B, a.cap, 3), np.float32)
    mk1 = np.zeros((a.B, a.cap, 3), np.float32)
    cnt = np.zeros(a.B, np.int32)
    Ht = []
    for b in range(a.B):
        n = int(rng.integers(a.cap // 4, a.cap + 1))  # ragged: MNN keeps a quarter to all of the top-k keypoints
        k0, k1, h = Hm.scene(rng, n, noise=0.5, outliers=a.outliers)
        mk0[b, :n], mk1[b, :n], cnt[b] = k0, k1, n
        Ht.append(h)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    args = (t(mk0), t(mk1), t(cnt), t(np.array([Hm.IMG_SHAPE] * a.B, np.int32)), t(np.stack(Ht).astype(np.float32)))
    for _ in range(3):
        nm.homography(*args)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = nm.homography(*args)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    status = out[2].cpu().numpy()
    err = out[3][:, 3].cpu().numpy()
    print(json.dumps({"B": a.B, "cap": a.cap, "outliers": a.outliers, "mean_nmatch": float(cnt.mean()), "ms_median": float(np.median(times)),
                      "ms_min": float(np.min(times)), "ms_max": float(np.max(times)), "found": int((status >= 0).sum()),
                      "max_chosen_iteration": int(status.max()), "median_HE_error_px": float(np.median(err)), "max_HE_error_px": float(np.max(err))}))


if __name__ == "__main__":
    main()
