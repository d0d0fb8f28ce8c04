#!/usr/bin/env python3
"""Device time of the pair metrics under depth + motion (einx_pair_metrics_pose) against the homography form
(einx_pair_metrics), which shares the O(N M) neighbour search and differs by two or four depth samples per keypoint: B = 32 pairs,
1024 x 1024 keypoints, 400 matches, D = 256, 260 x 346 depth maps with 20 % holes, thresholds (1, 3).  Seeded synthetic inputs.
Device events around 50 calls, 7 runs after a warm-up, the median (and the extremes) per call.

    python tools/pose_metrics_bench.py [--root DIR] [--what pose|hom] [--out FILE]

--root: the directory that holds the package to time (default: this checkout).  `--what hom --root <a checkout of the parent
commit>` times the homography form there: the yardstick of profiles/pose_metrics_bench.txt."""
import argparse
import importlib
import os
import statistics
import sys
import types

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--what", default="pose", choices=("pose", "hom"))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.root)
NM = importlib.import_module("ei-nexus_official_amd.core.metrics._native_metrics")
DEV = "cuda:0"
B, CAP, D, H, W, M = 32, 1024, 256, 260, 346, 400


def feats(seed):
    """what batch_metrics reads of a BatchedFeats: (y, x, score) keypoints on the extractors' half-integer grid, unit descriptors"""
    g = np.random.default_rng(seed)
    pos = np.stack([g.integers(0, H, (B, CAP)) + 0.5, g.integers(0, W, (B, CAP)) + 0.5, g.random((B, CAP))], 2).astype(np.float32)
    desc = g.standard_normal((B, CAP, D)).astype(np.float32)
    desc /= np.linalg.norm(desc, axis=2, keepdims=True)
    det = types.SimpleNamespace(positions=torch.from_numpy(pos).to(DEV), counts=torch.full((B,), CAP, dtype=torch.int32, device=DEV))
    return types.SimpleNamespace(det=det, sparse_desc=torch.from_numpy(desc).to(DEV), image_size=(H, W), ordering="yx")


ev, im = feats(1), feats(2)
mk0, mk1 = torch.zeros((B, CAP, 3), device=DEV), torch.zeros((B, CAP, 3), device=DEV)
mk0[:, :M] = ev.det.positions[:, :M]
mk1[:, :M] = ev.det.positions[:, :M] + 1.0
mr = types.SimpleNamespace(mk0=mk0, mk1=mk1, nmatch=torch.full((B,), M, dtype=torch.int32, device=DEV))
depth = []
for s in (3, 4):
    g = np.random.default_rng(s)
    d = 2.0 + g.random((B, H, W)).astype(np.float32)
    d[g.random((B, H, W)) < 0.2] = 0.0
    depth.append(torch.from_numpy(d).to(DEV))
K = torch.tensor([[226.0, 0, 173.0], [0, 226.0, 130.0], [0, 0, 1]], device=DEV).expand(B, 3, 3).contiguous()
T = torch.eye(4, device=DEV).expand(B, 4, 4).clone()
T[:, 0, 3], T[:, 1, 3] = 0.05, -0.02


def timed(fn, calls=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        runs.append(a.elapsed_time(b) / calls * 1000.0)
    return f"median {statistics.median(runs):.1f} us (min {min(runs):.1f}, max {max(runs):.1f})"


lines = []
if args.what == "hom":
    lines.append("batch_metrics (homography form, identity), --root checkout: " + timed(lambda: NM.batch_metrics(ev, im, mr, None, (1, 3), (1, 3))))
else:
    for occ in (None, 1.0):
        fn = lambda: NM.batch_metrics_pose(ev, im, mr, K, K, T, tuple(depth), None, (1, 3), (1, 3), (1, 3), occ)  # noqa: E731
        row = " ".join(f"{v:.4f}" for v in fn()[0].tolist())
        lines.append(f"batch_metrics_pose occlusion_th={occ}: {timed(fn)}; row 0 = {row}")
    lines.append("batch_metrics_pose EPI only (no depth): " + timed(lambda: NM.batch_metrics_pose(ev, im, mr, K, K, T, None, None, (), (), (1, 3), None)))
    lines.append("batch_metrics (homography form, identity), this checkout: " + timed(lambda: NM.batch_metrics(ev, im, mr, None, (1, 3), (1, 3))))
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
