#!/usr/bin/env python3
"""Device time of the ground-truth matches (csrc/gt_matches.hip) at B pairs of cap x cap keypoints on H x W depth
maps, against the same contract written with dense torch operators on the same device (materialised B x N x M distance matrices,
arg-min, a gather for the mutual check: the shape of computation the reference's gt_matches_from_pose_depth has).  Device events
around one call each; the dense form is checked against the op on the O(N + M) labels before it is timed.

    python tools/gt_matches_bench.py [--B 32] [--cap 1024] [--H 260] [--W 346] [--iters 20]
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


def dense_baseline(kp0, kp1, depth0, depth1, K0, K1, T01, T10, pos_th=3, neg_th=5):
    """DESIGN.md 8e written with dense torch operators, keypoints in (x, y): stage A per keypoint with gathers from the depth
    map, stage B on materialised [B,N,M] distance matrices (arg-min, a gather for the mutual check, where); returns the labels"""
    B = kp0.shape[0]
    rows = torch.arange(B, device=kp0.device)[:, None]

    def tap(depth, xi, yi):  # depth at integer pixels, NaN for a hole, and whether the pixel is inside the map
        H, W = depth.shape[-2:]
        inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        v = depth[rows, yi.clamp(0, H - 1), xi.clamp(0, W - 1)]
        return torch.where(v > 0, v, torch.full_like(v, float("nan"))), inside

    def depth_at(kp, depth):
        ix, iy = kp[..., 0] - 0.5, kp[..., 1] - 0.5
        x0, y0 = ix.floor(), iy.floor()
        acc, hole = torch.zeros_like(ix), torch.zeros_like(ix, dtype=torch.bool)
        for dy in (0, 1):
            for dx in (0, 1):
                v, inside = tap(depth, x0.long() + dx, y0.long() + dy)
                w = ((x0 + 1 - ix) if dx == 0 else (ix - x0)) * ((y0 + 1 - iy) if dy == 0 else (iy - y0))
                hole |= inside & v.isnan() & (w != 0)
                acc = acc + torch.where(inside & ~v.isnan(), v * w, torch.zeros_like(v))
        v, inside = tap(depth, ix.round().long(), iy.round().long())
        d = torch.where(hole, torch.where(inside, v, torch.zeros_like(v)), acc)
        return d, d > 0

    def to_other_view(kp, d, ok, Ks, Ko, T):
        f, c = torch.stack([Ks[:, 0, 0], Ks[:, 1, 1]], -1)[:, None], Ks[:, None, :2, 2]
        fo, co = torch.stack([Ko[:, 0, 0], Ko[:, 1, 1]], -1)[:, None], Ko[:, None, :2, 2]
        ray = torch.cat([(kp - c) / f, torch.ones_like(d)[..., None]], -1) * d[..., None]
        q = ray @ T[:, :3, :3].mT + T[:, None, :3, 3]
        uv = q[..., :2] / q[..., 2:].clamp_min(1e-4) * fo + co
        seen = ok & (q[..., 2] > 1e-4) & (uv >= 0).all(-1) & (uv <= 2 * co - 1).all(-1)
        return uv, seen

    def sq(a, b):
        dx, dy = a[:, :, None, 0] - b[:, None, :, 0], a[:, :, None, 1] - b[:, None, :, 1]
        return dx * dx + dy * dy

    d0, ok0 = depth_at(kp0, depth0)
    d1, ok1 = depth_at(kp1, depth1)
    p01, seen0 = to_other_view(kp0, d0, ok0, K0, K1, T01)
    p10, seen1 = to_other_view(kp1, d1, ok1, K1, K0, T10)
    a, c = sq(p01, kp1), sq(kp0, p10)
    both = seen0[:, :, None] & seen1[:, None, :]
    dist = torch.where(both, torch.maximum(a, c), torch.full_like(a, float("inf")))
    row_min, row_arg = dist.min(2)
    col_min, col_arg = dist.min(1)
    mutual0 = (col_arg.gather(1, row_arg) == torch.arange(dist.shape[1], device=dist.device)) & (row_min < pos_th ** 2)
    mutual1 = (row_arg.gather(1, col_arg) == torch.arange(dist.shape[2], device=dist.device)) & (col_min < pos_th ** 2)
    far0 = ok0 & (a.min(2).values > neg_th ** 2)
    far1 = ok1 & (c.min(1).values > neg_th ** 2)
    label = lambda far, mutual, arg: torch.where(far, torch.full_like(arg, -1), torch.where(mutual, arg, torch.full_like(arg, -2)))  # noqa: E731
    return label(far0, mutual0, row_arg), label(far1, mutual1, col_arg)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--H", type=int, default=260)
    ap.add_argument("--W", type=int, default=346)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import gt_matches_ref as R
    from helpers import load_pkg
    nm = importlib.import_module(load_pkg().__name__ + ".core.metrics._native_metrics")
    sc = R.scene(7, a.B, a.cap, a.cap, (a.H, a.W), (a.H, a.W), f0=256.0, f1=256.0, n_corr=a.cap // 2)
    t = {k: torch.from_numpy(v).to("cuda:0") for k, v in sc.items()}
    op = lambda: nm.gt_matches(t["kp0"], t["kp1"], t["n"], t["m"], t["depth0"], t["depth1"], t["K0"], t["K1"], t["T01"], t["T10"],  # noqa: E731
                               ordering="xy")
    ref = lambda: dense_baseline(t["kp0"], t["kp1"], t["depth0"], t["depth1"], t["K0"], t["K1"], t["T01"], t["T10"])  # noqa: E731
    got, (m0, m1) = op(), ref()
    differ = int((got["matches0"] != m0).sum() + (got["matches1"] != m1).sum())  # float noise of the torch form near a threshold
    pred = torch.where(got["matches0"] >= 0, got["matches0"], got["matches0"].new_tensor(-1))
    score = torch.rand(pred.shape, device=pred.device)
    line = {"B": a.B, "cap": a.cap, "H": a.H, "W": a.W, "positives_per_pair": float((got["matches0"] > -1).sum()) / a.B,
            "labels_differing_from_dense_torch": differ, "labels": int(m0.numel() + m1.numel()),
            "gt_matches": timed(op, a.iters), "dense_torch": timed(ref, a.iters),
            "match_pr": timed(lambda: nm.match_pr(pred, got["matches0"], t["n"], scores0=score), a.iters)}
    line["speedup"] = line["dense_torch"]["ms_median"] / line["gt_matches"]["ms_median"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
