#!/usr/bin/env python3
"""Device time of the core.geometry entries (csrc/geometry.hip) against the same rules written in torch operators on
the same device (grid_sample, matmul, einsum): dense_warp_consistency with and without the cycle check, project on sparse
keypoints, sym_epipolar_distance_all.  Device events around one call each, kernel and torch form alternating; the comparison is
for time only (the torch forms round differently and are no test).

    python tools/geometry_bench.py [--B 32] [--H 260] [--W 346] [--N 1024] [--iters 9]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"


def t_sample_depth(pts, dm):
    """bilinear + nearest grid_sample of the NaN-masked map, NaN samples replaced by the nearest pixel"""
    h, w = dm.shape[-2:]
    masked = torch.where(dm > 0, dm, torch.full_like(dm, float("nan")))[:, None]
    grid = (pts / pts.new_tensor([w, h]) * 2 - 1)[:, None]
    lin = F.grid_sample(masked, grid, mode="bilinear", align_corners=False)
    near = F.grid_sample(masked, grid, mode="nearest", align_corners=False)
    d = torch.where(lin != lin, near, lin)[:, 0, 0]
    return d, (d == d) & (d > 0)


def t_pinhole(p3, K):
    z = p3[..., 2]
    uv = p3[..., :2] / z.clamp(min=1e-4)[..., None] * torch.stack([K[:, 0, 0], K[:, 1, 1]], -1)[:, None] + K[:, None, :2, 2]
    size = 2 * K[:, None, :2, 2] - 1
    return uv, (z > 1e-4) & ((uv >= 0) & (uv <= size)).all(-1)


def t_unproject(pts, K, d):
    xy = (pts - K[:, None, :2, 2]) / torch.stack([K[:, 0, 0], K[:, 1, 1]], -1)[:, None]
    return torch.cat([xy, torch.ones_like(xy[..., :1])], -1) * d[..., None]


def t_project(kp, d, valid, Ki, Kj, T, depth_j, ccth):
    R, t = T[:, :3, :3], T[:, :3, 3]
    uv, ok = t_pinhole(t_unproject(kp, Ki, d) @ R.mT + t[:, None], Kj)
    vis = valid & ok
    if ccth is None:
        return uv, vis
    dj, validj = t_sample_depth(uv, depth_j)
    Ri = R.mT
    ti = -(Ri @ t[..., None])[..., 0]
    back, back_ok = t_pinhole(t_unproject(uv, Kj, dj) @ Ri.mT + ti[:, None], Ki)
    return uv, vis & (((kp - back) ** 2).sum(-1) < ccth) & back_ok & validj


def t_dense(depth_i, depth_j, Ki, Kj, T, ccth):
    B, H, W = depth_i.shape
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=DEV), torch.arange(W, dtype=torch.float32, device=DEV), indexing="ij")
    kp = (torch.stack([x, y], -1).reshape(1, H * W, 2) + 0.5).expand(B, -1, -1)
    d = depth_i.reshape(B, -1)
    return t_project(kp, d, d > 0, Ki, Kj, T, depth_j, ccth)


def t_epipolar(p0, p1, E, eps=1e-15):
    h = lambda p: torch.cat([p, torch.ones_like(p[..., :1])], -1)  # noqa: E731
    p0, p1 = h(p0), h(p1)
    s = torch.einsum("bmi,bij,bnj->bnm", p1, E, p0).abs()
    l1, l0 = torch.einsum("bij,bnj->bni", E, p0), torch.einsum("bij,bmi->bmj", E, p1)
    return (s / (l1[..., None, 0] ** 2 + l1[..., None, 1] ** 2 + eps).sqrt() + s / (l0[:, None, :, 0] ** 2 + l0[:, None, :, 1] ** 2 + eps).sqrt()) / 2


def timed(fns, iters):
    """median / min / max device ms of each function, the functions alternating"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v)), "n": len(v)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--H", type=int, default=260)
    ap.add_argument("--W", type=int, default=346)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=9)
    a = ap.parse_args()
    from helpers import load_pkg
    nm = importlib.import_module(load_pkg().__name__ + ".core.metrics._native_metrics")
    rng = np.random.default_rng(0)
    B, H, W, N = a.B, a.H, a.W, a.N
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)  # noqa: E731

    def depth_map():  # a slanted background, a nearer box, 7 % holes
        yy, xx = np.mgrid[0:H, 0:W]
        d = 4.0 + 0.004 * xx[None] + 0.002 * yy[None] + rng.uniform(0, 0.5, (B, 1, 1))
        d[:, H // 4:H // 2, W // 3:W // 3 * 2] = 2.0
        d[rng.uniform(size=d.shape) < 0.07] = 0.0
        return dev(d)
    di, dj = depth_map(), depth_map()
    K = dev(np.tile(np.array([[226.0, 0, W / 2], [0, 226.0, H / 2], [0, 0, 1]]), (B, 1, 1)))
    T = np.tile(np.eye(4), (B, 1, 1))
    ang = rng.uniform(-0.03, 0.03, B)
    T[:, 0, 0], T[:, 0, 2], T[:, 2, 0], T[:, 2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
    T[:, :3, 3] = rng.uniform(-0.15, 0.15, (B, 3))
    T = dev(T)
    kp = dev(np.stack([rng.uniform(1, W - 1, (B, N)), rng.uniform(1, H - 1, (B, N))], -1))
    d, valid = t_sample_depth(kp, di)
    d = d.contiguous()
    p1 = dev(np.stack([rng.uniform(1, W - 1, (B, N)), rng.uniform(1, H - 1, (B, N))], -1))
    Fm = dev(rng.normal(size=(B, 3, 3)) * np.array([[1e-5, 1e-5, 1e-3], [1e-5, 1e-5, 1e-3], [1e-3, 1e-3, 1.0]]))
    out = {"B": B, "H": H, "W": W, "N": N, "hole_fraction": float((di <= 0).float().mean())}
    for tag, cc in (("dense_warp", None), ("dense_warp_cc", 1.0)):
        out[tag] = timed({"kernel": lambda: nm.geom_dense_warp(di, dj, K, K, T, cc_bound=cc), "torch": lambda: t_dense(di, dj, K, K, T, cc)}, a.iters)
        k, r = nm.geom_dense_warp(di, dj, K, K, T, cc_bound=cc), t_dense(di, dj, K, K, T, cc)
        out[tag]["visible_fraction"] = float(k["visible"].float().mean())
        out[tag]["flags_differing_from_torch"] = int((k["visible"].reshape(B, -1) != r[1]).sum())
    out["dense_warp_both_directions_cc"] = timed({"kernel": lambda: nm.geom_dense_warp(di, dj, K, K, T, cc_bound=1.0, both=True)}, a.iters)
    out["project_cc"] = timed({"kernel": lambda: nm.geom_project(kp, K, K, T, d=d, valid=valid, depth_j=dj, cc_bound=1.0),
                               "torch": lambda: t_project(kp, d, valid, K, K, T, dj, 1.0)}, a.iters)
    out["epipolar_all"] = timed({"kernel": lambda: nm.epipolar_all(kp, p1, Fm), "torch": lambda: t_epipolar(kp, p1, Fm)}, a.iters)
    e = (nm.epipolar_all(kp, p1, Fm) - t_epipolar(kp, p1, Fm)).abs().max()
    out["epipolar_all"]["max_abs_difference_from_torch"] = float(e)
    out["epipolar_all"]["output_MB"] = B * N * N * 4 / 1e6
    for k in ("dense_warp", "dense_warp_cc", "project_cc", "epipolar_all"):
        out[k]["torch_over_kernel"] = out[k]["torch"]["ms_median"] / out[k]["kernel"]["ms_median"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
