#!/usr/bin/env python3
"""Device time of the fused descriptor loss (csrc/loss.hip) at B pairs of SuperPoint-shaped raw descriptor maps
(256 x H/8 x W/8), masked `mae` as every shipped train config asks for it, against what a caller had to do without it: resolve
`normalized_descriptors` on both sides with the existing kernels (einx_upsample_normalize, two [B,256,H,W] maps) and reduce them
with torch operators on the same device.  Device events around one call each; the two values are compared before timing.

    python tools/loss_bench.py [--B 32] [--H 260] [--W 346] [--D 256] [--iters 20]      (one JSON line; kept as profiles/loss_bench.txt)
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
    ap.add_argument("--H", type=int, default=260)
    ap.add_argument("--W", type=int, default=346)
    ap.add_argument("--D", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from helpers import load_pkg
    pkg = load_pkg()
    N, synth = pkg.native, pkg.synth
    dev = "cuda:0"
    pads = N.padder_pads(a.H, a.W, 8)
    padded = (a.H + pads[2] + pads[3], a.W + pads[0] + pads[1])
    hc, wc = padded[0] // 8, padded[1] // 8
    one = lambda seed: torch.from_numpy(synth.normalish(seed, (1, a.D, hc, wc)))  # noqa: E731
    jitter = lambda seed: torch.from_numpy(synth.uniform(seed, (a.B, 1, 1, 1), 0.5, 1.5))  # noqa: E731
    ra, rb = (one(1) * jitter(3)).to(dev).contiguous(), (one(2) * jitter(4)).to(dev).contiguous()
    mask = torch.from_numpy(synth.uniform01(5, (a.B, 1, a.H, a.W)) > 0.4).to(dev)

    def fused():
        sc = N.desc_loss(ra, 1.0, rb, 1.0, padded, pads, 8, mask, "mae")
        return sc[:, 0].sum() / sc[:, 1].sum()

    def resolve():
        return N.upsample_normalize(ra, padded, pads, 1.0), N.upsample_normalize(rb, padded, pads, 1.0)

    def reduce(x, y):  # the reference's expression, the mask broadcast over the channels instead of repeated
        return ((x - y).abs() * mask).sum() / (mask.sum() * a.D)

    def materialised():
        return reduce(*resolve())

    v0, v1 = float(fused()), float(materialised())
    maps = resolve()
    line = {"B": a.B, "D": a.D, "H": a.H, "W": a.W, "mode": "mae", "masked": True, "fused_value": v0, "materialised_float32_value": v1,
            "map_bytes_per_side": int(maps[0].numel() * 4), "fused_ws_bytes": int(N.lib().einx_desc_loss_ws_bytes(
                a.B, a.D, hc, wc, padded[0], padded[1], pads[2], pads[0], a.H, a.W, 8)),
            "fused": timed(fused, a.iters), "materialise_and_reduce": timed(materialised, a.iters),
            "resolve_both_maps_only": timed(resolve, a.iters), "torch_reduce_only": timed(lambda: reduce(*maps), a.iters)}
    line["speedup"] = line["materialise_and_reduce"]["ms_median"] / line["fused"]["ms_median"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
