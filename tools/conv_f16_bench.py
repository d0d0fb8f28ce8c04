#!/usr/bin/env python3
"""Device time of the opt-in fp16 convolutions (conv_f16_kernel) against today's fp32 kernels, in ONE process.

Layers: every covered layer shape (cin % 8 == 0, not the first layer) of SuperPointv1 and of the event VGG at B = 32 on the
264 x 352 padded map.  Per round one call of fp32 (einx_conv_block: the parent's kernels, unchanged), one of fp16
(einx_conv_block_f16) and a second one of fp32, device events around each; medians over the rounds.  The distance of the two fp32
medians is the run-to-run spread.  Per layer: achieved TFLOP/s (2 B H W cout cin ks^2) and the compulsory HBM traffic rate (fp32
input read once + fp32 output written once) of both modes, against the f16 matrix peak and the HBM peak.

Forwards: the whole EIM forward (SP+MNN B = 32, SP+LightGlue B = 64, SP+MNN one pair), two models on the same weights, one with
`half_precision` on both extractors; same alternation.

    python tools/conv_f16_bench.py [--iters 15] [--skip-forwards]      (output: profiles/conv_f16_bench.txt)
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

F16_MFMA_PEAK_TFLOPS = 2516.6  # dense fp16, MI355X data sheet
F32_MFMA_PEAK_TFLOPS = 157.3
HBM_PEAK_GBS = 8000.0


def timed(variants, iters):
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(iters):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in times.items()}


def layer_shapes(ext, Hp, Wp):
    """(cin, cout, ks, relu, bn, pool, H, W) of every covered layer"""
    bb, det, desc = ext._stacks()
    out, h, w = [], Hp, Wp
    for i, (block, pool) in enumerate(bb):
        conv, bn, relu = ext._spec(block)
        if i > 0 and conv.in_channels % 8 == 0:
            out.append((conv.in_channels, conv.out_channels, conv.kernel_size[0], bool(relu), bn is not None, bool(pool), h, w))
        if pool:
            h, w = h // 2, w // 2
    for block in list(det) + list(desc):
        conv, bn, relu = ext._spec(block)
        if conv.in_channels % 8 == 0:
            out.append((conv.in_channels, conv.out_channels, conv.kernel_size[0], bool(relu), bn is not None, False, h, w))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--skip-forwards", action="store_true")
    a = ap.parse_args()
    from helpers import load_pkg
    pkg = load_pkg()
    N = pkg.native
    L = N.lib()
    dev = "cuda:0"
    import bench

    wl = bench.Workload(pkg, dev, "sp_mnn", 2, calibrate=False)
    shapes = {}
    for net, ext in (("superpointv1", wl.model.image_extractor.extractor), ("vgg", wl.model.event_extractor.extractor)):
        for s in layer_shapes(ext, 264, 352):
            shapes.setdefault(s, []).append(net)
    g = torch.Generator().manual_seed(3)
    B = a.B
    for (cin, cout, ks, relu, bn, pool, H, W), nets in shapes.items():
        x = torch.randn((B, cin, H, W), generator=g).to(dev)
        wgt = (torch.randn((cout, cin, ks, ks), generator=g) / (ks * ks * cin) ** 0.5).to(dev)
        bias = torch.randn((cout,), generator=g).to(dev)
        bnt = (torch.rand(cout, generator=g).to(dev) + 0.5, torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev),
               torch.rand(cout, generator=g).to(dev) + 0.5, 1e-5) if bn else None
        layer = N.ConvLayer(wgt, bias, bnt, relu=relu, pool=pool)
        med = timed({"fp32_a": lambda: layer(x), "fp16": lambda: layer(x, half=True), "fp32_b": lambda: layer(x)}, a.iters)
        layer(x)
        k32 = L.einx_conv_last_kernel().decode()
        layer(x, half=True)
        k16 = L.einx_conv_f16_last_kernel().decode()
        flop = 2.0 * B * H * W * cout * cin * ks * ks
        Ho, Wo = (H // 2, W // 2) if pool else (H, W)
        byts = 4.0 * B * (cin * H * W + cout * Ho * Wo)
        fp32_ms, spread = 0.5 * (med["fp32_a"] + med["fp32_b"]), abs(med["fp32_a"] - med["fp32_b"])
        tf16, gb16 = flop / med["fp16"] / 1e9, byts / med["fp16"] / 1e6
        print(json.dumps({"layer": f"{cin}->{cout} {ks}x{ks}{' pool' if pool else ''} @{H}x{W}", "nets": nets, "B": B, "fp32_ms": round(fp32_ms, 4),
                          "fp32_spread_ms": round(spread, 4), "fp16_ms": round(med["fp16"], 4), "speedup": round(fp32_ms / med["fp16"], 2),
                          "fp16_slower_beyond_spread": bool(med["fp16"] > fp32_ms + spread),
                          "fp32_tflops": round(flop / fp32_ms / 1e9, 1), "fp32_fraction_of_f32_peak": round(flop / fp32_ms / 1e9 / F32_MFMA_PEAK_TFLOPS, 3),
                          "fp16_tflops": round(tf16, 1), "fp16_fraction_of_f16_peak": round(tf16 / F16_MFMA_PEAK_TFLOPS, 3),
                          "fp16_hbm_gbs": round(gb16, 0), "fp16_fraction_of_hbm_peak": round(gb16 / HBM_PEAK_GBS, 3),
                          # the roof that bounds the layer: the larger of FLOP / matrix peak and compulsory bytes / HBM peak
                          "fp16_binding_roof": "f16 matrix" if tf16 / F16_MFMA_PEAK_TFLOPS > gb16 / HBM_PEAK_GBS else "HBM",
                          "fp16_share_of_binding_roof": round(max(tf16 / F16_MFMA_PEAK_TFLOPS, gb16 / HBM_PEAK_GBS), 3),
                          "fp32_kernel": k32, "fp16_kernel": k16}), flush=True)
        del x, layer
    if a.skip_forwards:
        return
    for config, Bf in (("sp_mnn", 32), ("sp_lg", 64), ("sp_mnn", 1)):
        w32 = bench.Workload(pkg, dev, config, Bf, calibrate=True)
        w16 = bench.Workload(pkg, dev, config, Bf, calibrate=False, same_scene=w32.same_scene)  # the same weights and inputs
        w16.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w32.sd.items()}, strict=False)
        for ext in (w16.model.event_extractor.extractor, w16.model.image_extractor.extractor):
            ext.half_precision = True
            assert ext.conv_mode == "fp16"
        med = timed({"fp32_a": w32.step, "fp16": w16.step, "fp32_b": w32.step}, a.iters)
        fp32_ms, spread = 0.5 * (med["fp32_a"] + med["fp32_b"]), abs(med["fp32_a"] - med["fp32_b"])
        nm = {k: float(np.mean([int(t.shape[0]) for t in w.step()[2]["matched_kpts0"]])) for k, w in (("fp32", w32), ("fp16", w16))}
        print(json.dumps({"forward": config, "B": Bf, "fp32_ms": round(fp32_ms, 3), "fp32_spread_ms": round(spread, 3), "fp16_ms": round(med["fp16"], 3),
                          "speedup": round(fp32_ms / med["fp16"], 2), "pairs_per_s": {"fp32": round(1e3 * Bf / fp32_ms, 1), "fp16": round(1e3 * Bf / med["fp16"], 1)},
                          "mean_matches": nm}), flush=True)
        del w32, w16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
