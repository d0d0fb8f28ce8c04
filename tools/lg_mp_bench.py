#!/usr/bin/env python3
"""Device time of LightGlue with `mp: True` (einx_lightglue_mp: the layers' linears in fp16 on the matrix cores)
against the fp32 einx_lightglue and `flash: True`, on the shipped model (d = 256, 4 x 64, 9 layers) at B pairs of cap x cap
keypoints.  Variants, timed ALTERNATELY in one process (one call of each per round, device events around the call, outputs and
workspace allocated once; median over the rounds):

    fp32_a / fp32_b   einx_lightglue, twice in every round: the distance of the two medians is the run-to-run spread
    flash             einx_lightglue_flash, plain run (no early stopping, no pruning)
    mp                einx_lightglue_mp with EINX_LG_LIN_F16 (fp32 attention)
    mp_flash          einx_lightglue_mp with EINX_LG_LIN_F16 | EINX_LG_ATTN_F16
    gemm_f16          the f16 GEMM alone: the 72 launches of a forward through einx_lg_linear_f16 on random inputs at the forward's
                      shapes over 2B stacked entries (per layer 256 -> 768, 256 -> 256, 256 | 256 -> 512, 512 -> 256 + residual, then
                      256 -> 512, 256 -> 256, 256 | 256 -> 512, 512 -> 256 + residual)

For the kernels' own times run the tool under `rocprofv3 --kernel-trace --stats` (in a run of its own): lg_gemm_kernel<.., EngF32>
and <.., EngF16> appear side by side in one session.

    python tools/lg_mp_bench.py [--B 64 1] [--cap 1024] [--iters 15] [--only gemm_f16]   (output: profiles/lg_mp_bench.txt)
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F16_MFMA_PEAK_TFLOPS = 2516.6  # dense fp16, MI355X data sheet
# (K1, K2, N, residual) of the eight launches of a layer
LAYER_GEMMS = [(256, 0, 768, 0), (256, 0, 256, 0), (256, 256, 512, 0), (512, 0, 256, 1), (256, 0, 512, 0), (256, 0, 256, 0), (256, 256, 512, 0),
               (512, 0, 256, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--only", default=None, help="time this variant alone (for a profiler run)")
    a = ap.parse_args()
    from helpers import lgf64_shipped_state_dict, load_pkg
    pkg = load_pkg()
    N = pkg.native
    _lib = importlib.import_module(pkg.__name__ + "._lib")
    L = N.lib()
    dev = "cuda:0"
    sd = lgf64_shipped_state_dict(7)
    lg = pkg.LightGlue({"mp": True}).to(dev)
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    lg.eval()
    w, w_mp = lg._pack()[0], lg._pack(mp=True)[0]  # the fp32 image (folded, as every forward packs it) and the mode's
    p = N._ptr
    for B in a.B:
        cap, d, heads, layers = a.cap, 256, 4, 9
        g = torch.Generator().manual_seed(5 + B)
        desc = [torch.nn.functional.normalize(torch.randn((B, cap, d), generator=g), dim=-1).to(dev) for _ in range(2)]
        kpts = [(torch.rand((B, cap, 3), generator=g) * torch.tensor([260.0, 346.0, 1.0])).to(dev) for _ in range(2)]
        cnt = torch.full((B,), cap, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.einx_lightglue_mp_ws_bytes(B, cap, cap, d, heads, d, layers)), dtype=torch.uint8, device=dev)
        m0, m1 = (torch.empty((B, cap), dtype=torch.int64, device=dev) for _ in range(2))
        s0, s1 = (torch.empty((B, cap), dtype=torch.float32, device=dev) for _ in range(2))
        la = torch.empty((B, cap + 1, cap + 1), dtype=torch.float32, device=dev)
        ref0, ref1 = (torch.empty((B, cap, d), dtype=torch.float32, device=dev) for _ in range(2))
        stream = N._stream(la)
        inputs = (p(kpts[0]), p(desc[0]), p(cnt), cap, p(kpts[1]), p(desc[1]), p(cnt), cap, B, 260.0, 346.0, 260.0, 346.0, p(ws))
        outs = (p(m0), p(m1), p(s0), p(s1), p(la), p(ref0), p(ref1))
        x = torch.randn((2 * B, cap, 512), generator=g).to(dev)  # read as [.., 256] or [.., 512] rows
        x2 = torch.randn((2 * B, cap, 256), generator=g).to(dev)
        w16 = (torch.randn((768, 512), generator=g) / 16).to(dev).half()
        bias = torch.randn((768,), generator=g).to(dev)
        y = torch.zeros((2 * B, cap, 768), dtype=torch.float32, device=dev)
        cnt2 = torch.full((2 * B,), cap, dtype=torch.int32, device=dev)

        def fp32():
            N.check(L.einx_lightglue(ctypes.byref(w), *inputs, *outs, 1, stream), "einx_lightglue")

        def flash():
            N.check(L.einx_lightglue_flash(ctypes.byref(w), None, ctypes.sizeof(_lib.LgHead), -1.0, -1.0, 0, *inputs, *outs, 1, None, None, None, None,
                                           None, None, stream), "einx_lightglue_flash")

        def mp_call(mode):
            N.check(L.einx_lightglue_mp(ctypes.byref(w_mp), None, ctypes.sizeof(_lib.LgHead), -1.0, -1.0, 0, *inputs, *outs, 1, None, None, None, None,
                                        None, None, mode, stream), "einx_lightglue_mp")

        def gemm_f16():
            for _ in range(layers):
                for k1, k2, n, resid in LAYER_GEMMS:
                    N.check(L.einx_lg_linear_f16(p(x), p(x2) if k2 else None, k1 if k2 else 0, k1 + k2, p(w16), p(bias), n, p(y), n, p(y) if resid else None,
                                                 p(cnt2), cap, 2 * B, resid, stream), "einx_lg_linear_f16")

        variants = {"fp32_a": fp32, "flash": flash, "mp": lambda: mp_call(N.LG_LIN_F16), "mp_flash": lambda: mp_call(N.LG_LIN_F16 | N.LG_ATTN_F16),
                    "gemm_f16": gemm_f16, "fp32_b": fp32}
        if a.only:
            variants = {a.only: variants[a.only]}
        for fn in variants.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.iters):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in times.items()}
        line = {"B": B, "cap": cap, "d": d, "iters": a.iters, "ms_median": med, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
                "ms_max": {k: float(np.max(v)) for k, v in times.items()}}
        if not a.only:
            fp32_ms = 0.5 * (med["fp32_a"] + med["fp32_b"])
            spread = abs(med["fp32_a"] - med["fp32_b"])
            gemm_flop = 2.0 * sum((k1 + k2) * n for k1, k2, n, _ in LAYER_GEMMS) * 2 * B * cap * layers
            line.update({"fp32_ms": fp32_ms, "fp32_run_to_run_spread_ms": spread,
                         "mp_faster_than_fp32_by_ms": fp32_ms - med["mp"], "mp_flash_faster_than_flash_by_ms": med["flash"] - med["mp_flash"],
                         "mp_flash_faster_than_flash_by_more_than_spread": bool(med["flash"] - med["mp_flash"] > spread),
                         "pairs_per_s": {k: 1e3 * B / (fp32_ms if k == "fp32" else med[k]) for k in ("fp32", "flash", "mp", "mp_flash")},
                         "gemm_gflop_per_forward": gemm_flop / 1e9, "gemm_f16_tflops": gemm_flop / med["gemm_f16"] / 1e9,
                         "gemm_f16_fraction_of_f16_mfma_peak": gemm_flop / med["gemm_f16"] / 1e9 / F16_MFMA_PEAK_TFLOPS})
        print(json.dumps(line))


if __name__ == "__main__":
    main()
