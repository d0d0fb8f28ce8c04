#!/usr/bin/env python3
"""Device time of LightGlue with `flash: True` (einx_lightglue_flash: attention in fp16 on the matrix cores) against
the fp32 einx_lightglue, on the shipped model (d = 256, 4 x 64, 9 layers) at B pairs of cap x cap keypoints.  Variants, timed
ALTERNATELY in one process (one call of each per round, device events around the call, outputs and workspace allocated once;
median over the rounds):

    fp32_a / fp32_b   einx_lightglue, twice in every round: the distance of the two medians is the run-to-run spread
    flash             einx_lightglue_flash, plain run (no early stopping, no pruning)
    attn_f16          the flash attention alone: the 18 launches of a forward through einx_lg_attention_f16 on random q, k, v
                      (9 self over 2B stacked entries at row stride 256, 9 cross through kv_shift = B at row stride 512)

For the kernels' own times run the tool under `rocprofv3 --kernel-trace --stats`: lg_attn_kernel and lg_attn_f16_kernel appear side
by side in one session.

    python tools/lg_flash_bench.py [--B 64 1] [--cap 1024] [--iters 15]   (output: profiles/lg_flash_bench.txt)
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

# 4 (2 products x multiply-add) x heads x head_dim x nq x nk per attention call, 4 calls per layer and pair (2 self, 2 cross)
F16_MFMA_PEAK_TFLOPS = 2516.6  # dense fp16, MI355X data sheet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=15)
    a = ap.parse_args()
    from helpers import lgf64_shipped_state_dict, load_pkg
    pkg = load_pkg()
    N = pkg.native
    _lib = importlib.import_module(pkg.__name__ + "._lib")
    L = N.lib()
    dev = "cuda:0"
    sd = lgf64_shipped_state_dict(7)
    lg = pkg.LightGlue({}).to(dev)
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    w = lg.eval()._pack()[0]
    p = N._ptr
    for B in a.B:
        cap, d, heads, layers = a.cap, 256, 4, 9
        g = torch.Generator().manual_seed(5 + B)
        desc = [torch.nn.functional.normalize(torch.randn((B, cap, d), generator=g), dim=-1).to(dev) for _ in range(2)]
        kpts = [(torch.rand((B, cap, 3), generator=g) * torch.tensor([260.0, 346.0, 1.0])).to(dev) for _ in range(2)]
        cnt = torch.full((B,), cap, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.einx_lightglue_flash_ws_bytes(B, cap, cap, d, heads, d, layers)), dtype=torch.uint8, device=dev)
        m0, m1 = (torch.empty((B, cap), dtype=torch.int64, device=dev) for _ in range(2))
        s0, s1 = (torch.empty((B, cap), dtype=torch.float32, device=dev) for _ in range(2))
        la = torch.empty((B, cap + 1, cap + 1), dtype=torch.float32, device=dev)
        ref0, ref1 = (torch.empty((B, cap, d), dtype=torch.float32, device=dev) for _ in range(2))
        stream = N._stream(la)
        inputs = (p(kpts[0]), p(desc[0]), p(cnt), cap, p(kpts[1]), p(desc[1]), p(cnt), cap, B, 260.0, 346.0, 260.0, 346.0, p(ws))
        outs = (p(m0), p(m1), p(s0), p(s1), p(la), p(ref0), p(ref1))
        qkv = torch.randn((2 * B, cap, 2 * d), generator=g).to(dev)  # q | v side by side, as the merged to_qk | to_v buffer
        ctx = torch.empty((2 * B, cap, d), dtype=torch.float32, device=dev)
        cnt2 = torch.full((2 * B,), cap, dtype=torch.int32, device=dev)
        dense = qkv[:, :, :d].contiguous()

        def fp32():
            N.check(L.einx_lightglue(ctypes.byref(w), *inputs, *outs, 1, stream), "einx_lightglue")

        def flash():
            N.check(L.einx_lightglue_flash(ctypes.byref(w), None, ctypes.sizeof(_lib.LgHead), -1.0, -1.0, 0, *inputs, *outs, 1, None, None, None, None,
                                           None, None, stream), "einx_lightglue_flash")

        def attn_f16():
            for _ in range(layers):
                N.check(L.einx_lg_attention_f16(p(dense), p(dense), p(dense), p(ctx), p(cnt2), p(cnt2), cap, cap, 2 * B, heads, d // heads, d, 0, stream),
                        "einx_lg_attention_f16")
                N.check(L.einx_lg_attention_f16(p(qkv), p(qkv), ctypes.c_void_p(qkv.data_ptr() + 4 * d), p(ctx), p(cnt2), p(cnt2), cap, cap, 2 * B, heads,
                                                d // heads, 2 * d, B, stream), "einx_lg_attention_f16")

        variants = {"fp32_a": fp32, "flash": flash, "attn_f16": attn_f16, "fp32_b": fp32}
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
        fp32_ms = 0.5 * (med["fp32_a"] + med["fp32_b"])
        spread = abs(med["fp32_a"] - med["fp32_b"])
        attn_flop = 4.0 * d * cap * cap * 4 * layers * B
        line = {"B": B, "cap": cap, "d": d, "iters": a.iters, "ms_median": med, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
                "ms_max": {k: float(np.max(v)) for k, v in times.items()}, "fp32_ms": fp32_ms, "fp32_run_to_run_spread_ms": spread,
                "flash_faster_by_ms": fp32_ms - med["flash"], "flash_faster_by_more_than_spread": bool(fp32_ms - med["flash"] > spread),
                "pairs_per_s": {"fp32": 1e3 * B / fp32_ms, "flash": 1e3 * B / med["flash"]},
                "attention_gflop_per_forward": attn_flop / 1e9, "attn_f16_tflops": attn_flop / med["attn_f16"] / 1e9,
                "attn_f16_fraction_of_f16_mfma_peak": attn_flop / med["attn_f16"] / 1e9 / F16_MFMA_PEAK_TFLOPS}
        print(json.dumps(line))


if __name__ == "__main__":
    main()
