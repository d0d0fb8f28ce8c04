#!/usr/bin/env python3
"""Device time of LightGlue with early stopping (einx_lightglue_early_stop) against the full-depth einx_lightglue, on
the shipped model (d = 256, 4 x 64, 9 layers) at B pairs of cap x cap keypoints.  Variants, timed ALTERNATELY in one process (one
call of each per round, device events around the call, outputs and workspace allocated once; median over the rounds):

    parent_a / parent_b   einx_lightglue, twice in every round: the distance of the two medians is the run-to-run spread.  With
                          --parent-lib the symbol is taken from that library (a build of the parent commit), else from this build
    never                 the new op with nothing stopping (every token bias at -30: no confidence reaches its threshold)
    stop1 / stop3 / stop5 the new op with every pair stopping there (token bias +30 at that layer, -30 before it)

    python tools/lg_early_stop_bench.py [--B 64 1] [--cap 1024] [--iters 15] [--parent-lib PATH]   (output: profiles/lg_early_stop_bench.txt)
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
DEPTH = 0.5


def model_for(pkg, sd, stop, dev):
    """the shipped model with its token biases set so that every pair stops after `stop` layers (None: never)"""
    sd = dict(sd)
    for i in range(8):
        v = 30.0 if stop is not None and i == stop - 1 else -30.0
        sd[f"token_confidence.{i}.token.0.bias"] = np.full((1,), v, np.float32)
    lg = pkg.LightGlue({"depth_confidence": DEPTH}).to(dev)
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return lg.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    from helpers import lgf64_shipped_state_dict, load_pkg
    pkg = load_pkg()
    N = pkg.native
    _lib = importlib.import_module(pkg.__name__ + "._lib")
    L = N.lib()
    parent = L
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        parent.einx_lightglue.restype, parent.einx_lightglue.argtypes = _lib.SIGNATURES["einx_lightglue"]
    dev = "cuda:0"
    sd = lgf64_shipped_state_dict(7)
    stops = (None, 1, 3, 5)
    models = {s: model_for(pkg, sd, s, dev) for s in stops}
    p = N._ptr
    for B in a.B:
        cap, d = a.cap, 256
        g = torch.Generator().manual_seed(5 + B)
        desc = [torch.nn.functional.normalize(torch.randn((B, cap, d), generator=g), dim=-1).to(dev) for _ in range(2)]
        kpts = [(torch.rand((B, cap, 3), generator=g) * torch.tensor([260.0, 346.0, 1.0])).to(dev) for _ in range(2)]
        cnt = torch.full((B,), cap, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.einx_lightglue_early_stop_ws_bytes(B, cap, cap, d, 4, d, 9)), dtype=torch.uint8, device=dev)
        m0, m1 = (torch.empty((B, cap), dtype=torch.int64, device=dev) for _ in range(2))
        s0, s1 = (torch.empty((B, cap), dtype=torch.float32, device=dev) for _ in range(2))
        la = torch.empty((B, cap + 1, cap + 1), dtype=torch.float32, device=dev)
        ref0, ref1 = (torch.empty((B, cap, d), dtype=torch.float32, device=dev) for _ in range(2))
        stop = torch.empty((B,), dtype=torch.int32, device=dev)
        stream = N._stream(la)
        inputs = (p(kpts[0]), p(desc[0]), p(cnt), cap, p(kpts[1]), p(desc[1]), p(cnt), cap, B, 260.0, 346.0, 260.0, 346.0, p(ws))
        outs = (p(m0), p(m1), p(s0), p(s1), p(la), p(ref0), p(ref1))

        def full(lib, w):
            return lambda: N.check(lib.einx_lightglue(ctypes.byref(w), *inputs, *outs, 1, stream), "einx_lightglue")

        def early(pack):
            w, _, _, heads = pack
            return lambda: N.check(L.einx_lightglue_early_stop(ctypes.byref(w), heads, ctypes.sizeof(_lib.LgHead), DEPTH, *inputs, *outs, p(stop),
                                                               stream), "einx_lightglue_early_stop")

        w_full = models[None]._pack()[0]
        variants = {"parent_a": full(parent, w_full), "never": early(models[None]._pack())}
        for s in stops[1:]:
            variants[f"stop{s}"] = early(models[s]._pack())
        variants["parent_b"] = full(parent, w_full)
        expect = {"never": 9, "stop1": 1, "stop3": 3, "stop5": 5}
        for name, fn in variants.items():  # warm-up, and the forced depth is the depth that ran
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            if name in expect:
                assert stop.tolist() == [expect[name]] * B, (name, stop.tolist()[:4])
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
        parent_ms = 0.5 * (med["parent_a"] + med["parent_b"])
        spread = abs(med["parent_a"] - med["parent_b"])
        line = {"B": B, "cap": cap, "d": d, "iters": a.iters, "parent_lib": a.parent_lib or "this build",
                "ms_median": med, "ms_min": {k: float(np.min(v)) for k, v in times.items()}, "ms_max": {k: float(np.max(v)) for k, v in times.items()},
                "parent_ms": parent_ms, "parent_run_to_run_spread_ms": spread,
                "never_stopping_overhead_ms": med["never"] - parent_ms,
                "ms_per_layer_skipped": {f"stop{s}": (med["never"] - med[f"stop{s}"]) / (9 - s) for s in stops[1:]},
                "stop3_faster_than_parent_by_ms": parent_ms - med["stop3"],
                "stop3_faster_than_parent_by_more_than_spread": bool(parent_ms - med["stop3"] > spread)}
        print(json.dumps(line))


if __name__ == "__main__":
    main()
