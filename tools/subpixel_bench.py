#!/usr/bin/env python3
"""What the opt-in sub-pixel keypoints cost: SP+MNN forwards with `subpixel` off against on, in ONE process.

Legs: 32 pairs (EIM.forward), a single pair (EIM.forward) and a single pair through EIM.forward_graph.  Two models on the same
weights and inputs, one with `subpixel = True` on both extractors.  Per round one call of off, one of on and a second one of off,
a host clock around each call up to a device synchronise; medians over the rounds after a warm-up of every variant.  The distance
of the two "off" medians is the run-to-run spread that a difference has to exceed to mean anything.

--off-only times the two "off" variants alone; --root points at another checkout of the package (one without the switch, say),
so that its "off" time can be taken by the same script, in the same call, on the same machine.

    python tools/subpixel_bench.py [--rounds 30] [--rounds-b1 200] [--off-only] [--root DIR] [--label NAME]
    (output: profiles/subpixel_bench.txt)
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np


def timed(variants, rounds, sync):
    for fn in variants.values():
        for _ in range(3):
            fn()
    sync()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            sync()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: float(np.median(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--rounds-b1", type=int, default=200)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fall-back"
    pkg = importlib.import_module("ei-nexus_official_amd")
    bench = importlib.import_module("bench")
    dev = "cuda:0"
    sync = torch.cuda.synchronize

    for B, graph, rounds in ((32, False, a.rounds), (1, False, a.rounds_b1), (1, True, a.rounds_b1)):
        off = bench.Workload(pkg, dev, "sp_mnn", B, calibrate=True)
        step = (lambda w: (lambda: w.model.forward_graph(w.ev, w.img_src, w.mask))) if graph else (lambda w: w.step)
        variants = {"off_a": step(off)}
        on = None
        if not a.off_only:
            on = bench.Workload(pkg, dev, "sp_mnn", B, calibrate=False)
            on.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in off.sd.items()}, strict=False)
            for ext in (on.model.event_extractor.extractor, on.model.image_extractor.extractor):
                ext.subpixel = True
                assert ext.keypoint_mode == "subpixel"
            variants["on"] = step(on)
        variants["off_b"] = step(off)
        med = timed(variants, rounds, sync)
        off_ms, spread = 0.5 * (med["off_a"] + med["off_b"]), abs(med["off_a"] - med["off_b"])
        row = {"tree": a.label, "forward": "sp_mnn", "B": B, "mode": "forward_graph" if graph else "forward", "rounds": rounds,
               "off_ms": round(off_ms, 4), "off_spread_ms": round(spread, 4), "off_a_ms": round(med["off_a"], 4), "off_b_ms": round(med["off_b"], 4)}
        if on is not None:
            e0, i0, m0 = off.step()
            e1, i1, m1 = on.step()
            moved = float(np.mean([float((p1[:, :2] - p0[:, :2]).abs().max()) for p0, p1 in zip(e0["sparse_positions"], e1["sparse_positions"])]))
            row.update({"on_ms": round(med["on"], 4), "on_minus_off_ms": round(med["on"] - off_ms, 4),
                        "on_beyond_spread": bool(abs(med["on"] - off_ms) > spread), "mean_of_largest_offset_px": round(moved, 4),
                        "mean_matches": {"off": float(np.mean([int(t.shape[0]) for t in m0["matched_kpts0"]])),
                                         "on": float(np.mean([int(t.shape[0]) for t in m1["matched_kpts0"]]))}})
        print(json.dumps(row), flush=True)
        del off, on, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
