#!/usr/bin/env python3
"""Device time of the event representations (csrc/event_reps.hip and, as the yardstick, einx_voxel_grid): B samples of n events
at 346 x 260, inputs already on the device, every named op timed in the SAME run with device events around the whole launch
sequence of one call.  Events: integer pixel coordinates, sorted stamps, p in {-1, +1} (pkg.synth.synth_raw_events).

    python tools/representation_bench.py {TimeSurface,EventStack,EventDistanceMap,VoxelGrid} ... [--B 32] [--bins 5 16] [--events 60000]
                                         [--iters 30] [--evaluator STEPS]

--evaluator STEPS: also SameTimeEvaluator.run (SP + MNN, raw host events -> metrics) pairs/s once per named representation_type.
One JSON line per (op, bins); `x_voxel` is the op's median over the voxel grid's of the same run.
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OPS = {"TimeSurface": "time_surface", "EventStack": "event_stack", "EventDistanceMap": "distance_map", "VoxelGrid": "voxel"}
H, W = 260, 346


def op_times(pkg, rep, names, B, bins, events, iters):
    L, N = pkg.native.lib(), pkg.native
    x, y, t, p, offs = rep._pack(events, "cuda:0")
    out = torch.empty((B, bins, H, W), dtype=torch.float32, device="cuda:0")
    op = offs.ctypes.data_as(ctypes.c_void_p)
    res = {}
    for name in names:
        sym = OPS[name]
        ws = torch.empty(getattr(L, f"einx_{sym}_ws_bytes")(B, bins, H, W, int(offs[-1])), dtype=torch.uint8, device="cuda:0")
        head = (N._ptr(x), N._ptr(y), N._ptr(t), N._ptr(p), op, B, bins, H, W)
        tail = (N._ptr(out), N._ptr(ws), ws.numel(), N._stream(out))
        if name == "VoxelGrid":
            call = lambda: L.einx_voxel_grid(*head, 1, *tail)  # noqa: E731  (normalised: what the evaluators build)
        else:
            call = lambda fn=getattr(L, f"einx_{sym}"): fn(*head, *tail)  # noqa: E731
        for _ in range(5):
            assert call() == 0, name
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        res[name] = ms
    return res


def evaluator_rate(pkg, name, B, bins, events, steps):
    cfg = pkg.default_config("SP_MNN", event_channels=bins)
    model = pkg.EIM(cfg, device="cuda:0").eval()
    sd = pkg.synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    img = torch.from_numpy(pkg.synth.synth_image(9, B, H, W)).to("cuda:0")
    ev = pkg.SameTimeEvaluator(model, bins, (W, H), representation_type=name)

    def feed(n):
        for _ in range(n):
            yield events, img.clone()  # SuperPoint scales its image in place

    for _ in ev.run(feed(3)):
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in ev.run(feed(steps)):
        pass
    torch.cuda.synchronize()
    return B * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ops", nargs="+", choices=sorted(OPS))
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--bins", type=int, nargs="+", default=[5, 16])
    ap.add_argument("--events", type=int, default=60000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--evaluator", type=int, default=0, metavar="STEPS")
    a = ap.parse_args()
    from helpers import load_pkg
    pkg = load_pkg()
    rep = importlib.import_module(pkg.__name__ + ".datasets.representations")
    events = [pkg.synth.synth_raw_events(5000 + b, a.events) for b in range(a.B)]
    for bins in a.bins:
        times = op_times(pkg, rep, a.ops, a.B, bins, events, a.iters)
        vox = float(np.median(times["VoxelGrid"])) if "VoxelGrid" in times else None
        for name, ms in times.items():
            line = {"op": name, "B": a.B, "bins": bins, "events_per_sample": a.events, "ms_median": round(float(np.median(ms)), 4),
                    "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4), "iters": a.iters}
            if vox:
                line["x_voxel"] = round(line["ms_median"] / vox, 2)
            print(json.dumps(line), flush=True)
    if a.evaluator:
        for name in a.ops:
            rate = evaluator_rate(pkg, name, a.B, a.bins[0], events, a.evaluator)
            print(json.dumps({"SameTimeEvaluator.run": name, "B": a.B, "bins": a.bins[0], "steps": a.evaluator, "pairs_per_s": round(rate, 1)}),
                  flush=True)


if __name__ == "__main__":
    main()
