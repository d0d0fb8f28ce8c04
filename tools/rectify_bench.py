#!/usr/bin/env python3
"""Time of rectifying a resident event stream (csrc/rectify.hip einx_events_remap, datasets/rectify.py): N synthetic
time-sorted events on a 260 x 346 sensor under the MVSEC rule, with a fisheye map whose border leaves the bounds, against the same
rule written two other ways:

    torch    map[oy, ox] with torch operators on the same device, a boolean mask and four masked selects
    numpy    the reference's form (datasets/MVSEC_rectify.py:23-45) on the host, on host copies of the same arrays

The three results are compared bit for bit before anything is timed.  Medians of `--runs` runs after a warm-up; device times from
device events around the call, `rectify_events` and numpy from a host clock (the former ends in its read-back).  The share of HBM
bandwidth is over the ALGORITHMIC bytes: 20 B read per event and 20 B written per kept event.

    python tools/rectify_bench.py [--events 100000000] [--runs 7] [--numpy-runs 7] [--out profiles/rectify_bench.txt]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12  # bytes / s: measured float4 copy, specification
H, W = 260, 346


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(times):
    return {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times)), "n": len(times)}


def torch_form(x, y, t, p, map_x, map_y):
    ox, oy = torch.round(x).long(), torch.round(y).long()
    rx, ry = map_x[oy, ox], map_y[oy, ox]
    mask = (rx >= 0) & (rx < W - 1) & (ry >= 0) & (ry < H - 1)
    return rx[mask], ry[mask], t[mask], p[mask]


def numpy_form(x, y, t, p, map_x, map_y):
    ox, oy = np.round(x).astype(np.int32), np.round(y).astype(np.int32)
    rx, ry = map_x[oy, ox], map_y[oy, ox]
    mask = (rx >= 0) & (rx < W - 1) & (ry >= 0) & (ry < H - 1)
    return rx[mask], ry[mask], t[mask], p[mask]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--numpy-runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: a timing taken anywhere else says nothing"
    pkg = importlib.import_module("ei-nexus_official_amd")
    nat = pkg.native
    rectify = importlib.import_module(pkg.__name__ + ".datasets.rectify")

    # an MVSEC-like map: the fisheye model with the sensor's intrinsics, projected with a longer focal length, so that the
    # border of the sensor maps outside the bounds as it does in the dataset's own event maps
    K, D = (199.65, 199.65, 177.4, 126.8), (-0.048, 0.0113, -0.0553, 0.0399)
    P = np.array([[226.38, 0.0, 173.65], [0.0, 226.15, 133.73], [0.0, 0.0, 1.0]])
    c, s = np.cos(0.01), np.sin(0.01)
    map_x, map_y = rectify.fisheye_rectify_map(K, D, np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), P, (W, H), device=DEV)
    # the map as an event map: stretched about the centre so that pixels near the border leave the bounds (the kept share is reported)
    map_x = ((map_x - W / 2) * 1.25 + W / 2).contiguous()
    map_y = ((map_y - H / 2) * 1.25 + H / 2).contiguous()

    n = a.events
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randint(0, W, (n,), generator=g, device=DEV).float()
    y = torch.randint(0, H, (n,), generator=g, device=DEV).float()
    p = torch.randint(0, 2, (n,), generator=g, device=DEV).float()
    t = torch.cumsum(torch.rand(n, generator=g, device=DEV, dtype=torch.float64) * 2e-6, 0) + 1.5e9
    seq = pkg.EventSequence.from_tensors(x, y, t, p)
    del x, y, t, p

    # the same bits three ways
    res = rectify.rectify_events(seq, map_x, map_y, "mvsec")
    tx, ty, tt, tp = torch_form(seq.x, seq.y, seq.t, seq.p, map_x, map_y)
    same_torch = all(torch.equal(u, v) for u, v in ((res.x, tx), (res.y, ty), (res.t, tt), (res.p, tp)))
    del tx, ty, tt, tp
    hx, hy, ht, hp = (v.cpu().numpy() for v in (seq.x, seq.y, seq.t, seq.p))
    hmx, hmy = map_x.cpu().numpy(), map_y.cpu().numpy()
    nx, ny, nt, npol = numpy_form(hx, hy, ht, hp, hmx, hmy)
    same_numpy = all(np.array_equal(u.cpu().numpy().view(np.uint8), v.view(np.uint8)) for u, v in ((res.x, nx), (res.y, ny), (res.t, nt), (res.p, npol)))
    assert same_torch and same_numpy, (same_torch, same_numpy)
    kept = res.kept
    del res, nx, ny, nt, npol

    bounds = (float(W - 1), float(H - 1))
    out = nat.events_remap(seq.x, seq.y, seq.t, seq.p, map_x, map_y, *bounds)
    op = lambda: nat.events_remap(seq.x, seq.y, seq.t, seq.p, map_x, map_y, *bounds, out=out)  # noqa: E731
    full = lambda: rectify.rectify_events(seq, map_x, map_y, "mvsec")  # noqa: E731
    tf = lambda: torch_form(seq.x, seq.y, seq.t, seq.p, map_x, map_y)  # noqa: E731
    for _ in range(2):
        op(), full(), tf()
    torch.cuda.synchronize()
    t_op, t_full, t_torch = [], [], []
    for _ in range(a.runs):  # alternating
        t_op.append(event_ms(op))
        t_torch.append(event_ms(tf))
        t_full.append(host_ms(full))
    t_np = []
    for i in range(a.numpy_runs + 1):
        t0 = time.perf_counter()
        numpy_form(hx, hy, ht, hp, hmx, hmy)
        if i:  # the first run is the warm-up
            t_np.append((time.perf_counter() - t0) * 1e3)

    algorithmic = 20 * n + 20 * kept
    line = {"events": n, "kept": kept, "kept_share": kept / n, "sensor": [H, W], "rule": "mvsec", "bit_equal_to_torch_and_numpy": True,
            "einx_events_remap": stats(t_op), "torch_composition": stats(t_torch), "rectify_events_with_read_back": stats(t_full),
            "numpy_on_the_host": stats(t_np) if t_np else None,
            "algorithmic_bytes": algorithmic, "bytes_moved_by_the_three_passes": 28 * n + 20 * kept}
    sec = line["einx_events_remap"]["ms_median"] * 1e-3
    line["events_per_s"] = n / sec
    line["algorithmic_bytes_per_s"] = algorithmic / sec
    line["share_of_achievable_hbm_6.3TBps"] = algorithmic / sec / HBM_ACHIEVABLE
    line["share_of_peak_hbm_8TBps"] = algorithmic / sec / HBM_PEAK
    line["speedup_over_torch"] = line["torch_composition"]["ms_median"] / line["einx_events_remap"]["ms_median"]
    if t_np:
        line["speedup_over_numpy"] = line["numpy_on_the_host"]["ms_median"] / line["einx_events_remap"]["ms_median"]
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/rectify_bench.py --events {a.events} --runs {a.runs} --numpy-runs {a.numpy_runs}\n")
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
