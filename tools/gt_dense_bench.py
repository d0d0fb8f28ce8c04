#!/usr/bin/env python3
"""Device time of the dense-grid ground-truth matches (csrc/gt_matches.hip gt_dense_*) at B pairs of H x W depth maps
with every pixel centre of both views a keypoint -- with labels and counts only -- against the way the library could already do the
job: the generic gt_matches fed grid_keypoints, which evaluates all H W x H W point pairs.  Seeded synthetic depth with 20 % holes
(tests/gt_dense_f64.py::random_scene with holes=5: one pixel in five; the fraction is measured from the maps and reported).  The
two paths are compared bit for bit on the timed inputs before anything is timed; device events around one call each, the two
dense forms and the generic one alternating; then select_pairs' throughput on a 200-frame stack, the whole selection repeated
and timed each time.

    python tools/gt_dense_bench.py [--B 32] [--H 260] [--W 346] [--iters 20] [--generic-iters 3] [--frames 200] [--select-iters 7] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(times):
    return {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times)), "n": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--H", type=int, default=260)
    ap.add_argument("--W", type=int, default=346)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--generic-iters", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--select-iters", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: a timing taken anywhere else says nothing"
    import gt_dense_f64 as D
    from helpers import load_pkg
    name = load_pkg().__name__
    nm = importlib.import_module(name + ".core.metrics._native_metrics")
    pairs = importlib.import_module(name + ".datasets.pairs")

    c = D.random_scene(7, a.B, (a.H, a.W), (a.H, a.W), holes=5)  # the values 0, 1, 2 of 15 become holes: one pixel in five
    hole_fraction = float(np.mean([(~(d > 0)).mean() for d in (c.depth0, c.depth1)]))
    t = {k: torch.from_numpy(getattr(c, k)).to(DEV) for k in ("depth0", "depth1", "K0", "K1", "T01", "T10")}
    kp = pairs.grid_keypoints(a.H, a.W, "yx", DEV)[None].expand(a.B, -1, -1).contiguous()
    dense = lambda labels=True: nm.gt_matches_dense(t["depth0"], t["depth1"], t["K0"], t["K1"], t["T01"], t["T10"], labels=labels)  # noqa: E731
    generic = lambda: nm.gt_matches(kp, kp, None, None, t["depth0"], t["depth1"], t["K0"], t["K1"], t["T01"], t["T10"], ordering="yx")  # noqa: E731

    got, exp = dense(), generic()
    keys = ("matches0", "matches1", "matching_scores0", "matching_scores1", "proj_0to1", "proj_1to0", "depth_keypoints0", "depth_keypoints1",
            "visible0", "visible1")
    differing = {k: int((got[k].view(torch.uint8) != exp[k].view(torch.uint8)).sum()) for k in keys}
    assert not any(differing.values()), differing
    assert torch.equal(dense(False)["counts"], got["counts"])
    counts = got["counts"].cpu().numpy()
    for _ in range(3):
        dense(), dense(False)
    torch.cuda.synchronize()
    tl, tc, tg = [], [], []
    for i in range(a.iters):  # alternating, the generic form every few rounds
        tl.append(event_ms(dense))
        tc.append(event_ms(lambda: dense(False)))
        if i * a.generic_iters // a.iters != (i + 1) * a.generic_iters // a.iters:
            tg.append(event_ms(generic))
    line = {"B": a.B, "H": a.H, "W": a.W, "keypoints_per_side": a.H * a.W, "hole_fraction": hole_fraction,
            "matches_per_pair": float(counts[:, 0].mean()), "visible_per_pair": float(np.minimum(counts[:, 2], counts[:, 3]).mean()),
            "outputs_differing_from_generic": sum(differing.values()),
            "dense_labels": stats(tl), "dense_counts_only": stats(tc), "generic_gt_matches": stats(tg)}
    line["speedup_labels"] = line["generic_gt_matches"]["ms_median"] / line["dense_labels"]["ms_median"]
    line["speedup_counts_only"] = line["generic_gt_matches"]["ms_median"] / line["dense_counts_only"]["ms_median"]
    # what the dense call must move at the least: both depth maps in, per pixel 8 + 1 + 1 + 4 bytes of workspace written and read
    # back, and with labels 4 + 1 + 1 + 8 + 8 + 4 bytes of outputs
    px = 2 * a.B * a.H * a.W
    line["dense_labels_min_bytes"] = px * (4 + 2 * 14 + 26)
    line["dense_labels_GBps_of_min_bytes"] = line["dense_labels_min_bytes"] / line["dense_labels"]["ms_median"] / 1e6

    # select_pairs: frames and poses uploaded once, every frame against its next five
    if a.frames:
        s = D.random_scene(8, a.frames, (a.H, a.W), (4, 4), holes=5)
        frames = torch.from_numpy(s.depth0).to(DEV)
        K = D._kmat(0.9 * a.W, a.W / 2, a.H / 2).astype(np.float32)
        poses = np.stack([D._pose(D._rot(0.001 * k, -0.002 * k, 0.003 * k), [0.03 * k, 0.005 * k, 0.002 * k]) for k in range(a.frames)])
        idx = [(i, i + k) for i in range(a.frames) for k in range(1, 6) if i + k < a.frames]
        pairs.select_pairs(frames, K, poses, idx)  # warm-up at the timed shapes
        torch.cuda.synchronize()
        secs = []
        for _ in range(a.select_iters):
            t0 = time.perf_counter()
            r = pairs.select_pairs(frames, K, poses, idx)  # ends in the last batch's read-back
            secs.append(time.perf_counter() - t0)
        med = float(np.median(secs))
        line["select_pairs"] = {"frames": a.frames, "pairs": len(idx), "batch": 64, "kept": int(r["kept"].sum()),
                                "hole_fraction": float((~(s.depth0 > 0)).mean()), "runs": len(secs), "seconds_median": med,
                                "seconds_min": float(np.min(secs)), "seconds_max": float(np.max(secs)), "pairs_per_s_median": len(idx) / med,
                                "pairs_per_s_min": len(idx) / float(np.max(secs)), "pairs_per_s_max": len(idx) / float(np.min(secs))}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/gt_dense_bench.py --B {a.B} --H {a.H} --W {a.W} --iters {a.iters} --generic-iters {a.generic_iters} --frames {a.frames} --select-iters {a.select_iters}\n")
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
