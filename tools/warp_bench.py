#!/usr/bin/env python3
"""Time of the perspective warp (csrc/warp.hip einx_warp_perspective, datasets/warp.py) at the evaluators' batch:
32 x 1 x 260 x 346 images, float32 and uint8, one sampled homography per image (core.geometry.homography.sample_homographies,
difficulty 0.7), against the same warp written with torch on the same device:

    grid_sample    the source points formed with torch operators in float64 from the same H^-1, then
                   F.grid_sample(float32, align_corners=False, padding_mode="zeros") -- timed with and without forming the grid

and one evaluator step (SP + MNN, synthetic weights, 32 pairs of 20 000 raw events) as SameTimeEvaluator runs it under the identity
and as HomographicEvaluator runs it: the difference is what the warp, the mask, the labels and match_pr add to a batch.

The float32 result is compared with grid_sample's before anything is timed (valid pixels, 1e-3 of 255: grid_sample computes its
weights from a float32 grid).  Medians of `--runs` runs after a warm-up, device events around the calls for the ops, a host clock
that ends in a synchronise for the steps.  The share of HBM bandwidth is over the ALGORITHMIC bytes (every source and destination
pixel once, one flag per pixel); at this size the op is a launch, not a stream, and the figure says so.

    python tools/warp_bench.py [--batch 32] [--runs 21] [--step-runs 9] [--out profiles/warp_bench.txt]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
HBM_ACHIEVABLE = 6.3e12  # bytes / s: measured float4 copy
H, W = 260, 346


def event_ms(fn, reps=20):
    """mean of `reps` back-to-back calls between two device events: one call is too short for the events' resolution"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(times):
    return {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times)), "n": len(times)}


def torch_grid(Hinv, Hd, Wd, Hs, Ws):
    """the normalised sampling grid [B,Hd,Wd,2] float32 and the validity rule, with torch operators in float64"""
    h = Hinv.reshape(-1, 9)[:, :, None, None]
    x = (torch.arange(Wd, device=Hinv.device, dtype=torch.float64) + 0.5)[None, None, :]
    y = (torch.arange(Hd, device=Hinv.device, dtype=torch.float64) + 0.5)[None, :, None]
    w = (h[:, 6] * x + h[:, 7] * y) + h[:, 8]
    qx, qy = ((h[:, 0] * x + h[:, 1] * y) + h[:, 2]) / w, ((h[:, 3] * x + h[:, 4] * y) + h[:, 5]) / w
    valid = torch.isfinite(w) & (w > 0) & (qx >= 0.5) & (qx <= Ws - 0.5) & (qy >= 0.5) & (qy <= Hs - 0.5)
    grid = torch.stack([2.0 * qx / Ws - 1.0, 2.0 * qy / Hs - 1.0], -1).float()
    return grid, valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--step-runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: a timing taken anywhere else says nothing"
    pkg = importlib.import_module("ei-nexus_official_amd")
    nat, synth = pkg.native, pkg.synth
    warp = importlib.import_module(pkg.__name__ + ".datasets.warp")
    hom = importlib.import_module(pkg.__name__ + ".core.geometry.homography")
    B = a.batch

    Hm = hom.sample_homographies(B, (W, H), rng=np.random.RandomState(1), difficulty=0.7)
    Hinv = warp.invert_homography(torch.from_numpy(Hm)).reshape(B, 9).to(DEV).contiguous()
    f32 = torch.from_numpy(synth.synth_image(3, B, H, W)).to(DEV)
    u8 = f32.to(torch.uint8)

    got, valid = nat.warp_perspective(f32, Hinv, H, W)
    grid, gvalid = torch_grid(Hinv, H, W, H, W)
    ref = F.grid_sample(f32, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    both = (valid.bool() & gvalid)[:, None]
    diff = float((got - ref)[both].abs().max())
    flags = int((valid.bool() != gvalid).sum())
    assert diff <= 1e-3 * 255 and flags <= 1e-5 * valid.numel(), (diff, flags)

    ops = {
        "einx_warp_perspective float32": lambda: nat.warp_perspective(f32, Hinv, H, W),
        "einx_warp_perspective uint8": lambda: nat.warp_perspective(u8, Hinv, H, W),
        "einx_warp_perspective float32, no valid output": lambda: nat.warp_perspective(f32, Hinv, H, W, want_valid=False),
        "warp_perspective (Python layer: inverse on the host, one upload) float32": lambda: warp.warp_perspective(f32, Hm),
        "F.grid_sample float32, grid given": lambda: F.grid_sample(f32, grid, mode="bilinear", padding_mode="zeros", align_corners=False),
        "torch grid + validity + F.grid_sample float32": lambda: F.grid_sample(f32, torch_grid(Hinv, H, W, H, W)[0], mode="bilinear",
                                                                               padding_mode="zeros", align_corners=False),
    }
    times = {k: [] for k in ops}
    for fn in ops.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.runs):  # alternating
        for k, fn in ops.items():
            times[k].append(event_ms(fn))

    # one evaluator step with and without the warp
    cfg = pkg.default_config("SP_MNN", event_channels=5)
    model = pkg.EIM(cfg, device=DEV).eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=11)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    rng = np.random.RandomState(7)
    n_ev = 20000
    evs = [{"x": rng.randint(0, W, n_ev).astype(np.float32), "y": rng.randint(0, H, n_ev).astype(np.float32),
            "t": 1.5e9 + np.cumsum(rng.uniform(1e-6, 1e-4, n_ev)), "p": rng.randint(0, 2, n_ev).astype(np.float32)} for _ in range(B)]
    img = synth.synth_image(5, B, H, W)
    eye = torch.eye(3, device=DEV)[None].repeat(B, 1, 1)
    srng = np.random.RandomState(2)
    same = pkg.SameTimeEvaluator(model, bins=5, resolution=(W, H), he_thresh=(3, 5, 10))
    homo = pkg.HomographicEvaluator(model, bins=5, resolution=(W, H), he_thresh=(3, 5, 10),
                                    sampler=lambda b, shape: hom.sample_homographies(b, shape, rng=srng, difficulty=0.7))
    steps = {"SameTimeEvaluator.step, identity": lambda: same.step(evs, torch.from_numpy(img).to(DEV), eye),
             "HomographicEvaluator.step": lambda: homo.step(evs, torch.from_numpy(img).to(DEV))}
    step_times = {k: [] for k in steps}
    t_sampler = []
    for fn in steps.values():
        for _ in range(2):
            fn()
    for _ in range(a.step_runs):  # alternating
        for k, fn in steps.items():
            step_times[k].append(host_ms(fn))
        t0 = time.perf_counter()
        hom.sample_homographies(B, (W, H), rng=srng, difficulty=0.7)
        t_sampler.append((time.perf_counter() - t0) * 1e3)

    px = B * H * W
    line = {"batch": B, "shape": [B, 1, H, W], "difficulty": 0.7, "valid_share": float(valid.float().mean()),
            "max_abs_diff_to_grid_sample_on_valid_pixels": diff, "validity_flags_that_differ": flags,
            "ops": {k: stats(v) for k, v in times.items()}, "steps": {k: stats(v) for k, v in step_times.items()},
            "sampler_on_the_host": stats(t_sampler), "algorithmic_bytes_float32": 9 * px, "algorithmic_bytes_uint8": 3 * px}
    sec = line["ops"]["einx_warp_perspective float32"]["ms_median"] * 1e-3
    line["float32_algorithmic_bytes_per_s"] = 9 * px / sec
    line["float32_share_of_achievable_hbm_6.3TBps"] = 9 * px / sec / HBM_ACHIEVABLE
    line["grid_sample_given_grid_over_einx"] = line["ops"]["F.grid_sample float32, grid given"]["ms_median"] / (sec * 1e3)
    line["torch_composition_over_einx"] = line["ops"]["torch grid + validity + F.grid_sample float32"]["ms_median"] / (sec * 1e3)
    line["step_added_ms"] = line["steps"]["HomographicEvaluator.step"]["ms_median"] - line["steps"]["SameTimeEvaluator.step, identity"]["ms_median"]
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/warp_bench.py --batch {a.batch} --runs {a.runs} --step-runs {a.step_runs}\n")
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
