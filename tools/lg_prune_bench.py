#!/usr/bin/env python3
"""Device time of LightGlue with point pruning (einx_lightglue_adaptive) against the full-width einx_lightglue of the
parent commit, on the shipped model (d = 256, 4 x 64, 9 layers) at B pairs of cap x cap keypoints.  Op level only (N.lightglue's C
entry points; no EIM).  Two child processes per shape, one after the other, each timing its variants ALTERNATELY (one call of each
per round, device events around the call, outputs and workspace allocated once; median over the rounds after 2 warm-up calls):

    parent process   parent_a / parent_b: einx_lightglue from --parent-lib (a build of the parent commit), twice in every round: the
                     distance of the two medians is the parent's run-to-run spread
    new process      keep_all: the new op with the switch on and nothing pruned (every matchability bias at +30): the overhead of
                     the decision and compaction launches
                     half / three_quarters: that share of each side pruned after the FIRST layer and nothing later: the bias of
                     layer 0 is set to minus the pooled median / upper quartile of its own logits on the inputs
                     (width_confidence 0.5: keep logit > 0); the share is checked in `live`
                     parent_here_a / full / parent_here_b: the parent's einx_lightglue, this build's, the parent's again, in
                     this process (einx_lightglue itself is unchanged; its place in the round is not the parent process's)
    No variant asks for log_assignment (the new op does not produce it).

    python tools/lg_prune_bench.py --parent-lib PATH [--B 64 1] [--cap 1024 2048] [--iters 15] [--out profiles/lg_prune_bench.txt]
"""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WIDTH = 0.5
SHARES = {"half": 0.5, "three_quarters": 0.75}


def inputs_for(B, cap, d, dev):
    import torch
    g = torch.Generator().manual_seed(5 + B + cap)
    desc = [torch.nn.functional.normalize(torch.randn((B, cap, d), generator=g), dim=-1).to(dev) for _ in range(2)]
    kpts = [(torch.rand((B, cap, 3), generator=g) * torch.tensor([260.0, 346.0, 1.0])).to(dev) for _ in range(2)]
    return desc, kpts


def model_for(pkg, sd, bias0, dev):
    """the shipped model with matchability biases that keep every row (+30), but for layer 0 when `bias0` is given"""
    import torch
    sd = dict(sd)
    for i in range(9):
        sd[f"log_assignment.{i}.matchability.bias"] = np.full((1,), 30.0 if (i or bias0 is None) else bias0, np.float32)
    lg = pkg.LightGlue({"width_confidence": WIDTH}).to(dev)
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return lg.eval()


def time_variants(variants, iters, check=None):
    import torch
    for name, fn in variants.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        if check:
            check(name)
    times = {k: [] for k in variants}
    for _ in range(iters):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return {"ms_median": {k: float(np.median(v)) for k, v in times.items()}, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
            "ms_max": {k: float(np.max(v)) for k, v in times.items()}}


def child(a):
    import torch
    from helpers import lgf64_shipped_state_dict, load_pkg
    pkg = load_pkg()
    N = pkg.native
    _lib = importlib.import_module(pkg.__name__ + "._lib")
    _batched = importlib.import_module(pkg.__name__ + ".core.modules.matchers._batched")
    L = N.lib()
    dev = "cuda:0"
    B, cap, d = a.B[0], a.cap[0], 256
    sd = lgf64_shipped_state_dict(7)
    desc, kpts = inputs_for(B, cap, d, dev)
    cnt = torch.full((B,), cap, dtype=torch.int32, device=dev)
    p = N._ptr
    ws = torch.empty(int(L.einx_lightglue_adaptive_ws_bytes(B, cap, cap, d, 4, d, 9)), dtype=torch.uint8, device=dev)
    m0, m1 = (torch.empty((B, cap), dtype=torch.int64, device=dev) for _ in range(2))
    s0, s1 = (torch.empty((B, cap), dtype=torch.float32, device=dev) for _ in range(2))
    ref0, ref1 = (torch.empty((B, cap, d), dtype=torch.float32, device=dev) for _ in range(2))
    stream = N._stream(ref0)
    inputs = (p(kpts[0]), p(desc[0]), p(cnt), cap, p(kpts[1]), p(desc[1]), p(cnt), cap, B, 260.0, 346.0, 260.0, 346.0, p(ws))
    keep_all = model_for(pkg, sd, None, dev)

    def full(lib, w, la):
        return lambda: N.check(lib.einx_lightglue(ctypes.byref(w), *inputs, p(m0), p(m1), p(s0), p(s1), p(la), p(ref0), p(ref1), 1, stream),
                               "einx_lightglue")

    if a.role == "parent":
        parent = ctypes.CDLL(a.parent_lib)
        parent.einx_lightglue.restype, parent.einx_lightglue.argtypes = _lib.SIGNATURES["einx_lightglue"]
        w = keep_all._pack()[0]
        out = time_variants({"parent_a": full(parent, w, None), "parent_b": full(parent, w, None)}, a.iters)
        print(json.dumps(dict(role="parent", B=B, cap=cap, **out)))
        return
    # layer 0's matchability logits on (at most four of) these pairs, from the existing op's per-layer descriptors
    nb = min(B, 4)
    pbs = []
    for s in range(2):
        pb = _batched.PairBatch()
        pb.kpts, pb.desc, pb.counts = kpts[s][:nb].contiguous(), desc[s][:nb].contiguous(), cnt[:nb].contiguous()
        pb.cap, pb.B, pb.image_size, pb.counts_host = cap, nb, (260, 346), None
        pbs.append(pb)
    r = N.lightglue(keep_all._pack()[0], pbs[0], pbs[1], want_la=False, want_ref=True, all_layers=True)
    wm = keep_all.log_assignment[0].matchability.weight[0]
    z = torch.cat([r.ref0[:, 0].reshape(-1, d) @ wm, r.ref1[:, 0].reshape(-1, d) @ wm])
    del r
    models = {"keep_all": keep_all}
    for name, share in SHARES.items():
        models[name] = model_for(pkg, sd, -float(torch.quantile(z, share)), dev)
    prune0, prune1 = (torch.empty((B, cap), dtype=torch.float32, device=dev) for _ in range(2))
    kept0, kept1 = (torch.empty((B, cap), dtype=torch.int64, device=dev) for _ in range(2))
    live = torch.empty((2 * B,), dtype=torch.int32, device=dev)

    def adaptive(lg):
        w, _, _, heads = lg._pack()
        return lambda: N.check(L.einx_lightglue_adaptive(ctypes.byref(w), heads, ctypes.sizeof(_lib.LgHead), -1.0, WIDTH, 0, *inputs, p(m0), p(m1),
                                                         p(s0), p(s1), None, p(ref0), p(ref1), None, p(prune0), p(prune1), p(kept0), p(kept1),
                                                         p(live), stream), "einx_lightglue_adaptive")

    variants = {name: adaptive(lg) for name, lg in models.items()}
    # this build's einx_lightglue between two series of the parent's, in THIS process: the three share their place in the round
    parent = ctypes.CDLL(a.parent_lib)
    parent.einx_lightglue.restype, parent.einx_lightglue.argtypes = _lib.SIGNATURES["einx_lightglue"]
    variants["parent_here_a"] = full(parent, keep_all._pack()[0], None)
    variants["full"] = full(L, keep_all._pack()[0], None)
    variants["parent_here_b"] = full(parent, keep_all._pack()[0], None)
    seen = {}

    def check(name):
        if name not in models:
            return
        lv = live.float() / cap
        seen[name] = [float(lv.min()), float(lv.mean()), float(lv.max())]
        want = 1.0 - SHARES.get(name, 0.0)
        assert abs(seen[name][1] - want) <= 0.02 and seen[name][0] >= want - 0.1 and seen[name][2] <= want + 0.1, (name, seen[name])

    out = time_variants(variants, a.iters, check)
    print(json.dumps(dict(role="new", B=B, cap=cap, live_share_min_mean_max=seen, **out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--cap", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lg_prune_bench.txt"))
    ap.add_argument("--role", choices=("parent", "new"), default=None)
    a = ap.parse_args()
    if a.role:
        return child(a)
    lines = []
    for cap in a.cap:
        for B in a.B:
            res = {}
            for role in ("parent", "new"):  # a fresh child process each; this process never opens the device
                cmd = [sys.executable, os.path.abspath(__file__), "--role", role, "--B", str(B), "--cap", str(cap), "--iters", str(a.iters),
                       "--parent-lib", a.parent_lib]
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if done.returncode != 0:
                    sys.stderr.write(done.stdout + done.stderr)
                    raise SystemExit(f"lg_prune_bench: the {role} process failed ({done.returncode}); nothing more is started")
                res[role] = json.loads(done.stdout.strip().splitlines()[-1])
            pm, nm = res["parent"]["ms_median"], res["new"]["ms_median"]
            parent_ms, spread = 0.5 * (pm["parent_a"] + pm["parent_b"]), abs(pm["parent_a"] - pm["parent_b"])
            line = {"B": B, "cap": cap, "d": 256, "iters": a.iters, "parent": res["parent"], "new": res["new"], "parent_ms": parent_ms,
                    "parent_run_to_run_spread_ms": spread, "keep_all_overhead_ms": nm["keep_all"] - parent_ms,
                    "faster_than_parent_by_ms": {k: parent_ms - nm[k] for k in SHARES},
                    "half_faster_than_parent_by_more_than_spread": bool(parent_ms - nm["half"] > spread)}
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
