#!/usr/bin/env python3
"""Device time of the assignment NLL behind LightGlue.loss in eval mode (einx_lg_assign_nll) at B pairs of cap x cap
keypoints of width d, against the same contract written with dense torch operators on the same device (the recomputed
log_assignment, the weights, their product and exp() as B x (n+1) x (m+1) tensors: the shape of computation the reference's
LightGlue.loss has).  Device events around one call each; the dense form is checked against the op before it is timed.

    python tools/lg_loss_bench.py [--B 64] [--cap 1024] [--d 256] [--iters 20]     (output: profiles/lg_loss_bench.txt)
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dense_baseline(head, x0, x1, gt0, gt1, assignment, loss_fn):
    """MatchAssignment (lightglue.py:365-396), NLLLoss and row_norm with dense torch operators: returns nll, nll_pos, nll_neg, row_norm"""
    pw, pb, mw, mb = head
    d = x0.shape[-1]
    md0 = torch.nn.functional.linear(x0, pw, pb) / d ** 0.25
    md1 = torch.nn.functional.linear(x1, pw, pb) / d ** 0.25
    sim = md0 @ md1.mT
    z0, z1 = torch.nn.functional.linear(x0, mw.reshape(1, -1), mb), torch.nn.functional.linear(x1, mw.reshape(1, -1), mb)
    B, n, m = sim.shape
    la = sim.new_zeros((B, n + 1, m + 1))
    la[:, :n, :m] = (torch.log_softmax(sim, 2) + torch.log_softmax(sim, 1) + torch.nn.functional.logsigmoid(z0)
                     + torch.nn.functional.logsigmoid(z1).mT)
    la[:, :n, m] = torch.nn.functional.logsigmoid(-z0[..., 0])
    la[:, n, :m] = torch.nn.functional.logsigmoid(-z1[..., 0])
    nll, _, parts = loss_fn({"log_assignment": la}, {"gt_matches0": gt0, "gt_matches1": gt1, "gt_assignment": assignment})
    return nll, parts["nll_pos"], parts["nll_neg"], la.exp()[:, :-1].sum(2).mean(1)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_max": float(np.max(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import lg_loss_ref as R
    from helpers import load_pkg, synth
    pkg = load_pkg()
    N = pkg.native
    LGM = importlib.import_module(pkg.__name__ + ".core.modules.matchers.lightglue")
    dev = "cuda:0"
    shapes = [("final_proj.weight", (a.d, a.d)), ("final_proj.bias", (a.d,)), ("matchability.weight", (1, a.d)), ("matchability.bias", (1,))]
    sd = synth.synth_state_dict(shapes, 3)
    head = tuple(torch.from_numpy(sd[k]).to(dev) for k, _ in shapes)
    g = torch.Generator().manual_seed(5)
    x0 = torch.nn.functional.normalize(torch.randn((a.B, a.cap, a.d), generator=g), dim=-1).to(dev)
    x1 = torch.nn.functional.normalize(torch.randn((a.B, a.cap, a.d), generator=g), dim=-1).to(dev)
    gt0, gt1, pos0 = (torch.from_numpy(np.stack([v] * a.B)).to(dev) for v in R.labels("edges", a.cap, a.cap))
    assignment = torch.from_numpy(np.stack([R.scatter(pos0[0].cpu().numpy(), a.cap)] * a.B)).to(dev).bool()
    loss_fn = LGM.NLLLoss({})
    op = lambda: N.lg_nll_values(N.lg_assign_nll(head, x0, x1, gt0, gt1, pos0=pos0))  # noqa: E731
    op_dense = lambda: N.lg_nll_values(N.lg_assign_nll(head, x0, x1, gt0, gt1, assignment=assignment))  # noqa: E731
    ref = lambda: dense_baseline(head, x0, x1, gt0, gt1, assignment, loss_fn)  # noqa: E731
    (vals, row_norm), (nll, nll_pos, nll_neg, rn) = op(), ref()
    got = torch.cat([vals[:, :3], row_norm[:, None]], 1)
    exp = torch.stack([nll, nll_pos, nll_neg, rn], 1).double()
    line = {"B": a.B, "cap": a.cap, "d": a.d, "positives_per_pair": float((pos0 >= 0).sum()) / a.B,
            "max_abs_diff_from_dense_torch": float((got - exp).abs().max()),
            "lg_assign_nll_pos0": timed(op, a.iters), "lg_assign_nll_dense": timed(op_dense, a.iters), "dense_torch": timed(ref, a.iters)}
    line["speedup"] = line["dense_torch"]["ms_median"] / line["lg_assign_nll_pos0"]["ms_median"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
