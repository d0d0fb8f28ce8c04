#!/usr/bin/env python3
"""Fixture of LightGlue.loss in eval mode, generated from the reference (build container only):
    python tests/golden/gen_lg_loss.py   ->  tests/golden/lg_loss.npz
Runs the reference's LightGlue (core/modules/matchers/lightglue.py) on the CPU through _ref_stubs, in eval mode, on stacked B = 2
inputs with name-synthesised weights, then its `loss` on the integer-built labels of tests/lg_loss_ref.py, and stores RECORDED
RESULTS only: per case the reference's ref_descriptors (the input of everything downstream) and its eight values per key; the
float64 restatement (tests/lg_loss_ref.py) on those descriptors and its distance from the reference; the float32 peer's largest
|la - la_f64| and max |la|, which is what the tests' bound is made of.  Also what the reference does in the four situations the
drop-in mirrors or refuses (n != m both ways, m == 1 < n, eval mode with two layers of ref_descriptors, training mode), by type and
message."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_stubs  # noqa: E402
import lg_loss_ref as R  # noqa: E402
from helpers import lg_inputs, synth  # noqa: E402

_ref_stubs.install()
sys.path.insert(0, "/root/reference")
from core.modules.matchers.lightglue import LightGlue  # noqa: E402

torch.set_num_threads(1)
CASES = [
    dict(name="d64", input_dim=64, descriptor_dim=64, num_heads=2, n_layers=2, n=130, m=130, B=2, wseed=41, seed=410, kinds=["edges", "nopos"]),
    dict(name="d256", input_dim=256, descriptor_dim=256, num_heads=4, n_layers=1, n=200, m=200, B=2, wseed=42, seed=420, kinds=["edges", "ignore"]),
]
SIZE = torch.tensor([260, 346])


def model_for(c, n_layers=None):
    conf = _ref_stubs.to_attr({k: c[k] for k in ("input_dim", "descriptor_dim", "num_heads", "n_layers")})
    if n_layers is not None:
        conf["n_layers"] = n_layers
    lg = LightGlue(conf)
    sd = lg.state_dict()
    new = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in sd.items()], c["wseed"])
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()}, strict=False)
    return lg.eval(), new


def feats(c, n, m):
    d0, d1, k0, k1 = [], [], [], []
    for b in range(c["B"]):
        a = lg_inputs(dict(seed=c["seed"] + 10 * b, n=n, m=m, input_dim=c["input_dim"], shared=min(n, m) // 2))
        for lst, v in zip((d0, d1, k0, k1), a):
            lst.append(v)
    st = lambda l: torch.from_numpy(np.stack(l))  # noqa: E731
    return ({"sparse_descriptors": st(d0), "sparse_positions": st(k0), "image_size": [SIZE] * c["B"]},
            {"sparse_descriptors": st(d1), "sparse_positions": st(k1), "image_size": [SIZE] * c["B"]})


def gt_for(kinds, n, m):
    g0, g1, W = [], [], []
    for kind in kinds:
        a, b, p = R.labels(kind, n, m)
        g0.append(a), g1.append(b), W.append(R.scatter(p, m))
    return {"gt_matches0": torch.from_numpy(np.stack(g0)), "gt_matches1": torch.from_numpy(np.stack(g1)),
            "gt_assignment": torch.from_numpy(np.stack(W)).bool()}


def outcome(fn):
    try:
        r = fn()
        return {"raises": None, "keys": list(r[0])}
    except Exception as e:  # noqa: BLE001
        return {"raises": type(e).__name__, "message": str(e), "arg": e.args[0] if e.args else None}


def main():
    out, cases = {}, []
    for c in CASES:
        lg, sd = model_for(c)
        f0, f1 = feats(c, c["n"], c["m"])
        with torch.no_grad():
            pred = lg(f0, f1)
            losses, _ = lg.loss(pred, gt_for(c["kinds"], c["n"], c["m"]))
        name = c["name"]
        assert list(losses) == list(R.LOSS_KEYS), list(losses)
        assert pred["ref_descriptors0"].shape[1] == 1
        out[f"{name}.ref0"] = pred["ref_descriptors0"][:, 0].numpy()
        out[f"{name}.ref1"] = pred["ref_descriptors1"][:, 0].numpy()
        ref = np.stack([losses[k].double().numpy() for k in R.LOSS_KEYS], 1)  # [B, 8]
        out[f"{name}.ref_values"] = ref
        head = R.head_dict(sd, f"log_assignment.{c['n_layers'] - 1}.")
        f64, rows, dist, peer, absmax = [], [], 0.0, 0.0, 0.0
        for b, kind in enumerate(c["kinds"]):
            gt0, gt1, pos0 = R.labels(kind, c["n"], c["m"])
            x0, x1 = out[f"{name}.ref0"][b], out[f"{name}.ref1"][b]
            v, r8, la = R.loss(x0, x1, head, gt0, gt1, R.scatter(pos0, c["m"]))
            la32 = R.log_assignment(x0, x1, head, torch.float32)
            f64.append([v[k] for k in R.LOSS_KEYS]), rows.append(r8)
            peer = max(peer, float(np.abs(la32.astype(np.float64) - la).max()))
            absmax = max(absmax, float(np.abs(la).max()))
            dist = max(dist, float(np.abs(np.array(f64[-1]) - ref[b]).max()))
            # the reference's own log_assignment against the float64 one: a second peer
            peer_ref = float(np.abs(pred["log_assignment"][b].double().numpy() - la).max())
        out[f"{name}.f64_values"] = np.array(f64)
        out[f"{name}.f64_sums"] = np.array(rows)
        cases.append(dict(c, state_keys={k: list(v.shape) for k, v in sorted(sd.items())}, f64_vs_ref=dist, peer_la_err=peer, la_absmax=absmax,
                          ref_la_err_last_pair=peer_ref))
        print(name, "restatement vs reference", dist, "peer", peer, "ref la err", peer_ref, "max |la|", absmax)
        print(ref)

    # ---- what the reference does where the drop-in mirrors or refuses --------------------------------------------------------
    c = dict(CASES[0], n_layers=2)
    lg, _ = model_for(c)
    fails = {}
    for tag, n, m in (("n_gt_m", 12, 9), ("n_lt_m", 9, 12), ("m_is_1", 5, 1)):
        f0, f1 = feats(c, n, m)
        with torch.no_grad():
            pred = lg(f0, f1)
        fails[tag] = dict(outcome(lambda: lg.loss(pred, gt_for(["edges", "nopos"], n, m))), n=n, m=m, B=c["B"])
    f0, f1 = feats(c, 12, 12)
    with torch.no_grad():
        pred = lg(f0, f1)
    two = dict(pred, ref_descriptors0=pred["ref_descriptors0"].repeat(1, 2, 1, 1), ref_descriptors1=pred["ref_descriptors1"].repeat(1, 2, 1, 1))
    fails["eval_two_layers"] = outcome(lambda: lg.loss(two, gt_for(["edges", "nopos"], 12, 12)))
    lg.train()
    predt = lg(f0, f1)
    fails["training"] = outcome(lambda: lg.loss(predt, gt_for(["edges", "nopos"], 12, 12)))
    for k, v in fails.items():
        print(k, v)
    meta = {"torch": torch.__version__, "cases": cases, "failures": fails}
    path = os.path.join(HERE, "lg_loss.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == "__main__":
    main()
