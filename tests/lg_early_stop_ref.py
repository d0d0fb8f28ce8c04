"""LightGlue's early stopping (per-pair adaptive depth) for ONE pair, stated on top of tests/lg_f64.py: the layers and
the heads in float64 (or float32 on request), the decision in the float32 arithmetic of the contract.  Not collected by pytest.

After layer i < L - 1:  c = sigmoid(token_confidence[i].token[0](x)) over the n + m rows, below = #{c < thr[i]},
r = 1.0f - float32(below) / float32(n + m), the pair stops iff r > float32(depth_confidence); stop = i + 1 and the assignment is
log_assignment[i] on the descriptors after layer i.  Never stopping: stop = L, the full-depth result.  n == 0 or m == 0: stop = 0.

`near[i]` counts the confidences with |c - thr[i]| < NEAR: a float32 implementation may put those on the other side, so a decision
is SAFE when it is the same for every count in [below - near, below + near].  A test compares `stop` only where every decision the
pair met is safe."""
import numpy as np
import torch

import lg_f64

NEAR = 1e-5


def thresholds(n_layers):
    """thr[i] = float32(clip(0.8 + 0.1 exp(-4 i / n_layers), 0, 1)), i = 0 .. n_layers - 2"""
    return [np.float32(np.clip(0.8 + 0.1 * np.exp(-4.0 * i / n_layers), 0, 1)) for i in range(n_layers - 1)]


def ratio(below, total):
    return np.float32(1.0) - np.float32(below) / np.float32(total)


def decide(below, total, depth_confidence):
    """the float32 rule: IEEE float32 division, subtraction from 1.0f, compared with float32(depth_confidence)"""
    return bool(ratio(below, total) > np.float32(depth_confidence))


def safe(below, near, total, depth_confidence):
    lo, hi = max(below - near, 0), min(below + near, total)
    return decide(lo, total, depth_confidence) == decide(hi, total, depth_confidence)


def confidences(x0, x1, sd, i, prefix="", dtype=torch.float64):
    """token_confidence[i] on both sides' rows, [n + m]"""
    x = torch.cat([torch.from_numpy(np.ascontiguousarray(x0)).to(dtype), torch.from_numpy(np.ascontiguousarray(x1)).to(dtype)], 0)
    z = lg_f64._linear(x, sd, f"{prefix}token_confidence.{i}.", "token.0", dtype)[:, 0]
    return torch.sigmoid(z).numpy()


def truncated_state_dict(sd, stop, prefix=""):
    """the state dict of the model that has only the first `stop` layers: its last head is log_assignment[stop - 1]"""
    out = {}
    for k, v in sd.items():
        parts = k[len(prefix):].split(".")
        if parts[0] in ("transformers", "log_assignment") and int(parts[1]) >= stop:
            continue
        if parts[0] == "token_confidence" and int(parts[1]) >= stop - 1:
            continue
        out[k] = v
    return out


def run(sd, k0, d0, k1, d1, depth_confidence, size0=(260, 346), size1=(260, 346), filter_threshold=0.0, prefix="", dtype=torch.float64):
    """Returns stop, the per-layer lists below / near / r / safe up to the stopping layer, and the stopping head's result:
    log_assignment [n+1, m+1], matches0/1, scores0/1, x0 / x1 (the descriptors the head read)."""
    n, m = len(k0), len(k1)
    if n == 0 or m == 0:
        return dict(stop=0, below=[], near=[], r=[], safe=[])
    full = lg_f64.forward(sd, k0, d0, k1, d1, size0=size0, size1=size1, filter_threshold=filter_threshold, prefix=prefix, dtype=dtype)
    L = len(full["layers"])
    thr = thresholds(L)
    out = dict(stop=L, below=[], near=[], r=[], safe=[])
    for i in range(L - 1):
        c = confidences(*full["layers"][i], sd, i, prefix, dtype)
        below = int((c < float(thr[i])).sum())
        near = int((np.abs(c - float(thr[i])) < NEAR).sum())
        out["below"].append(below)
        out["near"].append(near)
        out["r"].append(float(ratio(below, n + m)))
        out["safe"].append(safe(below, near, n + m, depth_confidence))
        if decide(below, n + m, depth_confidence):
            out["stop"] = i + 1
            break
    x0, x1 = full["layers"][out["stop"] - 1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    with torch.no_grad():
        la = lg_f64.log_assignment(t(x0), t(x1), sd, f"{prefix}log_assignment.{out['stop'] - 1}.", dtype)
        m0, m1, s0, s1, _ = lg_f64.filter_matches(la, filter_threshold)
    out.update(log_assignment=la.numpy(), matches0=m0, matches1=m1, scores0=s0, scores1=s1, x0=x0, x1=x1)
    return out
