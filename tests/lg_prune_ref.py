"""LightGlue's point pruning (per-pair, per-side adaptive width) for ONE pair, stated on top of tests/lg_f64.py and
tests/lg_early_stop_ref.py: the layers and the heads in float64 (or float32 on request) over the CURRENT survivor sets, the two
comparisons in the float32 arithmetic of the contract.  Not collected by pytest.

After layer i < L - 1 of a pair that is still running, first the stop decision when depth_confidence > 0 (lg_early_stop_ref's rule
over the surviving rows, divided by the ORIGINAL n + m as the reference's `m + n`, lightglue.py:635); a pair that stops is not
pruned.  Then each side with more than min_kpts rows keeps
    float32(sigmoid(log_assignment[i].matchability(x))) > float32(1.0 - width_confidence)
 or, with early stopping only,  float32(sigmoid(token_confidence[i](x))) <= thr[i]
in its order; prune[ind[kept]] += 1.  A side left without rows finishes the pair: no matches, stop = i + 1 with early stopping.
The assignment runs over the survivors with head stop - 1 (the last one without early stopping) and is scattered back through ind.

`near_w` / `near_t` count the rows whose sigmoid lies within NEAR of the threshold it is compared with: a float32 implementation may
put those on the other side, so a pruning step is SAFE when both are 0.  NEAR: the float32 and the float64 run of this file differ
by 1.5e-6 at most in the matchability sigmoid on the pairs of tests/test_lg_prune_gpu.py (test_lg_prune_cpu.py measures it), so
lg_early_stop_ref's 1e-5 is more than four times that and is kept."""
import numpy as np
import torch

import lg_early_stop_ref as ES
import lg_f64

NEAR = ES.NEAR


def width_threshold(width_confidence):
    """float32(1.0 - double(width_confidence))"""
    return np.float32(1.0 - float(width_confidence))


def keep_mask(s, thr_w, c=None, thr_t=None):
    """the keep rule on sigmoid outputs (any float dtype): both comparisons in float32"""
    keep = np.asarray(s).astype(np.float32) > np.float32(thr_w)
    if c is not None:
        keep = keep | (np.asarray(c).astype(np.float32) <= np.float32(thr_t))
    return keep


def scatter_back(m0, s0, ind0, ind1, n):
    """lightglue.py:659-667 for one side: matches / scores of the survivors into original indexing; pruned points get -1 / 0"""
    out_m, out_s = np.full(n, -1, np.int64), np.zeros(n, np.asarray(s0).dtype)
    if len(ind0):
        out_m[ind0] = np.where(m0 == -1, -1, np.asarray(ind1, np.int64)[np.clip(m0, 0, None)] if len(ind1) else -1)
        out_s[ind0] = s0
    return out_m, out_s


def _sig(x, sd, key, dtype):
    return torch.sigmoid(lg_f64._linear(x, sd, "", key, dtype)[:, 0]).numpy()


def run(sd, k0, d0, k1, d1, width_confidence, min_kpts=0, depth_confidence=-1.0, size0=(260, 346), size1=(260, 346), filter_threshold=0.0,
        prefix="", dtype=torch.float64):
    """Returns stop (None without early stopping), steps = one dict per pruning step taken {layer, kept: (ind0, ind1) after it,
    pruned: (bool, bool) which sides passed the gate, near_w, near_t, sig: (s0, s1) the matchability sigmoids it compared}, the
    stop decisions {below, near, r, safe} per layer met, safe (every decision and step), prune0/1 float32, kept0/1, live,
    x0 / x1 (the survivors' descriptors the head read), log_assignment over the survivors (None when there is none), head, and
    matches0/1, scores0/1 in original indexing."""
    n, m = len(k0), len(k1)
    es = float(depth_confidence) > 0
    out = dict(stop=None, steps=[], below=[], near=[], r=[], safe_stop=[], prune0=np.ones(n, np.float32), prune1=np.ones(m, np.float32),
               kept0=np.arange(n), kept1=np.arange(m), matches0=np.full(n, -1, np.int64), matches1=np.full(m, -1, np.int64),
               scores0=np.zeros(n), scores1=np.zeros(m), log_assignment=None, x0=None, x1=None, head=None, safe=True)
    out["live"] = (n, m)
    if n == 0 or m == 0:
        out["stop"] = 0 if es else None
        return out
    with torch.no_grad():
        L = sum(1 for k in sd if k.startswith(prefix + "transformers.") and k.endswith(".self_attn.Wqkv.weight"))
        sdp = {k[len(prefix):]: v for k, v in sd.items()} if prefix else sd
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
        x0, x1 = t(d0), t(d1)
        if "input_proj.weight" in sdp:
            x0, x1 = lg_f64._linear(x0, sdp, "", "input_proj", dtype), lg_f64._linear(x1, sdp, "", "input_proj", dtype)
        d = x0.shape[1]
        Wr = lg_f64._w(sdp, "", "posenc.Wr.weight", dtype)
        heads = d // (2 * Wr.shape[0])
        enc0 = lg_f64.rotary(lg_f64.normalize_keypoints(t(np.asarray(k0)[:, :2]), size0, dtype), Wr)
        enc1 = lg_f64.rotary(lg_f64.normalize_keypoints(t(np.asarray(k1)[:, :2]), size1, dtype), Wr)
        ind = [np.arange(n), np.arange(m)]
        prune = [out["prune0"], out["prune1"]]
        thr_t, thr_w = ES.thresholds(L), width_threshold(width_confidence)
        stop, finished = L, False
        for i in range(L):
            p = f"transformers.{i}."
            x0 = lg_f64.self_block(x0, enc0, sdp, p + "self_attn.", heads, dtype)
            x1 = lg_f64.self_block(x1, enc1, sdp, p + "self_attn.", heads, dtype)
            x0, x1 = lg_f64.cross_block(x0, x1, sdp, p + "cross_attn.", heads, dtype)
            if i == L - 1:
                break
            tok = None
            if es:
                tok = [_sig(x, sdp, f"token_confidence.{i}.token.0", dtype) for x in (x0, x1)]
                c = np.concatenate(tok)
                below = int((c < float(thr_t[i])).sum())
                near = int((np.abs(c - float(thr_t[i])) < NEAR).sum())
                out["below"].append(below)
                out["near"].append(near)
                out["r"].append(float(ES.ratio(below, n + m)))
                out["safe_stop"].append(ES.safe(below, near, n + m, depth_confidence))
                if ES.decide(below, n + m, depth_confidence):
                    stop = i + 1
                    break
            xs, encs = [x0, x1], [enc0, enc1]
            step = dict(layer=i, pruned=[False, False], near_w=0, near_t=0, sig=[None, None])
            for s in range(2):
                if xs[s].shape[0] <= min_kpts:
                    continue
                sg = _sig(xs[s], sdp, f"log_assignment.{i}.matchability", dtype)
                keep = keep_mask(sg, thr_w, tok[s] if es else None, thr_t[i] if es else None)
                step["pruned"][s] = True
                step["sig"][s] = sg
                step["near_w"] += int((np.abs(sg - float(thr_w)) < NEAR).sum())
                if es:
                    step["near_t"] += int((np.abs(tok[s] - float(thr_t[i])) < NEAR).sum())
                idx = torch.from_numpy(np.nonzero(keep)[0])
                xs[s], encs[s], ind[s] = xs[s][idx], encs[s][:, idx], ind[s][keep]
                prune[s][ind[s]] += 1
            x0, x1, enc0, enc1 = xs[0], xs[1], encs[0], encs[1]
            step["kept"] = (ind[0].copy(), ind[1].copy())
            if any(step["pruned"]):
                out["steps"].append(step)
            if len(ind[0]) == 0 or len(ind[1]) == 0:
                stop, finished = i + 1, True
                break
        out.update(stop=stop if es else None, kept0=ind[0], kept1=ind[1], live=(len(ind[0]), len(ind[1])), x0=x0.numpy(), x1=x1.numpy())
        out["safe"] = all(out["safe_stop"]) and all(s["near_w"] == 0 and s["near_t"] == 0 for s in out["steps"])
        if finished:
            return out
        out["head"] = (stop if es else L) - 1
        la = lg_f64.log_assignment(x0, x1, sdp, f"log_assignment.{out['head']}.", dtype)
        m0, m1, s0, s1, _ = lg_f64.filter_matches(la, filter_threshold)
        out["log_assignment"] = la.numpy()
        out["matches0"], out["scores0"] = scatter_back(m0, s0, ind[0], ind[1], n)
        out["matches1"], out["scores1"] = scatter_back(m1, s1, ind[1], ind[0], m)
    return out
