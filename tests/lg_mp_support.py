"""What tests/test_lg_mp_gpu.py needs around the kernels: models, ragged PairBatches, the outputs a call defines, and the
match-decision rule against a float64 spec.  Not collected by pytest.  The rules are those of tests/test_lg_flash_gpu.py (DESIGN.md
8k), restated here so that the two test files do not depend on each other."""
import numpy as np
import torch

import lg_f64
from helpers import close_and_record, la_bound_f64, lgf64_pair, lgf64_shipped_state_dict, record_flips
from gpu_support import DEV, FTOL, _np, _t, pkg

PairBatch = __import__("importlib").import_module(pkg.__name__ + ".core.modules.matchers._batched").PairBatch
SIZE = (260, 346)

# (case, layers, [(n, m)], cap0, cap1): counts from {0, 1, 33, 129, 300}; equal caps stack the sides, unequal caps run one launch per
# side.  A count of 1 is always paired with a longer side (in a (1, 1) pair the two peers are the same computation).
FORWARD = [
    ("stacked_l3", 3, [(33, 129), (300, 1), (0, 33)], 300, 300),
    ("unstacked_l3", 3, [(129, 300), (1, 33), (33, 0)], 129, 300),
    ("stacked_l9", 9, [(300, 129), (33, 33), (1, 300)], 300, 300),
]

# The shipped model with two biases moved: matchability bias 1 by -5.4918 puts the pruning threshold (sigmoid > 0.01)
# into the widest gap of the layer-1 logits; token bias 5 by +5 with depth_confidence 0.9 stops both pairs after layer 5.  Under the
# mp contract the decisions keep their margins (lg_mp_ref.safe_refs, checked in tests/test_lg_mp_cpu.py).
WIDTH, DEPTH = 0.99, 0.9
MSHIFT, TSHIFT = {1: -5.4918}, {5: 5.0}
LAYERS = 9
ADAPTIVE_PAIRS = [(11, 31, 33), (11, 64, 64), (11, 0, 5)]


def cut_sd(sd, layers):
    keep = lambda k: k.split(".")[0] not in ("transformers", "log_assignment", "token_confidence") or int(k.split(".")[1]) < layers  # noqa: E731
    return {k: v for k, v in sd.items() if keep(k) and not (k.startswith("token_confidence.") and int(k.split(".")[1]) >= layers - 1)}


def conf(layers, **kw):
    return dict(input_dim=256, descriptor_dim=256, num_heads=4, n_layers=layers, **kw)


def model(cf, sd, mixed=False):
    lg = pkg.LightGlue(cf).to(DEV)
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    lg.refresh()
    lg.mixed_precision = mixed
    return lg.eval()


def pair(seed, n, m, din=256):
    """(k0, d0, k1, d1); an empty side is cut from a pair that has rows"""
    d0, d1, k0, k1 = lgf64_pair(seed, max(n, 1), max(m, 1), din)
    return k0[:n], d0[:n], k1[:m], d1[:m]


def feats(k, d):
    return {"sparse_descriptors": _t(d)[None], "sparse_positions": _t(k)[None], "image_size": [torch.tensor(SIZE)]}


def batch(ks, ds, cap, kfill=1e6, dfill=7.0):
    """PairBatch of ragged entries; the padding rows hold garbage (far keypoints, a constant descriptor)"""
    B, din = len(ks), ds[0].shape[1]
    K, D = np.full((B, cap, 3), kfill, np.float32), np.full((B, cap, din), dfill, np.float32)
    for b in range(B):
        K[b, :len(ks[b])], D[b, :len(ds[b])] = ks[b], ds[b]
    pb = PairBatch()
    pb.kpts, pb.desc, pb.counts = _t(K), _t(D), _t(np.asarray([len(k) for k in ks], np.int32))
    pb.cap, pb.B, pb.image_size, pb.counts_host = cap, B, SIZE, None
    return pb


def batches(pairs, cap0=None, cap1=None):
    cap0 = cap0 or max(max(len(p[0]) for p in pairs), 1)
    cap1 = cap1 or max(max(len(p[2]) for p in pairs), 1)
    return batch([p[0] for p in pairs], [p[1] for p in pairs], cap0), batch([p[2] for p in pairs], [p[3] for p in pairs], cap1, dfill=-3.0)


def bits(r, pairs):
    """what a call defines, per pair: the rows below the pair's counts (the outputs are torch.empty: the padding is not written)"""
    out = []
    for b, p in enumerate(pairs):
        n, m = len(p[0]), len(p[2])
        e = {"matches0": _np(r.matches0)[b, :n], "matches1": _np(r.matches1)[b, :m], "scores0": _np(r.scores0)[b, :n], "scores1": _np(r.scores1)[b, :m]}
        if r.la is not None and n and m:
            e["la"] = _np(r.la)[b, :n + 1, :m + 1]
        if r.ref0 is not None:
            e["ref0"], e["ref1"] = _np(r.ref0)[b][..., :n, :], _np(r.ref1)[b][..., :m, :]
        out.append({k: np.ascontiguousarray(v).copy() for k, v in e.items()})
    return out


def equal_bits(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)) for k in x)
                                    for x, y in zip(a, b))


def peer_bound(spec, peers, absmax):
    """helpers.la_bound_f64 of the peers' distances from the spec: twice the worse peer plus its ulp term"""
    return la_bound_f64([np.abs(p - spec).max() for p in peers], absmax)


def check_matches(tag, got, ex, bound, la=None):
    """assignments equal to the spec's decisions except at rows / columns whose spec margin (top-2 gap, distance from the filter's
    edge) is inside `bound`; the scores of the rows that agree within max(FTOL, bound)"""
    la = ex["log_assignment"] if la is None else la
    n, m = la.shape[0] - 1, la.shape[1] - 1
    s = la[:-1, :-1]
    row_gap, col_gap = lg_f64.top2_gaps(s, 1), lg_f64.top2_gaps(s, 0)
    edge = np.abs(s.max(1) - lg_f64.filter_edge(0.0))
    row_ok, col_ok = (row_gap < bound) | (edge < bound), col_gap < bound
    m0, m1, e0, e1 = got["m0"], got["m1"], ex["matches0"], ex["matches1"]
    assert (m0 < m).all() and (m1 < n).all()
    for i in np.nonzero(m0 != e0)[0]:
        assert row_ok[i] or any(col_ok[j] for j in (m0[i], e0[i]) if j >= 0), (tag, "row", int(i), int(m0[i]), int(e0[i]))
    for j in np.nonzero(m1 != e1)[0]:
        assert col_ok[j] or any(row_ok[i] for i in (m1[j], e1[j]) if i >= 0), (tag, "column", int(j), int(m1[j]), int(e1[j]))
    record_flips(f"{tag}.matches0 gpu vs spec", m0, e0, la)
    record_flips(f"{tag}.matches1 gpu vs spec", m1, e1, la.T)
    same0, same1 = m0 == e0, m1 == e1
    close_and_record(f"{tag}.matching_scores0 gpu vs spec", got["s0"][same0], ex["scores0"][same0], atol=max(FTOL, bound))
    close_and_record(f"{tag}.matching_scores1 gpu vs spec", got["s1"][same1], ex["scores1"][same1], atol=max(FTOL, bound))


def cut(r, pairs):
    """a match_batched(all_layers=True) result per pair: la, the descriptors after every layer, matches, scores"""
    la, ref0, ref1 = _np(r.la), _np(r.ref0), _np(r.ref1)
    m0, m1, s0, s1 = _np(r.matches0), _np(r.matches1), _np(r.scores0), _np(r.scores1)
    out = []
    for b, p in enumerate(pairs):
        n, m = len(p[0]), len(p[2])
        assert (m0[b, n:] == -1).all() and (m1[b, m:] == -1).all(), (b, "padding rows matched")
        out.append({"la": la[b, :n + 1, :m + 1], "layers": [(ref0[b, i, :n], ref1[b, i, :m]) for i in range(ref0.shape[1])],
                    "m0": m0[b, :n], "m1": m1[b, :m], "s0": s0[b, :n], "s1": s1[b, :m]})
    return out


def adaptive_case(mode):
    """mode "prune", "stop" or "both" -> (prune, stop, width_confidence, depth_confidence, the shifted state dict)"""
    prune, stop = mode != "stop", mode != "prune"
    sd = lgf64_shipped_state_dict(7)
    for i, s in (MSHIFT if prune else {}).items():
        sd[f"log_assignment.{i}.matchability.bias"] = sd[f"log_assignment.{i}.matchability.bias"] + np.float32(s)
    for i, s in (TSHIFT if stop else {}).items():
        sd[f"token_confidence.{i}.token.0.bias"] = sd[f"token_confidence.{i}.token.0.bias"] + np.float32(s)
    return prune, stop, (WIDTH if prune else -1), (DEPTH if stop else -1), sd
