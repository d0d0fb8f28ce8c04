"""LightGlue's `mp: True` contract as code, on top of tests/lg_f64.py.  Not collected by pytest.

For each of the nine nn.Linear of every transformer layer (SelfBlock Wqkv, out_proj, ffn.0, ffn.3; CrossBlock to_qk, to_v, to_out,
ffn.0, ffn.3):
  1. every input element is rounded to IEEE binary16, round to nearest even, overflow to infinity (`tensor.half()`) -- both halves of
     cat([x, message]) for ffn.0;
  2. every weight element is rounded the same way;
  3. the products (exact in fp32) are accumulated in fp32 in any order;
  4. the fp32 bias is added in fp32;
  5. the result stays fp32: it is NOT rounded to binary16.
Everything else is lg_f64's: input_proj, the positional encoding, rotary, residual, LayerNorm, GELU, the attention, the heads
(final_proj, matchability, token_confidence) and every decision.

MODES of the linear (`mode` below):
  "spec"   float64 on binary16-rounded operands: what the kernel is measured against
  "exact"  float64, no rounding: must reproduce lg_f64.forward
  "peer_a" float32 forward, torch's fp32 matmul of the rounded operands
  "peer_b" float32 forward, a blocked k-ascending chain: 32-deep partial products added to one fp32 accumulator in ascending k
The peers are two independent fp32 implementations of the same contract with different accumulation orders; helpers.la_bound_f64
turns their distance from "spec" into the bound for the kernel.

`linears(mode)` swaps lg_f64._linear for the time of a `with`: the layers' linears (a prefix that names a transformer layer) follow
the contract, every other one stays lg_f64's.  lg_f64.forward, lg_flash_ref's blocks, lg_early_stop_ref.run and lg_prune_ref.run reach
the linears through the module, so they compose: `with lg_flash_ref.blocks(m), lg_mp_ref.linears(m): ...` is mp + flash."""
import contextlib

import numpy as np
import torch

import lg_f64
import lg_flash_ref

DTYPE = lg_flash_ref.DTYPE
CHAIN = 32  # k-block of peer_b
_PLAIN = lg_f64._linear


def rn16(t):
    """round to binary16 (nearest even, overflow to infinity) and back to the tensor's dtype"""
    return t.to(torch.float16).to(t.dtype)


def linear(x, w, b, mode):
    """x [rows, K], w [N, K], b [N] in DTYPE[mode] -> [rows, N] in DTYPE[mode]"""
    assert x.dtype == w.dtype == b.dtype == DTYPE[mode], (x.dtype, w.dtype, mode)
    if mode == "exact":
        return x @ w.T + b
    xr, wr = rn16(x), rn16(w)
    if mode in ("spec", "peer_a"):
        return xr @ wr.T + b
    assert mode == "peer_b"
    acc = torch.zeros((x.shape[0], w.shape[0]), dtype=x.dtype)
    for k0 in range(0, x.shape[1], CHAIN):
        acc = acc + xr[:, k0:k0 + CHAIN] @ wr[:, k0:k0 + CHAIN].T
    return acc + b


def is_layer_prefix(prefix):
    return "transformers." in prefix


@contextlib.contextmanager
def linears(mode):
    """lg_f64._linear replaced by the contract's linear in `mode` for the layers' prefixes; restored on exit"""
    saved = lg_f64._linear

    def _linear(x, sd, prefix, key, dtype):
        if not is_layer_prefix(prefix):
            return saved(x, sd, prefix, key, dtype)
        assert dtype == DTYPE[mode], (dtype, mode)
        return linear(x, lg_f64._w(sd, prefix, key + ".weight", dtype), lg_f64._w(sd, prefix, key + ".bias", dtype), mode)

    lg_f64._linear = _linear
    try:
        yield
    finally:
        lg_f64._linear = saved


@contextlib.contextmanager
def contract(mode, flash=False):
    """the mp contract in `mode`, with the flash contract in the same mode on top when `flash`"""
    with contextlib.ExitStack() as st:
        if flash:
            st.enter_context(lg_flash_ref.blocks(mode))
        st.enter_context(linears(mode))
        yield


def forward(sd, kpts0, desc0, kpts1, desc1, mode="spec", flash=False, **kw):
    """lg_f64.forward (same arguments and outputs) under the mp contract in `mode` (and the flash contract when `flash`)"""
    with contract(mode, flash):
        return lg_f64.forward(sd, kpts0, desc0, kpts1, desc1, dtype=DTYPE[mode], **kw)


def _logit(s):
    s = np.asarray(s, np.float64)
    return np.log(s) - np.log1p(-s)


def safe_refs(adaptive, sd, pair, width, depth, flash=False):
    """The restatement of point pruning / early stopping (lg_prune_ref.run / lg_early_stop_ref.run: their decision logic, untouched)
    under the contract: the spec and the two peers ({"spec", "peer_a", "peer_b"} -> run).  `adaptive`: "prune", "stop" or "both".
    Before anything is compared with the spec's decisions they are shown to be out of the rounding's reach by the peers' own scatter,
    the rule of tests/test_lg_flash_gpu.py::_safe_refs:
      pruning: the peers took the spec's decisions, and every matchability logit the spec compared is further from the threshold
               than twice the largest deviation of a peer's logit from the spec's;
      stopping: at every layer the count of unconfident rows is further from the count at which the decision flips than twice the
               largest deviation of a peer's count from the spec's, plus one row."""
    import lg_early_stop_ref as ES
    import lg_prune_ref as P
    prune, stop = adaptive != "stop", adaptive != "prune"
    refs = {}
    for m in ("spec", "peer_a", "peer_b"):
        with contract(m, flash):
            refs[m] = P.run(sd, *pair, width, 0, depth, dtype=DTYPE[m]) if prune else ES.run(sd, *pair, depth, dtype=DTYPE[m])
    spec = refs["spec"]
    total = len(pair[0]) + len(pair[2])
    for m in ("peer_a", "peer_b"):
        assert refs[m]["stop"] == spec["stop"], (adaptive, m)
    if prune:
        thr = float(_logit(P.width_threshold(width)))
        margin, dev = np.inf, 0.0
        for m in ("peer_a", "peer_b"):
            assert len(refs[m]["steps"]) == len(spec["steps"]), (adaptive, m)
            for a, b in zip(spec["steps"], refs[m]["steps"]):
                assert a["layer"] == b["layer"] and all(np.array_equal(x, y) for x, y in zip(a["kept"], b["kept"])), (adaptive, m)
                for s in range(2):
                    if a["sig"][s] is not None:
                        margin = min(margin, float(np.abs(_logit(a["sig"][s]) - thr).min()))
                        dev = max(dev, float(np.abs(_logit(a["sig"][s]) - _logit(b["sig"][s])).max()))
        assert margin > 2 * dev, (adaptive, "pruning margin", margin, dev)
    if stop:
        flip = (1.0 - depth) * total  # the stop decision: 1 - below / total > depth
        dev = max(abs(a - b) for m in ("peer_a", "peer_b") for a, b in zip(spec["below"], refs[m]["below"]))
        margin = min(abs(b - flip) for b in spec["below"])
        assert margin > 2 * dev + 1, (adaptive, "stop margin in rows", margin, dev)
    return refs


def linear_np(X, W, b, mode="spec"):
    """the linear alone on numpy arrays -> float64 numpy"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DTYPE[mode])  # noqa: E731
    with torch.no_grad():
        return linear(t(X), t(W), t(b), mode).to(torch.float64).numpy()
