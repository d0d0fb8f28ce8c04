"""LightGlue's `flash: True` contract as code, on top of tests/lg_f64.py.  Not collected by pytest.

For every attention call, self and cross, per head:
  1. q, k, v are rounded to IEEE binary16, round to nearest even (`tensor.half()`), q and k after the rotary step, the cross block's
     qk unscaled; the 1/sqrt(dh) factor multiplies the product, as scaled_dot_product_attention does;
  2. softmax(scale q k^T) v;
  3. the result is rounded to binary16 and widened again.
Everything else is lg_f64's: projections, rotary, out_proj / to_out, FFN, assignment, filter.

MODES of the attention (`mode` below):
  "spec"   float64, steps 1 and 3 through torch.float16, the softmax exact: what the kernel is measured against
  "exact"  float64, no rounding: must reproduce lg_f64.forward (the blocks here are restated, not lg_f64's)
  "peer_a" float32 forward whose attention is the reference's line on CPU tensors:
           F.scaled_dot_product_attention(q.half(), k.half(), v.half()).float()
  "peer_b" float32 forward with the probabilities exp(s - max) rounded to binary16 before the second product, both products and the
           row sum accumulated in float32, o / l in float32, then step 3
The peers are two independent float implementations of the same contract; helpers.la_bound_f64 turns their distance from "spec"
into the bound for the kernel.

`blocks(mode)` swaps lg_f64.self_block / cross_block for the time of a `with`, so that lg_f64.forward, lg_early_stop_ref.run and
lg_prune_ref.run -- which reach the blocks through the module -- run the flash contract with their own decision logic unchanged."""
import contextlib

import numpy as np
import torch

import lg_f64

DTYPE = {"spec": torch.float64, "exact": torch.float64, "peer_a": torch.float32, "peer_b": torch.float32}


def rn16(t):
    """round to binary16 (nearest even, overflow to infinity) and back to the tensor's dtype"""
    return t.to(torch.float16).to(t.dtype)


def attention(q, k, v, mode):
    """q [H, n, dh], k / v [H, m, dh] in DTYPE[mode] -> [H, n, dh]"""
    assert q.dtype == DTYPE[mode], (q.dtype, mode)
    scale = q.shape[-1] ** -0.5
    if mode == "exact":
        return torch.softmax((q @ k.transpose(-1, -2)) * scale, -1) @ v
    if mode == "spec":
        return rn16(torch.softmax((rn16(q) @ rn16(k).transpose(-1, -2)) * scale, -1) @ rn16(v))
    if mode == "peer_a":
        return torch.nn.functional.scaled_dot_product_attention(q.half(), k.half(), v.half()).float()
    assert mode == "peer_b"
    s = (rn16(q) @ rn16(k).transpose(-1, -2)) * np.float32(scale)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    return rn16((rn16(p) @ rn16(v)) / p.sum(-1, keepdim=True))


def self_block(x, enc, sd, p, heads, dtype, mode):
    """lg_f64.self_block with the attention above"""
    n, d = x.shape
    dh = d // heads
    qkv = lg_f64._linear(x, sd, p, "Wqkv", dtype).reshape(n, heads, dh, 3).permute(1, 0, 2, 3)
    q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
    q, k = lg_f64.apply_rotary(enc, q), lg_f64.apply_rotary(enc, k)
    ctx = attention(q.contiguous(), k.contiguous(), v.contiguous(), mode).transpose(0, 1).reshape(n, d)
    return lg_f64.ffn(x, lg_f64._linear(ctx, sd, p, "out_proj", dtype), sd, p, dtype)


def cross_block(x0, x1, sd, p, heads, dtype, mode):
    """lg_f64.cross_block with the attention above: qk0 / qk1 unscaled (the reference's flash branch, :293-314)"""
    (n, d), m = x0.shape, x1.shape[0]
    dh = d // heads
    split = lambda t, r: t.reshape(r, heads, dh).transpose(0, 1).contiguous()  # noqa: E731  [H, rows, dh]
    qk0, qk1 = split(lg_f64._linear(x0, sd, p, "to_qk", dtype), n), split(lg_f64._linear(x1, sd, p, "to_qk", dtype), m)
    v0, v1 = split(lg_f64._linear(x0, sd, p, "to_v", dtype), n), split(lg_f64._linear(x1, sd, p, "to_v", dtype), m)
    m0 = attention(qk0, qk1, v1, mode).transpose(0, 1).reshape(n, d)
    m1 = attention(qk1, qk0, v0, mode).transpose(0, 1).reshape(m, d)
    return (lg_f64.ffn(x0, lg_f64._linear(m0, sd, p, "to_out", dtype), sd, p, dtype),
            lg_f64.ffn(x1, lg_f64._linear(m1, sd, p, "to_out", dtype), sd, p, dtype))


@contextlib.contextmanager
def blocks(mode):
    """lg_f64's two blocks replaced by the flash ones in `mode`; restored on exit"""
    saved = lg_f64.self_block, lg_f64.cross_block
    lg_f64.self_block = lambda x, enc, sd, p, heads, dtype: self_block(x, enc, sd, p, heads, dtype, mode)
    lg_f64.cross_block = lambda x0, x1, sd, p, heads, dtype: cross_block(x0, x1, sd, p, heads, dtype, mode)
    try:
        yield
    finally:
        lg_f64.self_block, lg_f64.cross_block = saved


def forward(sd, kpts0, desc0, kpts1, desc1, mode="spec", **kw):
    """lg_f64.forward (same arguments and outputs) under the flash contract in `mode`"""
    with blocks(mode):
        return lg_f64.forward(sd, kpts0, desc0, kpts1, desc1, dtype=DTYPE[mode], **kw)


def attention_np(Q, K, V, mode="spec"):
    """the attention alone on numpy arrays [H, rows, dh] -> float64 numpy"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DTYPE[mode])  # noqa: E731
    with torch.no_grad():
        return attention(t(Q), t(K), t(V), mode).to(torch.float64).numpy()
