"""LightGlue's forward for ONE pair, written from its equations in plain torch on the CPU: float64 by default (the exact answer the
kernels and the oracle are measured against), float32 on request (a second fp32 implementation next to the oracle).  Not collected
by pytest (no test_ prefix).  Line numbers cite the reference's core/modules/matchers/lightglue.py.

Inputs: the numpy state dict with the reference's key names (an optional `prefix` in front of them), keypoints [n, >=2] (first two
columns), descriptors [n, input_dim], the image size of EACH side, the filter threshold.  The head count and the layer count are
read off the weights (posenc.Wr is [head_dim / 2, 2]; transformers.<i>.* per layer)."""
import math

import numpy as np
import torch


def _w(sd, prefix, key, dtype):
    return torch.from_numpy(np.ascontiguousarray(sd[prefix + key])).to(dtype)


def _linear(x, sd, prefix, key, dtype):
    return x @ _w(sd, prefix, key + ".weight", dtype).T + _w(sd, prefix, key + ".bias", dtype)


def normalize_keypoints(kpts, size, dtype):
    """:137-148 with the size given per side (:535-538): (k - size / 2) / (max(size) / 2)"""
    size = torch.tensor([float(size[0]), float(size[1])], dtype=dtype)
    return (kpts - size / 2) / (size.max() / 2)


def rotary(kpts, Wr):
    """:151-175: projected = k Wr^T [n, dh/2]; cos / sin each repeated twice along the head dimension -> [2, n, dh]"""
    p = kpts @ Wr.T
    return torch.stack([torch.cos(p), torch.sin(p)], 0).repeat_interleave(2, dim=-1)


def apply_rotary(enc, t):
    """:151-159: t * cos + rotate_half(t) * sin, rotate_half maps each adjacent pair (x1, x2) to (-x2, x1); t [H, n, dh]"""
    x1, x2 = t[..., 0::2], t[..., 1::2]
    rot = torch.stack([-x2, x1], -1).flatten(-2)
    return t * enc[0] + rot * enc[1]


def ffn(x, message, sd, p, dtype):
    """Linear(2d, 2d) -> LayerNorm(2d, eps 1e-5) -> exact (erf) GELU -> Linear(2d, d), added to the residual (:253-258, :327-328)"""
    h = _linear(torch.cat([x, message], -1), sd, p, "ffn.0", dtype)
    mu = h.mean(-1, keepdim=True)
    var = ((h - mu) ** 2).mean(-1, keepdim=True)
    h = (h - mu) / torch.sqrt(var + 1e-5) * _w(sd, p, "ffn.1.weight", dtype) + _w(sd, p, "ffn.1.bias", dtype)
    h = 0.5 * h * (1 + torch.erf(h / math.sqrt(2.0)))
    return x + _linear(h, sd, p, "ffn.3", dtype)


def self_block(x, enc, sd, p, heads, dtype):
    """:240-273: Wqkv's output rows are laid out (head, dim, 3); rotary on q and k; softmax(q k^T / sqrt(dh)) v"""
    n, d = x.shape
    dh = d // heads
    qkv = _linear(x, sd, p, "Wqkv", dtype).reshape(n, heads, dh, 3).permute(1, 0, 2, 3)  # [H, n, dh, 3]
    q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
    q, k = apply_rotary(enc, q), apply_rotary(enc, k)
    attn = torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5, -1)
    ctx = (attn @ v).transpose(0, 1).reshape(n, d)
    return ffn(x, _linear(ctx, sd, p, "out_proj", dtype), sd, p, dtype)


def cross_block(x0, x1, sd, p, heads, dtype):
    """:275-331: one projection qk per side, both scaled by dh^-1/4; softmax of sim along each direction"""
    (n, d), m = x0.shape, x1.shape[0]
    dh = d // heads
    split = lambda t, r: t.reshape(r, heads, dh).transpose(0, 1)  # noqa: E731  [H, rows, dh]
    qk0 = split(_linear(x0, sd, p, "to_qk", dtype), n) * dh ** -0.25
    qk1 = split(_linear(x1, sd, p, "to_qk", dtype), m) * dh ** -0.25
    v0, v1 = split(_linear(x0, sd, p, "to_v", dtype), n), split(_linear(x1, sd, p, "to_v", dtype), m)
    sim = qk0 @ qk1.transpose(-1, -2)  # [H, n, m]
    m0 = torch.softmax(sim, -1) @ v1
    m1 = torch.softmax(sim.transpose(-1, -2), -1) @ v0
    m0, m1 = m0.transpose(0, 1).reshape(n, d), m1.transpose(0, 1).reshape(m, d)
    return (ffn(x0, _linear(m0, sd, p, "to_out", dtype), sd, p, dtype),
            ffn(x1, _linear(m1, sd, p, "to_out", dtype), sd, p, dtype))


def log_assignment(x0, x1, sd, p, dtype):
    """:365-399: final_proj / d^(1/4), sim = mdesc0 mdesc1^T; log_softmax along rows + along columns + logsigmoid(z0) +
    logsigmoid(z1); the dustbin column / row hold logsigmoid(-z); the corner is 0"""
    n, d = x0.shape
    m = x1.shape[0]
    md0 = _linear(x0, sd, p, "final_proj", dtype) / d ** 0.25
    md1 = _linear(x1, sd, p, "final_proj", dtype) / d ** 0.25
    sim = md0 @ md1.T
    z0 = _linear(x0, sd, p, "matchability", dtype)  # [n, 1]
    z1 = _linear(x1, sd, p, "matchability", dtype)
    out = torch.zeros((n + 1, m + 1), dtype=dtype)
    out[:n, :m] = (torch.log_softmax(sim, 1) + torch.log_softmax(sim, 0)
                   + torch.nn.functional.logsigmoid(z0) + torch.nn.functional.logsigmoid(z1).T)
    out[:n, m] = torch.nn.functional.logsigmoid(-z0[:, 0])
    out[n, :m] = torch.nn.functional.logsigmoid(-z1[:, 0])
    return out


# smallest x with float32 exp(x) > 0: exp rounds to the smallest subnormal 2^-149 from half of it, 2^-150, up
EXP_F32_EDGE = -150 * math.log(2.0)


def filter_edge(th):
    """the log_assignment value at which the filter's fp32 test exp(max) > th flips"""
    th = float(np.float32(th))
    return EXP_F32_EDGE if th <= 0 else math.log(th)


def filter_matches(la, th):
    """:402-418 on [n+1, m+1].  The DECISION follows the reference's fp32 rule: the maxima are rounded to fp32 and exp'd in fp32
    before `> th` (an f64 exp never underflows; in fp32 a mutual best is kept only while exp(max) > 0, down to about -103.97
    through the subnormal band).  The scores are exp of the maxima in the working dtype."""
    s = la[:-1, :-1]
    n, m = s.shape
    max0, m0 = s.max(1)
    m1 = s.max(0).indices
    mutual0 = torch.arange(n) == m1[m0]
    mutual1 = torch.arange(m) == m0[m1]
    e32 = torch.exp(max0.to(torch.float32))
    valid0 = mutual0 & (e32 > float(np.float32(th)))
    valid1 = mutual1 & valid0[m1]
    zero = torch.zeros((), dtype=la.dtype)
    ms0 = torch.where(mutual0, torch.exp(max0), zero)
    ms1 = torch.where(mutual1, ms0[m1], zero)
    return (torch.where(valid0, m0, -1).numpy(), torch.where(valid1, m1, -1).numpy(), ms0.numpy(), ms1.numpy(),
            max0.numpy())


def top2_gaps(s, axis):
    """best minus second best of every row (axis=1) / column (axis=0) of s; inf where there is no second candidate"""
    if s.shape[axis] < 2:
        return np.full(s.shape[1 - axis], np.inf)
    t = np.sort(s, axis=axis)
    return (t[:, -1] - t[:, -2]) if axis == 1 else (t[-1] - t[-2])


def forward(sd, kpts0, desc0, kpts1, desc1, size0=(260, 346), size1=(260, 346), filter_threshold=0.0, prefix="",
            dtype=torch.float64, n_layers=None, num_heads=None):
    """One pair.  Returns numpy arrays: log_assignment [n+1, m+1]; matches0/1, scores0/1; layers = [(desc0, desc1) after each
    layer]; the decision margins row_gap [n], col_gap [m] (top-2 gaps of the [n, m] block) and edge_dist [n] (|row maximum -
    the filter's edge|)."""
    with torch.no_grad():
        if n_layers is None:
            n_layers = sum(1 for k in sd if k.startswith(prefix + "transformers.") and k.endswith(".self_attn.Wqkv.weight"))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
        x0, x1 = t(desc0), t(desc1)
        if prefix + "input_proj.weight" in sd:  # input_dim != descriptor_dim (:450-453)
            x0, x1 = _linear(x0, sd, prefix, "input_proj", dtype), _linear(x1, sd, prefix, "input_proj", dtype)
        d = x0.shape[1]
        Wr = _w(sd, prefix, "posenc.Wr.weight", dtype)
        dh = 2 * Wr.shape[0]
        heads = d // dh if num_heads is None else num_heads
        assert heads * dh == d, (heads, dh, d)
        enc0 = rotary(normalize_keypoints(t(np.asarray(kpts0)[:, :2]), size0, dtype), Wr)
        enc1 = rotary(normalize_keypoints(t(np.asarray(kpts1)[:, :2]), size1, dtype), Wr)
        layers = []
        for i in range(n_layers):  # TransformerLayer.forward (:347-362): self on each side, then cross
            p = f"{prefix}transformers.{i}."
            x0 = self_block(x0, enc0, sd, p + "self_attn.", heads, dtype)
            x1 = self_block(x1, enc1, sd, p + "self_attn.", heads, dtype)
            x0, x1 = cross_block(x0, x1, sd, p + "cross_attn.", heads, dtype)
            layers.append((x0.numpy(), x1.numpy()))
        la = log_assignment(x0, x1, sd, f"{prefix}log_assignment.{n_layers - 1}.", dtype)
        m0, m1, s0, s1, max0 = filter_matches(la, filter_threshold)
        s = la[:-1, :-1].numpy()
        return dict(log_assignment=la.numpy(), matches0=m0, matches1=m1, scores0=s0, scores1=s1, layers=layers,
                    row_gap=top2_gaps(s, 1), col_gap=top2_gaps(s, 0), edge_dist=np.abs(max0 - filter_edge(filter_threshold)))
