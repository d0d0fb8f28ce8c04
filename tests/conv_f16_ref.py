"""The contract of the opt-in fp16 convolutions as code; not collected by pytest.

A covered layer: Conv2d(3x3 pad 1 | 1x1) + bias -> [ReLU] -> [BN(eval) affine] -> [MaxPool 2x2] with cin % 8 == 0, whose input
activations and weights are rounded to binary16 (`tensor.half()`: nearest even, overflow to infinity), whose products are exact and
summed in fp32 in any order, and whose epilogue is fp32.  `spec` evaluates it in float64 (the exact sum of the exact products);
`peer_a` / `peer_b` are two independent fp32 evaluations of the same rounded operands (their distance from `spec` is what fp32
summation costs); `stack_forward` applies the layer rule to an extractor's `_stacks()`.
"""
import torch
import torch.nn.functional as F


def rh(t):
    """the contract's rounding of an fp32 tensor"""
    return t.float().half().float()


def covered(cin, first):
    return (not first) and cin % 8 == 0


def _epilogue(y, bias, scale, shift, relu, pool):
    """bias -> ReLU -> affine -> pool in y's dtype (the constants are fp32 data, widened exactly)"""
    if bias is not None:
        y = y + bias.to(y.dtype).view(1, -1, 1, 1)
    if relu:
        y = y.clamp_min(0)
    if scale is not None:
        y = y * scale.to(y.dtype).view(1, -1, 1, 1) + shift.to(y.dtype).view(1, -1, 1, 1)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    return y


def spec(x, w, bias=None, scale=None, shift=None, relu=False, pool=False, rounding=True):
    """float64: conv2d of the rounded operands, epilogue in float64.  x [B,cin,H,W], w [cout,cin,ks,ks] fp32 CPU tensors."""
    xr, wr = (rh(x), rh(w)) if rounding else (x, w)
    y = F.conv2d(xr.double(), wr.double(), None, padding=w.shape[-1] // 2)
    return _epilogue(y, bias, scale, shift, relu, pool)


def abs_sum(x, w, rounding=True):
    """sum |x w| over a layer's K = ks^2 cin products, per output, float64"""
    xr, wr = (rh(x), rh(w)) if rounding else (x, w)
    return F.conv2d(xr.double().abs(), wr.double().abs(), None, padding=w.shape[-1] // 2)


def bound(x, w, got_like, scale=None, pool=False, factor=1.0):
    """the a-priori bound of K fp32 additions, K 2^-24 sum|x w|, carried through the epilogue by |scale|, plus 4 ulp of the value
    (the epilogue's own roundings); under a pool the largest bound of the window"""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    b = factor * K * 2.0 ** -24 * abs_sum(x, w)
    if scale is not None:
        b = b * scale.double().abs().view(1, -1, 1, 1)
    if pool:
        b = F.max_pool2d(b, 2, 2)
    return b + 4 * 2.0 ** -23 * got_like.double().abs()


def peer_a(x, w, bias=None, scale=None, shift=None, relu=False, pool=False, rounding=True):
    """torch's fp32 conv2d of the rounded operands with the fp32 epilogue (CPU)"""
    xr, wr = (rh(x), rh(w)) if rounding else (x, w)
    y = F.conv2d(xr.float(), wr.float(), None, padding=w.shape[-1] // 2)
    return _epilogue(y, bias, scale, shift, relu, pool)


def peer_b(native, x, w, bias=None, scale=None, shift=None, relu=False, pool=False, rounding=True, dev="cuda:0"):
    """today's einx_conv_block (the oracle-exact fp32 kernel) on the PRE-rounded operands: the same exact products, another order"""
    xr, wr = (rh(x), rh(w)) if rounding else (x.float(), w)
    layer = native.ConvLayer(wr.to(dev), None if bias is None else bias.to(dev), None, relu=relu, pool=pool)
    if scale is not None:  # the folded affine as given (no einx_bn_fold in between)
        layer.scale, layer.shift = scale.to(dev).contiguous(), shift.to(dev).contiguous()
        layer.desc.scale, layer.desc.shift = layer.scale.data_ptr(), layer.shift.data_ptr()
    return layer(xr.to(dev).contiguous()).cpu()


def bn_fold(bn):
    """einx_bn_fold's fp32 arithmetic: scale = g / sqrt(var + eps); shift = b - mean * scale"""
    s = bn.weight.detach().float().cpu() / torch.sqrt(bn.running_var.detach().float().cpu() + torch.tensor(bn.eps, dtype=torch.float32))
    return s, bn.bias.detach().float().cpu() - bn.running_mean.detach().float().cpu() * s


def stack_forward(ext, x, layer_fn, rounding=True):
    """The layer rule over an extractor's `_stacks()`: the first layer un-rounded, every other layer with cin % 8 == 0 rounded.
    x: the network's input [B,cin,H,W] (already scaled, H and W multiples of the cell size: no padding fold); layer_fn(x, w, bias,
    scale, shift, relu, pool, rounding) evaluates one layer (spec / peer_a / a peer_b closure).  -> (backbone_feats, logits, raw)."""
    bb, det, desc = ext._stacks()

    def run(t, block, pool, first):
        conv, bn, relu = ext._spec(block)
        scale, shift = (None, None) if bn is None else bn_fold(bn)
        w = conv.weight.detach().float().cpu()
        b = None if conv.bias is None else conv.bias.detach().float().cpu()
        return layer_fn(t, w, b, scale, shift, relu, pool, rounding and covered(w.shape[1], first))

    t = x
    for i, (block, pool) in enumerate(bb):
        t = run(t, block, pool, i == 0)
    feats = t
    outs = []
    for head in (det, desc):
        t = feats
        for block in head:
            t = run(t, block, False, False)
        outs.append(t)
    return feats, outs[0], outs[1]
