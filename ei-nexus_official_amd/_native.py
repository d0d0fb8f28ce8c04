"""Torch-tensor front door of the C ABI: validates device/dtype/contiguity, allocates outputs
and workspaces with torch (caching allocator, stream ordered) and enqueues the HIP kernels on the
current stream.  No arithmetic happens here; PyTorch is memory + stream plumbing only.
"""
import ctypes
import threading
import os
import math

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, DetectParams, check

F32 = torch.float32


def lib():
    return _lib.load()


I32, I64, U8 = torch.int32, torch.int64, torch.uint8


def _dev_check(*tensors, dt=F32):
    """Every tensor must be a contiguous HIP tensor of dtype `dt`: the kernels read raw pointers and
    assume the element size (an fp16/fp64/int64 tensor would be read out of bounds or as garbage)."""
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(
                "einx: tensors must live on a HIP device (torch device type 'cuda'); there is no CPU path. "
                f"Got a tensor on {t.device}.")
        if t.dtype != dt:
            raise TypeError(f"einx: expected a {dt} tensor, got {t.dtype} (the kernels compute in fp32 with int32 counts/indices; "
                            "cast at the call site, e.g. x.float())")
        if not t.is_contiguous():
            raise RuntimeError("einx: tensors must be contiguous")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _first_device(obj, depth=0):
    """HIP device of the first tensor found in a call argument (tensor, feats dict / list of tensors, PairBatch, BatchedFeats)."""
    if torch.is_tensor(obj):
        return obj.device if obj.device.type == "cuda" else None
    if depth > 2 or obj is None or isinstance(obj, (str, int, float, bool)):
        return None
    if isinstance(obj, dict):
        obj = list(obj.values())
    if isinstance(obj, (list, tuple)):
        for v in obj[:16]:
            d = _first_device(v, depth + 1)
            if d is not None:
                return d
        return None
    for name in ("desc", "score", "kpts"):  # PairBatch / BatchedFeats
        t = getattr(obj, name, None)
        if torch.is_tensor(t) and t.device.type == "cuda":
            return t.device
    return None


_scope = threading.local()


def on_input_device(fn):
    """The kernels are launched through ctypes on the stream of the INPUTS' device; HIP wants that device to be the current
    one.  torch's own operators switch devices per call, the reference therefore works with a model on cuda:1 while
    cuda:0 is current -- this decorator gives the drop-in's entry points the same behaviour (no-op on the current device).
    Entry points call each other (EIM.forward -> extract_batched -> ...): only the outermost one looks for the device, the
    nested ones run under its decision (their tensors derive from its inputs) -- the scan was 60 us of a 0.8 ms single-pair
    forward (round 5)."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        if getattr(_scope, "depth", 0):
            return fn(*args, **kwargs)
        dev = None
        for a in args:
            if type(a) is torch.Tensor:  # the common case, without the generic walk
                if a.device.type == "cuda":
                    dev = a.device
                    break
        if dev is None:
            for a in list(args) + list(kwargs.values()):  # `self` (a module) holds no tensor attribute the scan looks at
                dev = _first_device(a)
                if dev is not None:
                    break
        if dev is None:
            return fn(*args, **kwargs)
        _scope.depth = 1
        try:
            if dev.index is None or dev.index == torch.cuda.current_device():
                return fn(*args, **kwargs)
            with torch.cuda.device(dev):
                return fn(*args, **kwargs)
        finally:
            _scope.depth = 0

    return wrapped


def _workspace(nbytes, device):
    """The caller-owned scratch of one op call: `nbytes` is what the op's *_ws_bytes query returned.  Every workspace of the
    package is allocated here (the one seam tests/test_workspace_gpu.py puts its guard bytes behind)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _stream(t):
    # (torch.cuda.current_stream builds a Stream object per call: 6-7 us, nine times per forward)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(t.device.index if t.device.index is not None else torch.cuda.current_device()))


def padder_pads(h, w, p):
    """Padder.__init__ arithmetic (reference core/modules/utils/util.py:6-15) -> (w0, w1, h0, h1)."""
    hp = (((h // p) + 1) * p - h) % p
    wp = (((w // p) + 1) * p - w) % p
    return (wp // 2, wp - wp // 2, hp // 2, hp - hp // 2)


def topk_ranks(N, k):
    """Indices torch.quantile(q,'midpoint') gathers, in the reference's fp32 arithmetic."""
    q = np.float32(N - k) / np.float32(N)
    rank = np.float32(q * np.float32(N - 1))
    return int(math.floor(float(rank))), int(math.ceil(float(rank)))


def topk_capacity(N, top_k, det_thr):
    if not top_k or top_k >= N or det_thr < 1.0:
        return N
    lo, _ = topk_ranks(N, int(top_k))
    return N - 1 - lo


# ------------------------------------------------------------------------------ conv
class ConvLayer:
    """Kernel-native image of one conv block: weights repacked on device, BN(eval) folded into a
    per-channel (scale, shift) by einx_bn_fold (IEEE fp32, same op order as the oracle)."""

    def __init__(self, weight, bias, bn=None, relu=True, pool=False):
        _dev_check(weight)
        cout, cin, ks, _ = weight.shape
        self.cin, self.cout, self.ks, self.relu, self.pool = cin, cout, ks, relu, pool
        L = lib()
        w = weight.detach().to(F32).contiguous()
        self.w_native = torch.empty(L.einx_conv_weight_elems(cin, cout, ks), dtype=F32, device=w.device)
        check(L.einx_conv_repack(_ptr(w), cin, cout, ks, _ptr(self.w_native), _stream(w)), "einx_conv_repack")
        self.bias = None if bias is None else bias.detach().to(F32).contiguous()
        self.scale = self.shift = None
        if bn is not None:
            g, b, mean, var = [t.detach().to(w.device, F32).contiguous() for t in bn[:4]]
            self.scale = torch.empty(cout, dtype=F32, device=w.device)
            self.shift = torch.empty(cout, dtype=F32, device=w.device)
            check(L.einx_bn_fold(_ptr(g), _ptr(b), _ptr(mean), _ptr(var), float(bn[4]), cout, _ptr(self.scale), _ptr(self.shift),
                                 _stream(w)), "einx_bn_fold")
            self._keep_bn = (g, b, mean, var)
        self.desc = ConvDesc(self.w_native.data_ptr(), 0 if self.bias is None else self.bias.data_ptr(),
                             0 if self.scale is None else self.scale.data_ptr(), 0 if self.shift is None else self.shift.data_ptr(),
                             cin, cout, ks, int(relu), int(pool))
        self._keep = w  # repack reads it asynchronously
        self._f16 = None

    def f16(self):
        """The binary16 weight image and its descriptor (_lib.ConvDescF16) for the opt-in fp16 convolutions, built
        at the first use beside the fp32 image and dropped with it; None for a layer the mode does not cover (cin % 8 != 0)."""
        if self.cin % 8 != 0:
            return None
        if self._f16 is None:
            L = lib()
            w = self._keep
            self.w_f16 = torch.empty(L.einx_conv_weight_elems_f16(self.cin, self.cout, self.ks), dtype=torch.float16, device=w.device)
            check(L.einx_conv_repack_f16(_ptr(w), self.cin, self.cout, self.ks, _ptr(self.w_f16), _stream(w)), "einx_conv_repack_f16")
            self._f16 = _lib.ConvDescF16(ctypes.sizeof(_lib.ConvDescF16), self.w_f16.data_ptr(), self.desc.bias, self.desc.scale, self.desc.shift,
                                         self.cin, self.cout, self.ks, int(self.relu), int(self.pool))
        return self._f16

    def __call__(self, x, fold=None, half=False):
        """x [B,cin,Hs,Ws]; fold = (h0, w0, H, W) applies replicate padding on the fly.  half: through einx_conv_block_f16 where
        einx_conv_f16_plan covers the layer and the call (never with a fold)."""
        _dev_check(x)
        B, C, Hs, Ws = x.shape
        if C != self.cin:
            raise ValueError(f"conv expects {self.cin} input channels, got {C}")
        h0, w0, H, W = fold if fold is not None else (0, 0, Hs, Ws)
        Ho, Wo = (H // 2, W // 2) if self.pool else (H, W)
        out = torch.empty((B, self.cout, Ho, Wo), dtype=F32, device=x.device)
        L = lib()
        if half and (h0, w0, H, W) == (0, 0, Hs, Ws) and L.einx_conv_f16_plan(self.cin, self.cout, self.ks, int(self.pool), B, H, W) is not None:
            check(L.einx_conv_block_f16(_ptr(x), B, H, W, ctypes.byref(self.f16()), _ptr(out), _stream(x)), "einx_conv_block_f16")
            return out
        check(L.einx_conv_block(_ptr(x), B, Hs, Ws, h0, w0, H, W, ctypes.byref(self.desc), _ptr(out), _stream(x)), "einx_conv_block")
        return out


def bn_tuple(bn):
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


def div_inplace(x, divisor):
    _dev_check(x)
    check(lib().einx_div_inplace(_ptr(x), x.numel(), float(divisor), _stream(x)), "einx_div_inplace")
    return x


def image_prepare(image, divisor):
    """SuperPointv1's input handling for RGB / non-contiguous images (superpoint_extractor.py:372-376): `image /= divisor` in
    place THROUGH the tensor's strides, and the network's contiguous single-channel input (C == 3: kornia's rgb_to_grayscale of
    the scaled image) as a new tensor.  divisor 1.0 = the image has been scaled by an earlier call (x / 1 == x)."""
    if image.device.type != "cuda":
        raise RuntimeError(f"einx: input must be on a HIP device (no CPU path), got {image.device}")
    if image.dtype != F32:
        raise TypeError("einx extractors compute in fp32; pass a float32 tensor")
    B, C, H, W = image.shape  # any strides: the kernel walks them
    gray = torch.empty((B, 1, H, W), dtype=F32, device=image.device)
    if gray.numel():
        sb, sc, sh, sw = image.stride()
        check(lib().einx_image_prepare(_ptr(image), B, C, H, W, sb, sc, sh, sw, float(divisor), _ptr(gray), _stream(image)), "einx_image_prepare")
    return gray


# ------------------------------------------------------------------------------ detector
MASK_PAD_ZERO, MASK_PAD_REPLICATE = 0, 1  # include/einx.h: EINX_MASK_PAD_*


def mask_bytes(mask):
    """mask of any dtype -> (uint8 view / copy the score kernels read, the Padder's padding rule for that dtype).  The reference
    pads a bool mask with zeros and every other dtype by repeating its edge pixels (core/modules/utils/util.py:17-32); of a mask
    that is not bool the non-zero pixels are the visible ones (stated departures, for signed and denormal values:
    the reference tests `conv(mask.float(), ones / 9) > 0`, EventExtractors.py:544-550)."""
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8), MASK_PAD_ZERO
    return mask.ne(0).contiguous().view(torch.uint8), MASK_PAD_REPLICATE


def score_map(logits, mask=None, pads=(0, 0, 0, 0), dilate=False, border=0):
    """-> (probability [B,C,hc,wc], score [B,1,Hp,Wp]).  mask [B,1,H,W]: bool, or any other dtype (see mask_bytes)."""
    _dev_check(logits)
    if mask is not None and mask.device.type != "cuda":
        raise RuntimeError(f"einx: the mask must live on a HIP device, got {mask.device}")
    B, C, hc, wc = logits.shape
    cell = 8 if C == 65 else 1
    Hp, Wp = hc * cell, wc * cell
    w0, w1, h0, h1 = pads
    H, W = Hp - h0 - h1, Wp - w0 - w1
    prob = torch.empty_like(logits)
    score = torch.empty((B, 1, Hp, Wp), dtype=F32, device=logits.device)
    m8, pad = None, MASK_PAD_ZERO
    if mask is not None:
        if tuple(mask.shape[-2:]) != (H, W):
            raise ValueError(f"mask spatial size {tuple(mask.shape[-2:])} does not match the image ({H},{W})")
        m8, pad = mask_bytes(mask)
    check(lib().einx_score_map_pad(_ptr(logits), B, C, hc, wc, _ptr(m8), pad, H, W, h0, w0, int(dilate), int(border), _ptr(prob),
                                   _ptr(score), _stream(logits)), "einx_score_map_pad")
    return prob, score


def dense_positions(score, ordering="yx"):
    """score [B,1,H,W] (unpadded) -> [B,H*W,3] dense keypoint list (get_dense_positions)."""
    _dev_check(score)
    B, _, H, W = score.shape
    out = torch.empty((B, H * W, 3), dtype=F32, device=score.device)
    check(lib().einx_dense_positions(_ptr(score), B, H, W, int(ordering == "xy"), _ptr(out), _stream(score)), "einx_dense_positions")
    return out


def remove_border(score, border):
    _dev_check(score)
    B = score.shape[0]
    Hp, Wp = score.shape[-2:]
    check(lib().einx_remove_border(_ptr(score), int(score.numel() // (Hp * Wp)), Hp, Wp, int(border), _stream(score)), "einx_remove_border")
    return score


class Detection:
    """Device-side result of einx_detect for a batch."""
    __slots__ = ("positions", "indices", "counts", "thr", "not_converged", "nms", "cap", "padded", "pads", "stale")


def detect(score, *, top_k, radius, det_thr, pads=(0, 0, 0, 0), ordering="yx", cap=None, nms_iters=8, want_nms=True):
    """score [B,1,Hp,Wp] or [B,Hp,Wp] (already masked/border-zeroed)."""
    _dev_check(score)
    B = score.shape[0]
    Hp, Wp = score.shape[-2:]
    w0, w1, h0, h1 = pads
    H, W = Hp - h0 - h1, Wp - w0 - w1
    N = Hp * Wp
    if cap is None:
        cap = topk_capacity(N, top_k, det_thr)
    cap = max(int(cap), 1)
    p = DetectParams(B, Hp, Wp, H, W, h0, w0, int(radius), int(top_k or 0), float(det_thr), int(ordering == "xy"), cap, int(nms_iters))
    L = lib()
    dev = score.device
    ws = _workspace(L.einx_detect_ws_bytes(ctypes.byref(p)), dev)
    d = Detection()
    d.positions = torch.empty((B, cap, 3), dtype=F32, device=dev)
    d.indices = torch.empty((B, cap), dtype=torch.int32, device=dev)
    d.counts = torch.empty((B,), dtype=torch.int32, device=dev)
    d.thr = torch.empty((B,), dtype=F32, device=dev)
    d.not_converged = torch.empty((B,), dtype=torch.int32, device=dev)
    d.nms = torch.empty((B, H, W), dtype=F32, device=dev) if want_nms else None
    d.cap, d.padded, d.pads = cap, (Hp, Wp), pads
    check(L.einx_detect(_ptr(score), ctypes.byref(p), _ptr(ws), _ptr(d.nms), _ptr(d.positions), _ptr(d.indices), _ptr(d.counts),
                        _ptr(d.thr), _ptr(d.not_converged), _stream(score)), "einx_detect")
    return d


# ------------------------------------------------------------------------------ descriptors
def desc_sample(raw, indices, counts, padded_size, bilinear, scale, raw_cl=None):
    """raw [B,D,hc,wc].  raw_cl: the channels-last copy [B,hc*wc,D] from normalize_map(want_cl=True);
    when given (bilinear only) the taps are read from it -- same values, coalesced rows."""
    _dev_check(raw, raw_cl)
    _dev_check(indices, counts, dt=I32)
    B, D, hc, wc = raw.shape
    cap = indices.shape[1]
    out = torch.empty((B, cap, D), dtype=F32, device=raw.device)
    use_cl = raw_cl is not None and bilinear
    src = raw_cl if use_cl else raw
    check(lib().einx_desc_sample(_ptr(src), B, D, hc, wc, int(padded_size[0]), int(padded_size[1]), int(bilinear), int(use_cl),
                                 _ptr(indices), _ptr(counts), cap, float(scale), _ptr(out), _stream(raw)), "einx_desc_sample")
    return out


SUBPIXEL_DMAX = 0.5 - 2.0 ** -10  # largest sub-pixel offset per axis (csrc/subpixel.hip)


def desc_sample_pos(raw, positions, counts, padded_size, scale, ordering="yx", raw_cl=None):
    """raw [B,D,hc,wc] sampled bilinearly (zero padding, align_corners=False) at the float positions [B,cap,>=2] of the padded
    frame, then normalised: the reference's sparsify_low_resolution_descriptors for ANY position -> [B,cap,D].  raw_cl: see
    desc_sample."""
    _dev_check(raw, raw_cl, positions)
    _dev_check(counts, dt=I32)
    B, D, hc, wc = raw.shape
    if positions.dim() != 3 or positions.shape[0] != B or positions.shape[2] < 2 or counts.numel() != B:
        raise ValueError(f"einx: positions must be [B, cap, >= 2] and counts [B] for B = {B}, got {tuple(positions.shape)} and {tuple(counts.shape)}")
    cap = positions.shape[1]
    out = torch.empty((B, cap, D), dtype=F32, device=raw.device)
    use_cl = raw_cl is not None
    check(lib().einx_desc_sample_pos(_ptr(raw_cl if use_cl else raw), B, D, hc, wc, int(padded_size[0]), int(padded_size[1]), int(use_cl),
                                     _ptr(positions), int(positions.shape[2]), int(ordering == "xy"), _ptr(counts), cap, float(scale), _ptr(out),
                                     _stream(raw)), "einx_desc_sample_pos")
    return out


def refine_keypoints(score, indices, counts, positions, pads=(0, 0, 0, 0), ordering="yx", raw=None, raw_cl=None, sparse_desc=None, scale=1.0):
    """Sub-pixel refinement of detected keypoints IN PLACE (einx.h: einx_refine_keypoints): columns 0 and 1 of positions
    [B,cap,3] from the parabola through each peak of score [B,1,Hp,Wp] / [B,Hp,Wp] and its neighbours; with sparse_desc [B,cap,D]
    (cell-8 networks) the keypoints' descriptor rows are resampled from raw [B,D,hc,wc] (raw_cl: its channels-last copy) at
    the refined positions.  Without sparse_desc: positions only.  -> positions"""
    _dev_check(score, positions, raw, raw_cl, sparse_desc)
    _dev_check(indices, counts, dt=I32)
    B = score.shape[0]
    Hp, Wp = score.shape[-2:]
    w0, w1, h0, h1 = pads
    cap = indices.shape[1]
    if tuple(positions.shape) != (B, cap, 3) or tuple(indices.shape) != (B, cap) or counts.numel() != B or score.numel() != B * Hp * Wp:
        raise ValueError(f"einx: refine_keypoints wants score [B,Hp,Wp], indices [B,cap], counts [B] and positions [B,cap,3]; got "
                         f"{tuple(score.shape)}, {tuple(indices.shape)}, {tuple(counts.shape)}, {tuple(positions.shape)}")
    bilinear = sparse_desc is not None
    D = hc = wc = 0
    src = None
    if bilinear:
        if raw is None:
            raise ValueError("einx: resampling the descriptors needs the raw map")
        _, D, hc, wc = raw.shape
        if tuple(sparse_desc.shape) != (B, cap, D) or raw.shape[0] != B:
            raise ValueError(f"einx: sparse_desc must be [B,cap,D] = {(B, cap, D)}, got {tuple(sparse_desc.shape)}")
        src = raw_cl if raw_cl is not None else raw
    check(lib().einx_refine_keypoints(_ptr(score), B, Hp, Wp, Hp - h0 - h1, Wp - w0 - w1, h0, w0, int(ordering == "xy"), _ptr(indices), _ptr(counts),
                                      cap, _ptr(positions), _ptr(src), D, hc, wc, int(bilinear), int(bilinear and raw_cl is not None), float(scale),
                                      _ptr(sparse_desc), _stream(score)), "einx_refine_keypoints")
    return positions


def normalize_map(raw, scale, want_cl=False):
    """-> normalised map like `raw`; with want_cl also the channels-last copy [B,P,D] of the raw values."""
    _dev_check(raw)
    B, D = raw.shape[:2]
    P = int(raw.numel() // (B * D))
    out = torch.empty_like(raw)
    cl = torch.empty((B, P, D), dtype=F32, device=raw.device) if (want_cl and D <= 512) else None
    check(lib().einx_normalize_map(_ptr(raw), B, D, P, float(scale), _ptr(out), _ptr(cl), _stream(raw)), "einx_normalize_map")
    return (out, cl) if want_cl else out


def upsample_normalize(raw, padded_size, pads, scale):
    _dev_check(raw)
    B, D, hc, wc = raw.shape
    Hp, Wp = int(padded_size[0]), int(padded_size[1])
    w0, w1, h0, h1 = pads
    H, W = Hp - h0 - h1, Wp - w0 - w1
    out = torch.empty((B, D, H, W), dtype=F32, device=raw.device)
    nws = int(lib().einx_upsample_ws_bytes(B, H, W))
    ws = torch.empty((nws + 3) // 4, dtype=F32, device=raw.device)  # per-pixel norms handed from the first kernel to the second
    check(lib().einx_upsample_normalize(_ptr(raw), B, D, hc, wc, Hp, Wp, h0, w0, H, W, float(scale), _ptr(out), _ptr(ws), nws, _stream(raw)),
          "einx_upsample_normalize")
    return out


# ------------------------------------------------------------------------------ matching
class MatchResult:
    __slots__ = ("matches0", "matches1", "scores0", "scores1", "la", "mk0", "mk1", "nmatch", "ref0", "ref1", "mk0_flat", "mk1_flat", "stale", "stop",
                 "prune0", "prune1", "kept0", "kept1", "live")

    def __init__(self):
        self.mk0_flat = self.mk1_flat = None
        self.stale = None  # device int32 [1]: the matcher's weight watch (LightGlue), read back with the match counts
        self.stop = None  # device int32 [B]: the layer count each pair ran (LightGlue with early stopping only)
        # LightGlue with point pruning only: prune0/1 float32 [B,cap] (1 + the pruning steps a point survived), kept0/1
        # int64 [B,cap] (the survivors' original indices in compacted order, -1 behind them), live int32 [2B] (survivors per side)
        self.prune0 = self.prune1 = self.kept0 = self.kept1 = self.live = None


def mnn(desc0, n, desc1, m, want_la=True, ratio_thresh=None, distance_thresh=None, gather=None):
    """ratio_thresh / distance_thresh: find_nn's optional thresholds (MNN.py:12-22), falsy = off.
    gather = (kpts0, kpts1, cols): also the matched keypoints of every pair (gather_matches' r.mk0 / r.mk1 / r.nmatch), in the
    same call -- without thresholds the mutual check and the compaction are one launch."""
    _dev_check(desc0, desc1)
    _dev_check(n, m, dt=I32)
    B, cap0, D = desc0.shape
    cap1 = desc1.shape[1]
    L = lib()
    dev = desc0.device
    ws = _workspace(L.einx_mnn_ws_bytes(B, cap0, cap1), dev)
    r = MatchResult()
    r.matches0 = torch.empty((B, cap0), dtype=torch.int64, device=dev)
    r.matches1 = torch.empty((B, cap1), dtype=torch.int64, device=dev)
    r.scores0 = torch.empty((B, cap0), dtype=F32, device=dev)
    r.scores1 = torch.empty((B, cap1), dtype=F32, device=dev)
    r.la = torch.empty((B, cap0 + 1, cap1 + 1), dtype=F32, device=dev) if want_la else None
    r.ref0 = r.ref1 = None
    if ratio_thresh or distance_thresh:
        # the squared Python scalars are rounded to fp32 once, as torch does for `tensor <= scalar` / `scalar * tensor`
        r2 = float(np.float32(float(ratio_thresh) ** 2)) if ratio_thresh else 0.0
        t2 = float(np.float32(float(distance_thresh) ** 2)) if distance_thresh else 0.0
        check(L.einx_mnn_thresh(_ptr(desc0), _ptr(n), cap0, _ptr(desc1), _ptr(m), cap1, B, D, int(bool(ratio_thresh)), r2,
                                int(bool(distance_thresh)), t2, _ptr(ws), _ptr(r.matches0), _ptr(r.matches1), _ptr(r.scores0), _ptr(r.scores1),
                                _ptr(r.la), _stream(desc0)), "einx_mnn_thresh")
        return r if gather is None else gather_matches(r, gather[0], gather[1], n, gather[2])
    if gather is not None:
        k0, k1, cols = gather
        _dev_check(k0, k1)
        r.mk0 = torch.empty((B, cap0, cols), dtype=F32, device=dev)
        r.mk1 = torch.empty((B, cap0, cols), dtype=F32, device=dev)
        r.nmatch = torch.empty((B,), dtype=torch.int32, device=dev)
        check(L.einx_mnn_gather(_ptr(desc0), _ptr(n), cap0, _ptr(desc1), _ptr(m), cap1, B, D, _ptr(ws), _ptr(r.matches0), _ptr(r.matches1),
                                _ptr(r.scores0), _ptr(r.scores1), _ptr(r.la), _ptr(k0), _ptr(k1), int(cols), _ptr(r.mk0), _ptr(r.mk1),
                                _ptr(r.nmatch), _stream(desc0)), "einx_mnn_gather")
        return r
    check(L.einx_mnn(_ptr(desc0), _ptr(n), cap0, _ptr(desc1), _ptr(m), cap1, B, D, _ptr(ws), _ptr(r.matches0), _ptr(r.matches1),
                     _ptr(r.scores0), _ptr(r.scores1), _ptr(r.la), _stream(desc0)), "einx_mnn")
    return r


def gather_matches(r, kpts0, kpts1, n, cols):
    _dev_check(kpts0, kpts1)
    _dev_check(n, dt=I32)
    _dev_check(r.matches0, dt=I64)
    B, cap0, _ = kpts0.shape
    cap1 = kpts1.shape[1]
    dev = kpts0.device
    r.mk0 = torch.empty((B, cap0, cols), dtype=F32, device=dev)
    r.mk1 = torch.empty((B, cap0, cols), dtype=F32, device=dev)
    r.nmatch = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib().einx_gather_matches(_ptr(kpts0), _ptr(kpts1), _ptr(r.matches0), _ptr(n), cap0, cap1, B, cols, _ptr(r.mk0), _ptr(r.mk1),
                                    _ptr(r.nmatch), _stream(kpts0)), "einx_gather_matches")
    return r


def compact_matches(r):
    """r.mk0/r.mk1 [B,cap0,cols] + r.nmatch -> r.mk0_flat/r.mk1_flat [B*cap0,cols] packed pair after pair."""
    B, cap0, cols = r.mk0.shape
    if B == 1:  # one pair: its matched rows already sit at the front of mk0[0] / mk1[0] (no launch on the single-pair chain)
        r.mk0_flat, r.mk1_flat = r.mk0[0], r.mk1[0]
        return r
    r.mk0_flat = torch.empty((B * cap0, cols), dtype=F32, device=r.mk0.device)
    r.mk1_flat = torch.empty((B * cap0, cols), dtype=F32, device=r.mk0.device)
    check(lib().einx_compact_rows(_ptr(r.mk0), _ptr(r.mk1), _ptr(r.nmatch), B, cap0, cols, _ptr(r.mk0_flat), _ptr(r.mk1_flat),
                                  _stream(r.mk0)), "einx_compact_rows")
    return r


LG_ATTN_F16, LG_LIN_F16 = 1, 2  # the mode bits of einx_lightglue_mp (einx.h: EINX_LG_ATTN_F16, EINX_LG_LIN_F16)


def lightglue(weights, pb0, pb1, want_la=True, want_ref=False, all_layers=False, early_stop=None, pruning=None, flash=False, mp=False):
    """weights: _lib.LgWeights; pb0/pb1: PairBatch (kpts [B,cap,3], desc [B,cap,Din], counts).
    all_layers: ref0/ref1 are [B,n_layers,cap,d] (training-mode ref_descriptors) instead of [B,cap,d].
    early_stop = (heads, depth_confidence): einx_lightglue_early_stop with the _lib.LgHead array of every layer's heads; r.stop
    [B] int32 is the number of layers each pair ran.
    pruning = (heads, width_confidence, min_kpts): einx_lightglue_adaptive, with `early_stop` or without; r.prune0/1,
    r.kept0/1 and r.live are set, r.la is None whatever want_la says, ref0 / ref1 hold the survivors' rows (zeros behind them).
    flash: the same run through einx_lightglue_flash, every attention in fp16 on the matrix cores.
    mp: the same run through einx_lightglue_mp, the layers' linears in fp16 on the matrix cores, with `flash` or
    without; `weights` must then be the unfolded pack with the binary16 images (LightGlue._pack(mp=True))."""
    _dev_check(pb0.kpts, pb0.desc, pb1.kpts, pb1.desc)
    _dev_check(pb0.counts, pb1.counts, dt=I32)
    B, cap0, cap1 = pb0.B, pb0.cap, pb1.cap
    L = lib()
    dev = pb0.desc.device
    d = int(weights.d)
    if pruning is not None:
        if all_layers:
            raise ValueError("einx LightGlue: point pruning returns the surviving rows the head read, not every layer's")
        if not 0.0 < float(pruning[1]) <= 1.0:
            raise ValueError("einx LightGlue: point pruning takes a width_confidence in (0, 1]")
        want_la = False  # not produced
        nbytes = L.einx_lightglue_adaptive_ws_bytes(B, cap0, cap1, d, int(weights.heads), int(weights.input_dim), int(weights.n_layers))
    elif early_stop is not None:
        if all_layers:
            raise ValueError("einx LightGlue: early stopping returns the descriptors the stopping head read, not every layer's")
        nbytes = L.einx_lightglue_early_stop_ws_bytes(B, cap0, cap1, d, int(weights.heads), int(weights.input_dim), int(weights.n_layers))
    else:
        nbytes = L.einx_lg_ws_bytes_heads(B, cap0, cap1, d, int(weights.heads), int(weights.input_dim))
    if not nbytes:
        raise NotImplementedError("einx LightGlue: descriptor_dim must be num_heads x head_dim with head_dim a multiple of 4, at most 256")
    if mp:
        nbytes = L.einx_lightglue_mp_ws_bytes(B, cap0, cap1, d, int(weights.heads), int(weights.input_dim), int(weights.n_layers))
    elif flash:
        nbytes = L.einx_lightglue_flash_ws_bytes(B, cap0, cap1, d, int(weights.heads), int(weights.input_dim), int(weights.n_layers))
    ws = _workspace(nbytes, dev)
    r = MatchResult()
    r.matches0 = torch.empty((B, cap0), dtype=torch.int64, device=dev)
    r.matches1 = torch.empty((B, cap1), dtype=torch.int64, device=dev)
    r.scores0 = torch.empty((B, cap0), dtype=F32, device=dev)
    r.scores1 = torch.empty((B, cap1), dtype=F32, device=dev)
    r.la = torch.empty((B, cap0 + 1, cap1 + 1), dtype=F32, device=dev) if want_la else None
    nl = int(weights.n_layers)
    if want_ref and all_layers:
        r.ref0 = torch.zeros((B, nl, cap0, d), dtype=F32, device=dev)
        r.ref1 = torch.zeros((B, nl, cap1, d), dtype=F32, device=dev)
    else:
        r.ref0 = torch.empty((B, cap0, d), dtype=F32, device=dev) if want_ref else None
        r.ref1 = torch.empty((B, cap1, d), dtype=F32, device=dev) if want_ref else None
    (h0, w0), (h1, w1) = pb0.image_size, pb1.image_size
    ref_layers = nl if (want_ref and all_layers) else 1

    def flash_call(heads, depth, width, min_kpts):
        """einx_lightglue_flash, or with `mp` einx_lightglue_mp: one argument list, the mode bits before the stream"""
        args = (ctypes.byref(weights), heads, ctypes.sizeof(_lib.LgHead), float(depth), float(width), int(min_kpts),
                _ptr(pb0.kpts), _ptr(pb0.desc), _ptr(pb0.counts), cap0, _ptr(pb1.kpts), _ptr(pb1.desc), _ptr(pb1.counts),
                cap1, B, float(h0), float(w0), float(h1), float(w1), _ptr(ws), _ptr(r.matches0), _ptr(r.matches1),
                _ptr(r.scores0), _ptr(r.scores1), _ptr(r.la), _ptr(r.ref0), _ptr(r.ref1), ref_layers, _ptr(r.stop),
                _ptr(r.prune0), _ptr(r.prune1), _ptr(r.kept0), _ptr(r.kept1), _ptr(r.live))
        if mp:
            check(L.einx_lightglue_mp(*args, LG_LIN_F16 | (LG_ATTN_F16 if flash else 0), _stream(pb0.desc)), "einx_lightglue_mp")
        else:
            check(L.einx_lightglue_flash(*args, _stream(pb0.desc)), "einx_lightglue_flash")
        return r

    if pruning is not None:
        heads, width, min_kpts = pruning
        depth = float(early_stop[1]) if early_stop is not None else -1.0
        if early_stop is not None:
            r.stop = torch.empty((B,), dtype=torch.int32, device=dev)
        if want_ref:  # rows past the live count are zero
            r.ref0.zero_()
            r.ref1.zero_()
        r.prune0 = torch.empty((B, cap0), dtype=F32, device=dev)
        r.prune1 = torch.empty((B, cap1), dtype=F32, device=dev)
        r.kept0 = torch.empty((B, cap0), dtype=I64, device=dev)
        r.kept1 = torch.empty((B, cap1), dtype=I64, device=dev)
        r.live = torch.empty((2 * B,), dtype=I32, device=dev)
        if flash or mp:
            return flash_call(heads, depth, width, min_kpts)
        check(L.einx_lightglue_adaptive(ctypes.byref(weights), heads, ctypes.sizeof(heads._type_), depth, float(width), int(min_kpts),
                                        _ptr(pb0.kpts), _ptr(pb0.desc), _ptr(pb0.counts), cap0, _ptr(pb1.kpts), _ptr(pb1.desc), _ptr(pb1.counts),
                                        cap1, B, float(h0), float(w0), float(h1), float(w1), _ptr(ws), _ptr(r.matches0), _ptr(r.matches1),
                                        _ptr(r.scores0), _ptr(r.scores1), None, _ptr(r.ref0), _ptr(r.ref1), _ptr(r.stop), _ptr(r.prune0),
                                        _ptr(r.prune1), _ptr(r.kept0), _ptr(r.kept1), _ptr(r.live), _stream(pb0.desc)),
              "einx_lightglue_adaptive")
        return r
    if early_stop is not None:
        heads, depth = early_stop
        r.stop = torch.empty((B,), dtype=torch.int32, device=dev)
        if flash or mp:
            return flash_call(heads, depth, -1.0, 0)
        check(L.einx_lightglue_early_stop(ctypes.byref(weights), heads, ctypes.sizeof(heads._type_), float(depth), _ptr(pb0.kpts), _ptr(pb0.desc),
                                          _ptr(pb0.counts), cap0, _ptr(pb1.kpts), _ptr(pb1.desc), _ptr(pb1.counts), cap1, B, float(h0), float(w0),
                                          float(h1), float(w1), _ptr(ws), _ptr(r.matches0), _ptr(r.matches1), _ptr(r.scores0), _ptr(r.scores1),
                                          _ptr(r.la), _ptr(r.ref0), _ptr(r.ref1), _ptr(r.stop), _stream(pb0.desc)),
              "einx_lightglue_early_stop")
        return r
    if flash or mp:
        return flash_call(None, -1.0, -1.0, 0)
    check(L.einx_lightglue(ctypes.byref(weights), _ptr(pb0.kpts), _ptr(pb0.desc), _ptr(pb0.counts), cap0, _ptr(pb1.kpts), _ptr(pb1.desc),
                           _ptr(pb1.counts), cap1, B, float(h0), float(w0), float(h1), float(w1), _ptr(ws), _ptr(r.matches0),
                           _ptr(r.matches1), _ptr(r.scores0), _ptr(r.scores1), _ptr(r.la), _ptr(r.ref0), _ptr(r.ref1),
                           nl if (want_ref and all_layers) else 1, _stream(pb0.desc)),
          "einx_lightglue")
    return r


LG_NLL_COLUMNS = ("S_pos", "num_pos", "S_neg0", "num_neg0", "S_neg1", "num_neg1", "row_sum", "n")


def lg_assign_nll(head, x0, x1, gt_matches0, gt_matches1, pos0=None, assignment=None, n=None, m=None):
    """einx_lg_assign_nll: the sums behind LightGlue's assignment NLL and row_norm for ONE MatchAssignment head, [B,8] float64 =
    LG_NLL_COLUMNS per pair, no host synchronisation.  head: (proj_w [d,d], proj_b [d], match_w [1,d], match_b [1])
    fp32 tensors, or an _lib.LgWeights (its last head's pointers).  x0 [B,cap0,d] / x1 [B,cap1,d]: plain tensors, or a MatchResult
    as x0 (its ref0 / ref1, x1 ignored).  gt_matches0 / 1 int64 [B,cap].  The positives: pos0 int32 [B,cap0] (-1 = none) or a
    dense bool / uint8 `assignment` [B,cap0,cap1] (any strides).  n / m: int32 [B] counts or None (= cap)."""
    if isinstance(x0, MatchResult):
        x0, x1 = x0.ref0, x0.ref1
    if (pos0 is None) == (assignment is None):
        raise ValueError("einx: lg_assign_nll takes the positives as pos0= or as assignment=, one of the two")
    _dev_check(x0, x1)
    B, cap0, d = x0.shape
    cap1 = x1.shape[1]
    dev = x0.device
    if x1.shape[0] != B or x1.shape[2] != d:
        raise ValueError("einx: x0 and x1 differ in batch size or width")
    if isinstance(head, _lib.LgWeights):
        if int(head.d) != d:
            raise ValueError("einx: descriptors and head differ in width")
        hp = (head.proj_w, head.proj_b, head.match_w, head.match_b)
    else:
        _dev_check(*head)
        if tuple(head[0].shape) != (d, d) or head[1].numel() != d or head[2].numel() != d or head[3].numel() != 1:
            raise ValueError("einx: head weights do not fit descriptors of width %d" % d)
        hp = tuple(_ptr(t) for t in head)
    gt0, gt1 = gt_matches0.to(dev, I64).contiguous(), gt_matches1.to(dev, I64).contiguous()
    if tuple(gt0.shape) != (B, cap0) or tuple(gt1.shape) != (B, cap1):
        raise ValueError("einx: gt_matches0 / gt_matches1 must be [B,cap0] / [B,cap1]")
    strides = (0, 0, 0)
    if pos0 is not None:
        _dev_check(pos0, dt=I32)
        if tuple(pos0.shape) != (B, cap0):
            raise ValueError("einx: pos0 must be [B,cap0]")
    else:
        if assignment.dtype == torch.bool:
            assignment = assignment.view(U8)
        if assignment.dtype != U8 or assignment.device != dev or tuple(assignment.shape) != (B, cap0, cap1):
            raise ValueError("einx: assignment must be a bool / uint8 [B,cap0,cap1] tensor on the descriptors' device")
        strides = tuple(int(v) for v in assignment.stride())
    for c in (n, m):
        _dev_check(c, dt=I32)
    n = torch.full((B,), cap0, dtype=I32, device=dev) if n is None else n
    m = torch.full((B,), cap1, dtype=I32, device=dev) if m is None else m
    L = lib()
    nbytes = L.einx_lg_assign_nll_ws_bytes(B, cap0, cap1, d)
    if not nbytes:
        raise NotImplementedError("einx: lg_assign_nll needs B, cap0, cap1 > 0 and a descriptor width that is a multiple of 4")
    ws = _workspace(nbytes, dev)
    out = torch.empty((B, len(LG_NLL_COLUMNS)), dtype=torch.float64, device=dev)
    check(L.einx_lg_assign_nll(*hp, d, _ptr(x0), _ptr(n), cap0, _ptr(x1), _ptr(m), cap1, B, _ptr(gt0), _ptr(gt1), _ptr(pos0), _ptr(assignment),
                               *strides, _ptr(ws), _ptr(out), _stream(x0)), "einx_lg_assign_nll")
    return out


def lg_nll_values(rows, balancing=0.5):
    """[B,8] rows of lg_assign_nll -> [B,5] float64 = nll, nll_pos, nll_neg, num_matchable, num_unmatchable, and row_norm [B]
    (NaN in every column for a pair without keypoints on a side, whose row holds n = 0).  Device arithmetic only."""
    s_pos, n_pos, s_n0, n_n0, s_n1, n_n1, rs, n = rows.unbind(1)
    num_pos = n_pos.clamp_min(1.0)
    den = n_n0.clamp_min(1.0) + n_n1.clamp_min(1.0)
    nll_pos = -s_pos / num_pos
    nll_neg = -(s_n0 + s_n1) / den
    nll = balancing * nll_pos + (1 - balancing) * nll_neg
    vals = torch.stack([nll, nll_pos, nll_neg, num_pos, den / 2.0, rs / n], 1)  # n == 0: 0 / 0 = NaN in row_norm
    vals = torch.where((n > 0).unsqueeze(1), vals, vals.new_tensor(float("nan")))
    return vals[:, :5], vals[:, 5]


def similarity(desc0, n, desc1, m):
    """[B,cap0,cap1] descriptor similarity (MNN.py:88); zero outside the first n[b] x m[b] block."""
    _dev_check(desc0, desc1)
    _dev_check(n, m, dt=I32)
    B, cap0, D = desc0.shape
    cap1 = desc1.shape[1]
    sim = torch.empty((B, cap0, cap1), dtype=F32, device=desc0.device)
    check(lib().einx_similarity(_ptr(desc0), _ptr(n), cap0, _ptr(desc1), _ptr(m), cap1, B, D, _ptr(sim), _stream(desc0)), "einx_similarity")
    return sim


def normalize_rows(x, scale):
    """F.normalize(x, dim=1) * scale for a [R,C] matrix."""
    _dev_check(x)
    R, C = x.shape
    out = torch.empty_like(x)
    if R:
        check(lib().einx_normalize_rows(_ptr(x), R, C, float(scale), _ptr(out), _stream(x)), "einx_normalize_rows")
    return out


def normalize_keypoints(kpts, size, out_cols=2):
    """lightglue.py:137-148 on [..., cols>=2] keypoints -> [..., out_cols] (zeros beyond column 1)."""
    _dev_check(kpts)
    cols = kpts.shape[-1]
    rows = kpts.numel() // cols
    out = torch.empty(tuple(kpts.shape[:-1]) + (out_cols,), dtype=F32, device=kpts.device)
    if rows:
        check(lib().einx_normalize_keypoints(_ptr(kpts), rows, cols, float(size[0]), float(size[1]), _ptr(out), out_cols, _stream(kpts)),
              "einx_normalize_keypoints")
    return out


def random_positions(u, size):
    """u [R,2] uniform draws -> [R,3] = (u0*size0, u1*size1, 0)  (Matchers.py:80-91)."""
    _dev_check(u)
    R = u.shape[0]
    out = torch.empty((R, 3), dtype=F32, device=u.device)
    if R:
        check(lib().einx_random_positions(_ptr(u), R, float(size[0]), float(size[1]), _ptr(out), _stream(u)), "einx_random_positions")
    return out


def linear(x, w, bias, out=None, accumulate=False):
    """y = x @ w.T + bias on the fp32 matrix cores (einx_linear); accumulate: y += ..."""
    _dev_check(x, w, bias, out)
    M, K = x.shape
    Nn = w.shape[0]
    y = out if out is not None else torch.empty((M, Nn), dtype=F32, device=x.device)
    check(lib().einx_linear(_ptr(x), M, K, _ptr(w), _ptr(bias), Nn, _ptr(y), int(accumulate), _stream(x)), "einx_linear")
    return y


WATCH_CHUNK_WORDS = 4096  # include/einx.h: EINX_WATCH_CHUNK_WORDS


class ParamWatch:
    """Device-side content watch of a module's fp32 parameters / buffers (einx_params_hash): `.data` edits, which no host-side
    version counter sees, raise `stale` at the next forward.  Exact since round 5: EVERY word is hashed (round 4 sampled 65 per
    tensor), tensors cut into rows of 4096 words, one wave per row -- 1.3 M extractor weights are 380 rows riding on spare
    workgroups of the descriptor sampling kernel, LightGlue's 12 M one 10 us launch.  Built when the module packs its weights;
    `check()` enqueues one small launch on the current stream; the flag travels to the host with the counts the forward reads
    back anyway."""

    def __init__(self, tensors):
        ts = [t.detach() for t in tensors if torch.is_tensor(t) and t.dtype == F32 and t.numel() > 0 and t.device.type == "cuda"
              and t.is_contiguous()]
        if os.environ.get("EINX_NO_WATCH") == "1":  # tools: A/B of the watch's cost
            ts = []
        self.keep = ts
        self.stale = None
        rows = [[t.data_ptr() + 4 * off, min(WATCH_CHUNK_WORDS, t.numel() - off)] for t in ts for off in range(0, t.numel(), WATCH_CHUNK_WORDS)]
        self.n = len(rows)
        if not rows:
            return
        dev = ts[0].device
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.ref = torch.empty((self.n,), dtype=torch.int64, device=dev)
        self.scratch = torch.empty((self.n,), dtype=torch.int64, device=dev)
        self.stale = torch.zeros((1,), dtype=torch.int32, device=dev)
        check(lib().einx_params_hash(_ptr(self.table), self.n, _ptr(self.ref), None, None, _stream(self.table)), "einx_params_hash")

    def check(self):
        """enqueue the comparison on the current stream; returns the device flag (int32 [1], 1 = some tensor changed)"""
        if self.n:
            check(lib().einx_params_hash(_ptr(self.table), self.n, _ptr(self.scratch), _ptr(self.ref), _ptr(self.stale), _stream(self.table)),
                  "einx_params_hash")
        return self.stale


# ------------------------------------------------------------------------------ losses (forward values; csrc/loss.hip)
DESC_LOSS_MODES = {"mae": 0, "mse": 1, "cos": 2}
MAP_LOSS_MODES = {"sq": 0, "abs": 1, "bce": 2, "cos": 3}


def _loss_mask(mask, numel):
    """-> (the tensor the kernel reads, or None; its einx.h mask type).  bool / uint8: non-zero is 1; anything else: float32 weights."""
    if mask is None:
        return None, 0
    if mask.device.type != "cuda":
        raise RuntimeError(f"einx: the mask must live on a HIP device, got {mask.device}")
    if mask.numel() != numel:
        raise ValueError(f"einx: mask of {mask.numel()} elements where {numel} are expected")
    if mask.dtype == torch.bool:
        return mask.contiguous().view(U8), 1
    if mask.dtype == U8:
        return mask.contiguous(), 1
    return mask.to(F32).contiguous(), 2


def desc_loss(raw_a, scale_a, raw_b, scale_b, padded_size, pads, cell, mask=None, mode="mae"):
    """(sum, count) per image [B,2] float64 of DescriptorsLoss over the `normalized_descriptors` of two raw maps [B,D,hc,wc]
    without building the dense maps (einx_desc_loss).  mask: [B,H,W] (any shape with B*H*W elements) or None."""
    _dev_check(raw_a, raw_b)
    if raw_a.shape != raw_b.shape:
        raise ValueError(f"einx: raw maps of different shapes {tuple(raw_a.shape)} / {tuple(raw_b.shape)}")
    B, D, hc, wc = raw_a.shape
    Hp, Wp = int(padded_size[0]), int(padded_size[1])
    w0, w1, h0, h1 = pads
    H, W = Hp - h0 - h1, Wp - w0 - w1
    m, mt = _loss_mask(mask, B * H * W)
    out = torch.empty((B, 2), dtype=torch.float64, device=raw_a.device)
    L = lib()
    nws = int(L.einx_desc_loss_ws_bytes(B, D, hc, wc, Hp, Wp, h0, w0, H, W, int(cell)))
    ws = _workspace(nws, raw_a.device)
    check(L.einx_desc_loss(_ptr(raw_a), float(scale_a), _ptr(raw_b), float(scale_b), B, D, hc, wc, Hp, Wp, h0, w0, H, W, int(cell), _ptr(m), mt,
                           DESC_LOSS_MODES[mode], _ptr(out), _ptr(ws), nws, _stream(raw_a)), "einx_desc_loss")
    return out


def map_loss(x, y, mask=None, mode="sq"):
    """(sum, count) per image [B,2] float64 of a masked pair reduction over two float32 tensors [B,C,...] (einx_map_loss).
    mask: B*P elements (broadcast over the channels) or B*C*P (one weight per element), or None."""
    _dev_check(x, y)
    if x.shape != y.shape:
        raise ValueError(f"einx: tensors of different shapes {tuple(x.shape)} / {tuple(y.shape)}")
    B, C = int(x.shape[0]), (int(x.shape[1]) if x.dim() > 2 else 1)
    P = int(x.numel() // (B * C))
    full = mask is not None and C > 1 and mask.numel() == B * C * P
    m, mt = _loss_mask(mask, B * C * P if full else B * P)
    out = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    L = lib()
    nws = int(L.einx_map_loss_ws_bytes(B, P))
    ws = _workspace(nws, x.device)
    check(L.einx_map_loss(_ptr(x), _ptr(y), B, C, P, _ptr(m), mt, int(full), MAP_LOSS_MODES[mode], _ptr(out), _ptr(ws), nws, _stream(x)),
          "einx_map_loss")
    return out


def logits_loss(x, y, cell, crop=None, mask=None):
    """(sum, count) per image [B,2] float64 of LogitsLoss over [B,cell^2+1,hc,wc] logits (einx_logits_loss).
    crop: (h0, w0, H, W) of the un-padded window in the pixel-shuffled map, None: the whole map; mask: B*H*W elements or None."""
    _dev_check(x, y)
    if x.shape != y.shape:
        raise ValueError(f"einx: tensors of different shapes {tuple(x.shape)} / {tuple(y.shape)}")
    B, C, hc, wc = x.shape
    h0, w0, H, W = (0, 0, cell * hc, cell * wc) if crop is None else (int(v) for v in crop)
    m, mt = _loss_mask(mask, B * H * W)
    out = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    L = lib()
    nws = int(L.einx_map_loss_ws_bytes(B, hc * wc))
    ws = _workspace(nws, x.device)
    check(L.einx_logits_loss(_ptr(x), _ptr(y), B, C, int(cell), hc, wc, h0, w0, H, W, _ptr(m), mt, _ptr(out), _ptr(ws), nws, _stream(x)),
          "einx_logits_loss")
    return out


def _f64(values, n, what):
    """n host doubles for the map builders' K / D / R / P arguments"""
    a = np.ascontiguousarray(np.asarray(values, np.float64).reshape(-1))
    if a.size != n:
        raise ValueError(f"einx: {what} must hold {n} values, got {a.size}")
    return a


def rectify_map(model, K, D, R, P, H, W, device, iters=5, round_out=False):
    """(map_x, map_y) [H,W] fp32 of einx_rectify_map_fisheye / _radtan / einx_undistort_points_map_radtan (model: "fisheye", "radtan",
    "points"); K: 4 values, D: 4 (fisheye) or 5, R / P: 9 row-major each (R unused for "points")"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"einx: maps are built on a HIP device (torch device type 'cuda'); there is no CPU path. Got {device}.")
    k, d, p = _f64(K, 4, "K"), _f64(D, 4 if model == "fisheye" else 5, "D"), _f64(P, 9, "P")
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    mx, my = (torch.empty((H, W), dtype=F32, device=device) for _ in range(2))
    L = lib()
    with torch.cuda.device(device):
        if model == "points":
            check(L.einx_undistort_points_map_radtan(hp(k), hp(d), hp(p), H, W, int(iters), int(bool(round_out)), _ptr(mx), _ptr(my), _stream(mx)),
                  "einx_undistort_points_map_radtan")
        else:
            r = _f64(R, 9, "R")
            name = f"einx_rectify_map_{model}"
            check(getattr(L, name)(hp(k), hp(d), hp(r), hp(p), H, W, _ptr(mx), _ptr(my), _stream(mx)), name)
    return mx, my


def remap_bilinear(src, map_x, map_y):
    """src [F,Hs,Ws] uint8 or fp32 -> [F,H,W] of the same type, sampled bilinearly at the maps [H,W] (einx_remap_bilinear)"""
    _dev_check(src, dt=src.dtype)
    _dev_check(map_x, map_y)
    F_, Hs, Ws = (int(v) for v in src.shape)
    H, W = (int(v) for v in map_x.shape)
    dst = torch.empty((F_, H, W), dtype=src.dtype, device=src.device)
    if F_ == 0:
        return dst
    with torch.cuda.device(src.device):
        check(lib().einx_remap_bilinear(_ptr(src), 0 if src.dtype == U8 else 1, F_, Hs, Ws, _ptr(map_x), _ptr(map_y), H, W, _ptr(dst), _stream(src)),
              "einx_remap_bilinear")
    return dst


WARP_MODES = {"bilinear": 0, "nearest": 1}  # einx.h: EINX_WARP_BILINEAR, EINX_WARP_NEAREST


def warp_perspective(src, Hinv, Hd, Wd, mode="bilinear", want_valid=True):
    """src [B,C,Hs,Ws] uint8 or fp32, Hinv [B,9] float64 (destination -> source) -> (dst [B,C,Hd,Wd] of src's type, valid uint8
    [B,Hd,Wd] or None): einx_warp_perspective (csrc/warp.hip)"""
    _dev_check(src, dt=src.dtype)
    _dev_check(Hinv, dt=torch.float64)
    if src.dtype not in (U8, F32):
        raise TypeError(f"einx: warp_perspective takes uint8 or float32, got {src.dtype}")
    B, C, Hs, Ws = (int(v) for v in src.shape)
    if tuple(Hinv.shape) != (B, 9):
        raise ValueError(f"einx: Hinv must be [{B}, 9], got {tuple(Hinv.shape)}")
    dst = torch.empty((B, C, Hd, Wd), dtype=src.dtype, device=src.device)
    valid = torch.empty((B, Hd, Wd), dtype=U8, device=src.device) if want_valid else None
    with torch.cuda.device(src.device):
        check(lib().einx_warp_perspective(_ptr(src), 0 if src.dtype == U8 else 1, B, C, Hs, Ws, _ptr(Hinv), int(Hd), int(Wd), WARP_MODES[mode],
                                          _ptr(dst), _ptr(valid), _stream(src)), "einx_warp_perspective")
    return dst, valid


def events_remap(x, y, t, p, map_x, map_y, x_hi, y_hi, out=None):
    """einx_events_remap on a resident stream: (out_x, out_y, out_t, out_p, head) with the outputs sized like the inputs and
    head an int64 [2 + N] tensor whose first two words are (kept, out of map) and whose rest IS out_t's storage, so that one copy
    brings the counts and the stamps to the host.  out: the same tuple from an earlier call, to write into (graph capture)."""
    _dev_check(x, y, p, map_x, map_y)
    _dev_check(t, dt=torch.float64)
    n = int(t.numel())
    H, W = (int(v) for v in map_x.shape)
    if out is None:
        head = torch.empty(2 + n, dtype=I64, device=t.device)
        out = (torch.empty(n, dtype=F32, device=t.device), torch.empty(n, dtype=F32, device=t.device), head[2:].view(torch.float64),
               torch.empty(n, dtype=F32, device=t.device), head)
    ox, oy, ot, op, head = out
    L = lib()
    nws = int(L.einx_events_remap_ws_bytes(n))
    ws = _workspace(nws, t.device)
    with torch.cuda.device(t.device):
        check(L.einx_events_remap(_ptr(x), _ptr(y), _ptr(t), _ptr(p), n, _ptr(map_x), _ptr(map_y), H, W, float(x_hi), float(y_hi), _ptr(ox), _ptr(oy),
                                  _ptr(ot), _ptr(op), _ptr(head), _ptr(ws), nws, _stream(t)), "einx_events_remap")
    return out


# ------------------------------------------------------------------------------ pose tracks (csrc/posetrack.hip)
F64 = torch.float64


def _track_check(stamps, trans, quats):
    _dev_check(stamps, trans, quats, dt=F64)
    n = int(stamps.numel())
    if stamps.dim() != 1 or tuple(trans.shape) != (n, 3) or tuple(quats.shape) != (n, 4):
        raise ValueError(f"einx: a track is stamps [N], translations [N,3] and quaternions [N,4], got {tuple(stamps.shape)}, "
                         f"{tuple(trans.shape)}, {tuple(quats.shape)}")
    return n


def pose_interp(stamps, trans, quats, queries, inverse=True, dtype=F32):
    """einx_pose_interp: queries [Q] float64 on the track's device -> (poses [Q,4,4] of `dtype` (float32 or float64), out_of_range
    int32 [1] on the device); no host synchronisation"""
    n = _track_check(stamps, trans, quats)
    _dev_check(queries, dt=F64)
    if dtype not in (F32, F64):
        raise TypeError(f"einx: poses are float32 or float64, got {dtype}")
    q = int(queries.numel())
    out = torch.empty((q, 4, 4), dtype=dtype, device=stamps.device)
    bad = torch.empty(1, dtype=I32, device=stamps.device)
    with torch.cuda.device(stamps.device):
        check(lib().einx_pose_interp(_ptr(stamps), _ptr(trans), _ptr(quats), n, _ptr(queries), q, int(bool(inverse)), 0 if dtype == F32 else 1,
                                     _ptr(out), _ptr(bad), _stream(stamps)), "einx_pose_interp")
    return out, bad


def pose_relative(stamps, trans, quats, q0, q1):
    """einx_pose_relative: q0, q1 [P] float64 -> (T_0to1, T_1to0 [P,4,4] float32, out_of_range int32 [1]); no host synchronisation"""
    n = _track_check(stamps, trans, quats)
    _dev_check(q0, q1, dt=F64)
    p = int(q0.numel())
    if int(q1.numel()) != p:
        raise ValueError(f"einx: pose_relative takes two query arrays of one length, got {p} and {int(q1.numel())}")
    t01, t10 = (torch.empty((p, 4, 4), dtype=F32, device=stamps.device) for _ in range(2))
    bad = torch.empty(1, dtype=I32, device=stamps.device)
    with torch.cuda.device(stamps.device):
        check(lib().einx_pose_relative(_ptr(stamps), _ptr(trans), _ptr(quats), n, _ptr(q0), _ptr(q1), p, _ptr(t01), _ptr(t10), _ptr(bad),
                                       _stream(stamps)), "einx_pose_relative")
    return t01, t10, bad


def nearest_stamp(stamps, queries):
    """einx_nearest_stamp: sorted stamps [F] and queries [Q], float64 on one device -> int64 [Q]"""
    _dev_check(stamps, queries, dt=F64)
    f, q = int(stamps.numel()), int(queries.numel())
    if f == 0:
        raise ValueError("einx: nearest_stamp: no stamps")
    out = torch.empty(q, dtype=I64, device=stamps.device)
    with torch.cuda.device(stamps.device):
        check(lib().einx_nearest_stamp(_ptr(stamps), f, _ptr(queries), q, _ptr(out), _stream(stamps)), "einx_nearest_stamp")
    return out
