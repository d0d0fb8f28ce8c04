"""float64 restatement of the extractor losses (numpy), written from the contract of DESIGN.md 8f, plus the input recipes that the
fixture generator (tests/golden/gen_losses.py) and the tests share, so that the fixture stores outputs only.

Terms are formed as torch forms them on float32 tensors -- the difference and its square each rounded to float32 -- and then
summed in float64; BCE's logarithms and the cosine are evaluated in float64 from the float32 inputs.  Every function returns
(sums [B], counts [B]) in float64: a loss value is weight * sum(sums) / sum(counts), a per-pair value weight * sums / counts.
Not collected by pytest (no test_ prefix)."""
import numpy as np

from helpers import synth


# ------------------------------------------------------------------------------------------ (sum, count) per image
def _weights(mask, shape):
    """mask (bool / uint8: non-zero is 1; float: weights) broadcast to `shape` as float64; None: ones"""
    if mask is None:
        return np.ones(shape, np.float64)
    m = np.asarray(mask)
    w = (m != 0).astype(np.float64) if m.dtype in (np.bool_, np.uint8) else m.astype(np.float64)
    if w.size == int(np.prod(shape)):
        return w.reshape(shape)
    return np.broadcast_to(w.reshape((shape[0], 1) + tuple(shape[2:])), shape)


def terms(x, y, mode):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    if mode == "sq":
        d = (x - y).astype(np.float32)
        return (d * d).astype(np.float32).astype(np.float64)
    if mode == "abs":
        return np.abs((x - y).astype(np.float32)).astype(np.float64)
    if mode == "bce":
        p, t = x.astype(np.float64), (y > 0).astype(np.float64)
        with np.errstate(divide="ignore"):
            lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log(1.0 - p), -100.0)
        return -(t * lp + (1.0 - t) * lq)
    raise ValueError(mode)


def map_sums(x, y, mask, mode):
    """x, y [B,C,...]; mask with B*P elements (broadcast over C) or B*C*P, or None"""
    B = x.shape[0]
    t = terms(x, y, mode)
    w = _weights(mask, t.shape)
    return (t * w).reshape(B, -1).sum(1), w.reshape(B, -1).sum(1)


def cos_sums(x, y, mask):
    """cosine over dim 1 per position, eps 1e-8 on each norm; mask with B*P elements or None"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    B = x.shape[0]
    cos = (x * y).sum(1) / (np.maximum(np.sqrt((x * x).sum(1)), 1e-8) * np.maximum(np.sqrt((y * y).sum(1)), 1e-8))
    w = _weights(mask, (B, 1) + cos.shape[1:]).reshape(cos.shape)
    return (cos * w).reshape(B, -1).sum(1), w.reshape(B, -1).sum(1)


def pixel_shuffle(x, r):
    B, C, h, w = x.shape
    c = C // (r * r)
    return x.reshape(B, c, r, r, h, w).transpose(0, 1, 4, 2, 5, 3).reshape(B, c, h * r, w * r)


def logits_sums(x, y, cell, pads, mask):
    """channels 0 .. cell^2 - 1 pixel-shuffled, cropped by pads (w0, w1, h0, h1) (None: no crop), squared differences weighted by
    the mask [B,H,W]; count = every element of the window"""
    B = x.shape[0]
    xs, ys = pixel_shuffle(x[:, :cell * cell], cell), pixel_shuffle(y[:, :cell * cell], cell)
    if pads is not None:
        w0, w1, h0, h1 = pads
        Hp, Wp = xs.shape[-2:]
        xs, ys = xs[..., h0:Hp - h1, w0:Wp - w1], ys[..., h0:Hp - h1, w0:Wp - w1]
    t = terms(xs, ys, "sq")
    w = _weights(mask, t.shape)
    return (t * w).reshape(B, -1).sum(1), np.full(B, float(t[0].size))


def value(sums, counts, weight=1.0):
    with np.errstate(invalid="ignore", divide="ignore"):
        return weight * (np.sum(sums) / np.sum(counts))


def pair_values(sums, counts, weight=1.0):
    with np.errstate(invalid="ignore", divide="ignore"):
        return weight * (sums / counts)


# ------------------------------------------------------------------------------------------ the modules' contract
def score_loss(pred, gt, mask, mode, use_mask=True):
    """-> (sums, counts, gt after the call): mse-whole zeroes gt where the mask is true"""
    if not use_mask:
        mask = None
    if mode == "bce":
        return map_sums(pred, gt, None, "bce") + (gt,)
    if mode == "mse-whole":
        if mask is not None:
            gt = np.where(np.asarray(mask).reshape(gt.shape) != 0, np.float32(0.0), gt)
        return map_sums(pred, gt, None, "sq") + (gt,)
    return map_sums(pred, gt, mask, {"mse": "sq", "mae": "abs"}[mode]) + (gt,)


def descriptors_loss(pred, gt, mask, mode, use_mask=True):
    """-> (sums, counts, transform of sum / count): cosine_similarity returns 1 - mean"""
    if not use_mask:
        mask = None
    if mode == "cosine_similarity":
        return cos_sums(pred, gt, mask) + (lambda v: 1.0 - v,)
    return map_sums(pred, gt, mask, {"mse": "sq", "mae": "abs"}[mode]) + (lambda v: v,)


# ------------------------------------------------------------------------------------------ input recipes of the fixture
B, C, H, W = 2, 16, 20, 29       # un-padded size; padded to 24 x 32 (pads w 1 | 2, h 2 | 2), coarse 3 x 4
PADS = (1, 2, 2, 2)              # Padder((20, 29), 8).padding_size = (w0, w1, h0, h1)
CELL = 8


def unit_map(seed, shape, scale=1.0):
    x = synth.uniform(seed, shape, -1.0, 1.0)
    n = np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True))
    return (scale * x / n).astype(np.float32)


def inputs():
    d = {}
    d["desc_pred"], d["desc_gt"] = unit_map(101, (B, C, H, W)), unit_map(102, (B, C, H, W))
    d["score_pred"] = synth.uniform(103, (B, 1, H, W), 0.001, 0.999)
    s = synth.uniform01(104, (B, 1, H, W))
    d["score_gt"] = np.where(synth.uniform01(105, (B, 1, H, W)) > 0.85, s, np.float32(0.0)).astype(np.float32)
    d["logits_pred"] = synth.uniform(106, (B, CELL * CELL + 1, 3, 4), -4.0, 4.0)
    d["logits_gt"] = synth.uniform(107, (B, CELL * CELL + 1, 3, 4), -4.0, 4.0)
    d["feat_pred"], d["feat_gt"] = synth.uniform(108, (B, 8, 3, 4), 0.0, 2.0), synth.uniform(109, (B, 8, 3, 4), 0.0, 2.0)
    d["mask"] = synth.uniform01(110, (B, 1, H, W)) > 0.4
    d["mask_empty"] = np.zeros((B, 1, H, W), bool)
    return d


# name -> (loss class, constructor arguments, input keys (pred, gt), mask key or None, padder?)
VALUE_CASES = {
    "desc_mse_mask": ("DescriptorsLoss", dict(weight=2.0, mode="mse"), "desc", "mask", False),
    "desc_mae_mask": ("DescriptorsLoss", dict(weight=1.0, mode="mae"), "desc", "mask", False),
    "desc_mse_empty": ("DescriptorsLoss", dict(weight=1.0, mode="mse"), "desc", "mask_empty", False),
    "desc_mae_empty": ("DescriptorsLoss", dict(weight=1.0, mode="mae"), "desc", "mask_empty", False),
    "desc_mae_nomask": ("DescriptorsLoss", dict(weight=0.5, mode="mae"), "desc", None, False),
    "desc_mae_unused_mask": ("DescriptorsLoss", dict(weight=1.0, mode="mae", use_mask=False), "desc", "mask", False),
    "desc_cos_nomask": ("DescriptorsLoss", dict(weight=1.0, mode="cosine_similarity"), "desc", None, False),
    "score_mse_mask": ("ScoreLoss", dict(weight=1.0, mode="mse"), "score", "mask", False),
    "score_mae_mask": ("ScoreLoss", dict(weight=3.0, mode="mae"), "score", "mask", False),
    "score_mse_empty": ("ScoreLoss", dict(weight=1.0, mode="mse"), "score", "mask_empty", False),
    "score_mae_empty": ("ScoreLoss", dict(weight=1.0, mode="mae"), "score", "mask_empty", False),
    "score_mse_nomask": ("ScoreLoss", dict(weight=1.0, mode="mse"), "score", None, False),
    "score_mae_nomask": ("ScoreLoss", dict(weight=1.0, mode="mae"), "score", None, False),
    "score_whole_mask": ("ScoreLoss", dict(weight=1.0, mode="mse-whole"), "score", "mask", False),
    "score_bce_mask": ("ScoreLoss", dict(weight=1.0, mode="bce"), "score", "mask", False),
    "logits_mask_padder": ("LogitsLoss", dict(weight=1.5, mode="mse", cell_size=CELL), "logits", "mask", True),
    "logits_nomask_padder": ("LogitsLoss", dict(weight=1.0, mode="mse", cell_size=CELL), "logits", None, True),
    "logits_nomask_nopadder": ("LogitsLoss", dict(weight=1.0, mode="mse", cell_size=CELL), "logits", None, False),
    "feature_mse": ("FeatureLoss", dict(weight=1.0, mode="mse"), "feat", None, False),
    "feature_mae": ("FeatureLoss", dict(weight=2.0, mode="mae"), "feat", None, False),
}
RAISE_CASES = {
    "desc_mse_nomask": ("DescriptorsLoss", dict(weight=1.0, mode="mse"), "desc", None, False),
    "desc_cos_mask": ("DescriptorsLoss", dict(weight=1.0, mode="cosine_similarity"), "desc", "mask", False),
}


def restate(name, d):
    """float64 value of VALUE_CASES[name] on the inputs d"""
    cls, kw, key, mkey, padded = VALUE_CASES[name]
    pred, gt = d[key + "_pred"], d[key + "_gt"]
    mask = None if mkey is None else d[mkey]
    weight = kw["weight"]
    if cls == "DescriptorsLoss":
        s, c, f = descriptors_loss(pred, gt, mask, kw["mode"], kw.get("use_mask", True))
        with np.errstate(invalid="ignore", divide="ignore"):
            return weight * f(np.sum(s) / np.sum(c))
    if cls == "ScoreLoss":
        s, c, _ = score_loss(pred, gt.copy(), mask, kw["mode"], kw.get("use_mask", True))
    elif cls == "LogitsLoss":
        s, c = logits_sums(pred, gt, kw["cell_size"], PADS if padded else None, mask)
    else:
        s, c = map_sums(pred, gt, None, {"mse": "sq", "mae": "abs"}[kw["mode"]])
    return value(s, c, weight)
