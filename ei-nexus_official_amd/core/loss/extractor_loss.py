"""Forward values of the reference's extractor losses (core/loss/extractor_loss.py:6-383) on the device: same classes,
constructor arguments, `forward` signatures, return `(0-dim float32 tensor, {key: python float})` and `loss_info` keys.  The
arithmetic is csrc/loss.hip: every op returns one float64 (sum, count) pair per image, a loss value is
weight * sum(sums) / sum(counts) (pooled over the batch, as the reference computes it), `pair_values` gives
weight * sum_b / count_b per image for the evaluation harness.  The `.item()` of `loss_info` is the only host synchronisation
(the reference's too).  The reference's failures are reproduced: see DESIGN.md 8f for the table."""
import torch
from torch import nn

from ... import _native as N
from ..._extract import FeatsDict, _Lazy


class _PairLoss(nn.Module):
    info_key = None

    def _sums(self, pred_feats, gt_feats, mask=None, padder=None):
        """-> [B,2] float64 on the device: (sum, count) per image"""
        raise NotImplementedError

    def _value(self, s, c):
        return s / c  # 0 / 0 = NaN: an empty mask, like the reference

    def pair_values(self, pred_feats, gt_feats, mask=None, padder=None):
        """[B] float64 on the device: the loss of every pair on its own; no host synchronisation"""
        sc = self._sums(pred_feats, gt_feats, mask, padder)
        return self.weight * self._value(sc[:, 0], sc[:, 1])

    def _result(self, sc):
        loss = (self.weight * self._value(sc[:, 0].sum(), sc[:, 1].sum())).float()
        return loss, {self.info_key: loss.detach().item()}


class ScoreLoss(_PairLoss):
    info_key = "extractor_keypoints_loss"

    def __init__(self, weight, mode, use_mask=True):
        super().__init__()
        self.mode = mode
        self.weight = weight
        self.use_mask = use_mask

    def _sums(self, pred_feats, gt_feats, mask=None, padder=None):
        pred, gt = pred_feats["score"], gt_feats["score"]
        assert pred.shape == gt.shape, f"pred: {pred.shape}, gt: {gt.shape}"
        if not self.use_mask:
            mask = None
        if self.mode == "bce":  # the mask is ignored
            return N.map_loss(pred, gt, None, "bce")
        if self.mode == "mse-whole":
            if mask is not None:  # the ground truth is edited IN PLACE, then a plain MSE
                gt.view(gt.shape[0], -1)[mask.view(mask.shape[0], -1)] = 0.0
            return N.map_loss(pred, gt, None, "sq")
        if self.mode == "mse":
            return N.map_loss(pred, gt, mask, "sq")
        if self.mode == "mae":
            return N.map_loss(pred, gt, mask, "abs")
        raise NotImplementedError(f"Not implemented mode: {self.mode}")

    def forward(self, pred_feats, gt_feats, mask=None, padder=None):
        return self._result(self._sums(pred_feats, gt_feats, mask, padder))


class LogitsLoss(_PairLoss):
    info_key = "extractor_keypoints_loss"

    def __init__(self, weight, mode, cell_size):
        super().__init__()
        self.mode = mode
        self.weight = weight
        self.cell_size = cell_size

    def _sums(self, pred_feats, gt_feats, mask=None, padder=None):
        pred, gt = pred_feats["logits"], gt_feats["logits"]
        assert pred.shape == gt.shape, f"pred: {pred.shape}, gt: {gt.shape}"
        channel_dim = pred.shape[1]
        assert channel_dim == self.cell_size * self.cell_size + 1, f"channel_dim: {channel_dim}, cell_size: {self.cell_size}"
        if not self.cell_size > 1:
            assert channel_dim == 1, f"channel_dim: {channel_dim}, cell_size: {self.cell_size}"
        crop = None
        if padder is not None:
            w0, w1, h0, h1 = padder.padding_size
            Hp, Wp = self.cell_size * pred.shape[2], self.cell_size * pred.shape[3]
            crop = (h0, w0, Hp - h0 - h1, Wp - w0 - w1)
        return N.logits_loss(pred, gt, self.cell_size, crop, mask)

    def forward(self, pred_feats, gt_feats, mask=None, padder=None):
        return self._result(self._sums(pred_feats, gt_feats, mask, padder))


class DescriptorsLoss(_PairLoss):
    info_key = "extractor_descriptor_loss"
    _KEYS = {"normalized": "normalized_descriptors", "raw": "raw_descriptors", "coarse": "coarse_descriptors"}
    _DENSE_MODES = ("dual-softmax", "triplet", "mae+triplet")  # (H*W)^2 torch code in the reference; no shipped config uses them

    def __init__(self, weight, desc_type="normalized", mode="mse", use_mask=True, **kargs):
        super().__init__()
        self.weight = weight
        assert desc_type in ("normalized", "raw", "coarse")
        self.desc_type = desc_type
        self.mode = mode
        self.use_mask = use_mask
        self.kargs = kargs

    def _value(self, s, c):
        return 1 - s / c if self.mode == "cosine_similarity" else s / c

    def _fused_geometry(self, pred_feats, gt_feats, mask):
        """the two BatchedFeats when the fused kernel applies, else None"""
        if self.desc_type != "normalized":
            return None
        for d in (pred_feats, gt_feats):
            if not isinstance(d, FeatsDict) or d._batched is None or not dict.__contains__(d, "normalized_descriptors"):
                return None
            if not isinstance(dict.__getitem__(d, "normalized_descriptors"), _Lazy):
                return None  # resolved already, or replaced by the user: the given tensors are reduced
        a, b = pred_feats._batched, gt_feats._batched
        if a.raw is None or b.raw is None or a.raw.shape != b.raw.shape or a.raw.device != b.raw.device:
            return None
        if (a.cell, tuple(a.pads), tuple(a.padded)) != (b.cell, tuple(b.pads), tuple(b.padded)) or a.cell not in (1, 8):
            return None
        if mask is not None:
            w0, w1, h0, h1 = a.pads
            H, W = a.padded[0] - h0 - h1, a.padded[1] - w0 - w1
            if mask.dim() != 4 or tuple(mask.shape) != (a.raw.shape[0], 1, H, W):
                return None
        return a, b

    def _sums(self, pred_feats, gt_feats, mask=None, padder=None):
        if not self.use_mask:
            mask = None
        fused = self._fused_geometry(pred_feats, gt_feats, mask)
        if fused is None:
            key = self._KEYS[self.desc_type]
            pred, gt = pred_feats[key], gt_feats[key]
            assert pred.shape == gt.shape
            shape = pred.shape
        else:
            r = fused[0].raw
            w0, w1, h0, h1 = fused[0].pads
            shape = (r.shape[0], r.shape[1], fused[0].padded[0] - h0 - h1, fused[0].padded[1] - w0 - w1)
        if self.mode in self._DENSE_MODES:
            raise NotImplementedError(f"einx: DescriptorsLoss mode {self.mode!r} is not built (dense (H*W)^2 torch code in the reference; DESIGN.md 8f)")
        if self.mode not in ("mse", "mae", "cosine_similarity"):
            raise NotImplementedError(f"Not implemented mode: {self.mode}")
        if self.mode == "mse" and mask is None:  # the reference calls F.mse_loss(pred - gt): one argument
            raise TypeError("mse_loss() missing 1 required positional argument: 'target'")
        if self.mode == "cosine_similarity" and mask is not None:
            n_mask = mask.numel() * (shape[1] if mask.dim() > 1 and mask.shape[1] == 1 else 1)  # a [B,1,H,W] mask is repeated over the channels
            n_cos = shape[0] * int(torch.Size(shape[2:]).numel())
            if n_mask != n_cos:  # ... and then indexes the [B,H,W] cosine map
                raise IndexError(f"The shape of the mask [{n_mask}] at index 0 does not match the shape of the indexed tensor [{n_cos}] at index 0")
        if fused is not None:
            a, b = fused
            mode = {"mse": "mse", "mae": "mae", "cosine_similarity": "cos"}[self.mode]
            with torch.cuda.device(a.raw.device):
                return N.desc_loss(a.raw, a.scale, b.raw, b.scale, a.padded, a.pads, a.cell, mask, mode)
        mode = {"mse": "sq", "mae": "abs", "cosine_similarity": "cos"}[self.mode]
        return N.map_loss(pred, gt, mask, mode)

    def forward(self, pred_feats, gt_feats, mask=None):
        return self._result(self._sums(pred_feats, gt_feats, mask))


class FeatureLoss(_PairLoss):
    info_key = "feature_loss"

    def __init__(self, weight, mode, **kargs):
        super().__init__()
        self.weight = weight
        self.mode = mode

    def _sums(self, pred_feats, gt_feats, mask=None, padder=None):
        pred, gt = pred_feats["backbone_feats"], gt_feats["backbone_feats"]
        assert pred.shape == gt.shape, f"pred: {pred.shape}, gt: {gt.shape}"
        if self.mode == "mse":
            return N.map_loss(pred, gt, None, "sq")
        if self.mode == "mae":
            return N.map_loss(pred, gt, None, "abs")
        raise NotImplementedError(f"Not implemented mode: {self.mode}")

    def forward(self, pred_feats, gt_feats):
        return self._result(self._sums(pred_feats, gt_feats))
