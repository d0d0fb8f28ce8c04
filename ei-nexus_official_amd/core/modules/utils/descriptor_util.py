"""Descriptor post-processing helpers with the reference's names and signatures
(core/modules/utils/descriptor_util.py), backed by csrc/desc.hip (kernels K6/K10)."""
import torch

from ...._native import desc_sample, desc_sample_pos, normalize_map, upsample_normalize


def _f32(t):
    return t if t.dtype == torch.float32 else t.to(torch.float32)


def _scale(scale_factor):
    return float(scale_factor.detach()) if torch.is_tensor(scale_factor) else float(scale_factor)


def normalize_descriptors(raw_descriptors, scale_factor=1.0, normalize=True):
    """L2 normalisation over dim 1 times scale (descriptor_util.py:21-28)."""
    if not normalize:
        raise NotImplementedError("einx: un-normalised descriptors are not used by EI-Nexus")
    return normalize_map(_f32(raw_descriptors).contiguous(), _scale(scale_factor))


def get_dense_descriptors(normalized_descriptors):
    """[B,C,H,W] -> [B,H*W,C] view (descriptor_util.py:40-47)."""
    B, C = normalized_descriptors.shape[:2]
    return normalized_descriptors.reshape(B, C, -1).permute(0, 2, 1)


def _pack_positions(positions, size, bilinear):
    """list of [n_i,>=2] (y,x) positions on a [H,W] = `size` grid -> (indices [B,cap] int32, counts [B] int32); integer index
    arithmetic only (floor, y*W+x).  The positions are validated first, because the kernels read at the index unchecked:
      gather (bilinear=False): a position outside the map is an IndexError, as the reference's `raw[i, :, y, x]` raises for an
        index >= size (descriptor_util.py:59-61; it would wrap a negative one, which no detector emits: refused here too);
      bilinear: the sampler takes its sample at the centre of the position's pixel, so a position whose fractional part is not
        0.5 (the reference's grid_sample interpolates at the float position, descriptor_util.py:105-121) or that lies outside
        the padded image (zero padding there) is refused, not silently moved.  A NaN is refused by either rule.
    The check is one small reduction and one read-back per call: these drop-in helpers are off the hot path -- the extractors
    hand the detector's own `indices` straight to desc_sample and never come through here."""
    B = len(positions)
    H, W = int(size[0]), int(size[1])
    cap = max([int(p.shape[0]) for p in positions] + [1])
    dev = positions[0].device
    idx = torch.zeros((B, cap), dtype=torch.int32, device=dev)
    cnt = torch.tensor([int(p.shape[0]) for p in positions], dtype=torch.int32, device=dev)
    bad = []
    for b, p in enumerate(positions):
        if p.shape[0]:
            yx = p[:, :2]
            fl = yx.floor()
            ok = (fl[:, 0] >= 0) & (fl[:, 0] < H) & (fl[:, 1] >= 0) & (fl[:, 1] < W)
            if bilinear:
                ok = ok & (yx - fl == 0.5).all(dim=1)
            bad.append((~ok).any())
            fi = fl.to(torch.int32)
            idx[b, :p.shape[0]] = fi[:, 0] * W + fi[:, 1]
    if bad and bool(torch.stack(bad).any()):
        if bilinear:
            raise NotImplementedError(f"einx: sparsify_low_resolution_descriptors samples at pixel centres (y + 0.5, x + 0.5) inside the "
                                      f"padded image {(H, W)}; a position with another fractional part or outside it is not supported "
                                      f"(sample_descriptors_at samples at any position)")
        raise IndexError(f"position out of bounds for the descriptor map of size {(H, W)}")
    return idx, cnt


def sparsify_full_resolution_descriptors(raw_descriptors, positions, scale_factor=1.0, normalize=True):
    """integer gather + normalise for cell-1 networks (descriptor_util.py:50-71); IndexError for a position outside the map."""
    if not normalize:
        raise NotImplementedError
    raw = _f32(raw_descriptors).contiguous()
    H, W = raw.shape[-2:]
    idx, cnt = _pack_positions(positions, (H, W), bilinear=False)
    out = desc_sample(raw, idx, cnt, (H, W), bilinear=False, scale=_scale(scale_factor))
    return tuple(out[b, :int(positions[b].shape[0])] for b in range(len(positions)))


def sparsify_low_resolution_descriptors(raw_descriptors, positions, image_size, scale_factor=1.0, normalize=True):
    """bilinear grid_sample at keypoints + normalise for cell-8 networks (descriptor_util.py:74-128).  The positions are pixel
    centres of the padded image (what the detector emits); see _pack_positions for what is refused."""
    if not normalize:
        raise NotImplementedError
    raw = _f32(raw_descriptors).contiguous()
    Hp, Wp = int(image_size[0]), int(image_size[1])
    idx, cnt = _pack_positions(positions, (Hp, Wp), bilinear=True)
    out = desc_sample(raw, idx, cnt, (Hp, Wp), bilinear=True, scale=_scale(scale_factor))
    return [out[b, :int(positions[b].shape[0])] for b in range(len(positions))]


def sample_descriptors_at(raw_descriptors, positions, image_size, scale_factor=1.0, ordering="yx"):
    """What the reference's sparsify_low_resolution_descriptors (descriptor_util.py:74-128) returns for ANY finite positions --
    projected, warped or sub-pixel points, inside or outside the image: bilinear grid_sample (align_corners=False, zero padding)
    of raw_descriptors [B,C,hc,wc] at the float positions (list of [n_i,>=2] rows, (y, x, ..) or with ordering="xy" (x, y, ..), in
    the frame of `image_size` = (H, W) with pixel centres at .5), then normalise * scale.  -> list of [n_i,C].
    A non-finite coordinate is a ValueError (one small reduction and one read-back per call, as in _pack_positions)."""
    if ordering not in ("yx", "xy"):
        raise ValueError(f"ordering must be 'yx' or 'xy', got {ordering!r}")
    raw = _f32(raw_descriptors).contiguous()
    B = len(positions)
    if B != raw.shape[0]:
        raise ValueError(f"{B} position lists for a batch of {raw.shape[0]} descriptor maps")
    ns = [int(p.shape[0]) for p in positions]
    if any(p.dim() != 2 or p.shape[1] < 2 for p in positions):
        raise ValueError("positions must be [n, >= 2] per image")
    nonempty = [_f32(p[:, :2]) for p in positions if p.shape[0]]
    if nonempty and not bool(torch.stack([torch.isfinite(p).all() for p in nonempty]).all()):
        raise ValueError("einx: sample_descriptors_at needs finite positions (a NaN or infinite coordinate was given)")
    cap = max(ns + [1])
    pos = torch.zeros((B, cap, 2), dtype=torch.float32, device=raw.device)
    for b, p in enumerate(positions):
        if ns[b]:
            pos[b, :ns[b]] = p[:, :2]
    cnt = torch.tensor(ns, dtype=torch.int32, device=raw.device)
    out = desc_sample_pos(raw, pos, cnt, (int(image_size[0]), int(image_size[1])), _scale(scale_factor), ordering=ordering)
    return [out[b, :ns[b]] for b in range(B)]


def upsample_descriptors(raw_descriptors, image_size, scale_factor=1.0):
    """bilinear resize + normalise (descriptor_util.py:131-138)."""
    return upsample_normalize(_f32(raw_descriptors).contiguous(), image_size, (0, 0, 0, 0), _scale(scale_factor))
