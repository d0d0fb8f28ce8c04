"""Perspective warp of image batches on the device (csrc/warp.hip): the second view of a homographic pair.  Warping
the image of a same-time pair by a known homography H gives exact correspondences for any recording, with no depth: the pair goes
to the evaluators' `homography=` argument and to gt_matches(..., homography=H) as it is.

Coordinates are continuous: pixel (r, c) is centred at (x, y) = (c + 0.5, r + 0.5), the convention of `sparse_positions` and of
the ground-truth matches.  H maps the SOURCE image to the DESTINATION image; the kernel walks the destination and needs H^-1,
formed once here in float64 by the adjugate (nine products of two, a determinant of three, nine divisions: every operation
rounded as written, the same on the host and on the device)."""
import torch

from .. import _native as N

MODES = tuple(N.WARP_MODES)


def invert_homography(H):
    """H [...,3,3] (any float dtype, host or device) -> H^-1 [...,3,3] float64 on H's device, by the adjugate over the determinant.
    Nothing is read back: a singular matrix gives non-finite entries, which make every pixel of its sample invalid."""
    lead = tuple(H.shape[:-2])
    a = H.to(torch.float64).reshape(*lead, 9).unbind(-1)
    c0, c1, c2 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c0 + a[1] * c1) + a[2] * c2
    adj = (c0, a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
           c1, a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
           c2, a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3])
    return torch.stack([v / det for v in adj], -1).reshape(*lead, 3, 3)


def _homographies(H, B):
    if not torch.is_tensor(H):
        H = torch.as_tensor(H)
    if not H.is_floating_point():
        raise ValueError(f"warp: H must be a float tensor, got {H.dtype}")
    if H.dim() == 2:
        H = H[None].expand(B, 3, 3) if tuple(H.shape) == (3, 3) else H
    if H.dim() != 3 or tuple(H.shape) != (B, 3, 3):
        raise ValueError(f"warp: H must be [{B}, 3, 3] or [3, 3], got {tuple(H.shape)}")
    return H


def warp_perspective(x, H, out_shape=None, mode="bilinear"):
    """Warp every image of a batch by its own homography in one launch: (warped, valid).

    x: [B,C,H,W] or [B,H,W] on the device; uint8, float32 or bool (bool goes through uint8 and `mode="nearest"`, whatever `mode`
    says).  A non-contiguous tensor is copied once; the caller's tensor is never written.
    H: [B,3,3] or [3,3] (one for all), source -> destination, any float dtype, on the host or on any device.
    out_shape: (Hd, Wd) of the result, None: the source's.
    mode: "bilinear" (four taps, float32 weights) or "nearest" (the source pixel is copied: masks, label images).
    warped: x's dtype and layout, [B,C,Hd,Wd] or [B,Hd,Wd]; valid: bool [B,1,Hd,Wd], true where the destination pixel's source
    point has all four taps inside the source image and lies in front of the camera (w > 0).  An invalid pixel is 0 (False) in
    `warped`: there is no border blending, so a network never sees a value made of a border.  Definitions: include/einx.h,
    einx_warp_perspective."""
    if not torch.is_tensor(x):
        raise ValueError(f"warp: x must be a tensor, got {type(x).__name__}")
    if x.dim() not in (3, 4):
        raise ValueError(f"warp: x must be [B, C, H, W] or [B, H, W], got {tuple(x.shape)}")
    if x.dtype not in (torch.uint8, torch.float32, torch.bool):
        raise ValueError(f"warp: x must be uint8, float32 or bool, got {x.dtype}")
    if mode not in MODES:
        raise ValueError(f"warp: mode must be one of {MODES}, got {mode!r}")
    if out_shape is None:
        out_shape = x.shape[-2:]
    try:
        Hd, Wd = (int(v) for v in out_shape)
    except (TypeError, ValueError):
        raise ValueError(f"warp: out_shape must be (Hd, Wd), got {out_shape!r}") from None
    if Hd < 0 or Wd < 0:
        raise ValueError(f"warp: out_shape must not be negative, got {(Hd, Wd)}")
    B = int(x.shape[0])
    H = _homographies(H, B)
    if x.device.type != "cuda":
        raise RuntimeError(f"einx: tensors must live on a HIP device (torch device type 'cuda'); there is no CPU path. Got a tensor on {x.device}.")
    is_bool = x.dtype == torch.bool
    src = x.contiguous()
    src = src.view(torch.uint8) if is_bool else src
    src = src[:, None] if x.dim() == 3 else src
    Hinv = invert_homography(H).reshape(B, 9).to(x.device).contiguous()
    dst, valid = N.warp_perspective(src, Hinv, Hd, Wd, "nearest" if is_bool else mode)
    dst = dst[:, 0] if x.dim() == 3 else dst
    return (dst.view(torch.bool) if is_bool else dst), valid.view(torch.bool)[:, None]
