"""Small geometry helpers of core.geometry (reference core/geometry/utils.py): the same names, signatures and defaults, written
from their contracts.  Plain torch (or numpy, where the reference takes either) on the caller's device: 3x3 and
O(N) work with no kernel behind it.  Pinhole only: the two distortion helpers are refused by name."""
import numpy as np
import torch


def to_homogeneous(points):
    """[..., N] -> [..., N + 1] with a trailing 1 (torch tensor or numpy array; anything else is a ValueError)"""
    if torch.is_tensor(points):
        return torch.cat([points, torch.ones_like(points[..., :1])], -1)
    if isinstance(points, np.ndarray):
        return np.concatenate([points, np.ones_like(points[..., :1])], -1)
    raise ValueError("einx: to_homogeneous takes a torch tensor or a numpy array")


def from_homogeneous(points, eps=0.0):
    """[..., N + 1] -> [..., N]: the leading coordinates over (the last one + eps)"""
    return points[..., :-1] / (points[..., -1:] + eps)


def batched_eye_like(x, n):
    """[len(x), n, n] identities of x's dtype on x's device"""
    return torch.eye(n, dtype=x.dtype, device=x.device).expand(len(x), n, n).clone()


def skew_symmetric(v):
    """[..., 3] -> [..., 3, 3], the matrix [v]x with [v]x w = v x w"""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(v.shape[:-1] + (3, 3))


def transform_points(T, points):
    """homogeneous matrix T [..., D + 1, D + 1] applied to points [..., N, D] (rows times T^T), dehomogenised"""
    return from_homogeneous(to_homogeneous(points) @ T.transpose(-1, -2))


def is_inside(pts, shape):
    """pts [B,N,D] strictly inside (0, shape[b]) in every coordinate; shape [B,D]"""
    return (pts > 0).all(-1) & (pts < shape[:, None]).all(-1)


def so3exp_map(w, eps: float = 1e-7):
    """axis-angle vectors [..., 3] -> rotations [..., 3, 3] (Rodrigues): I + sin(a) [k]x + (1 - cos(a)) [k]x^2 with a = |w| and
    k = w / a; below eps the first-order I + [w]x"""
    angle = w.norm(p=2, dim=-1, keepdim=True)
    small = angle < eps
    K = skew_symmetric(w / torch.where(small, torch.ones_like(angle), angle))
    a = angle[..., None]
    full = K * torch.sin(a) + (K @ K) * (1 - torch.cos(a))
    return torch.eye(3, dtype=K.dtype, device=K.device) + torch.where(small[..., None], K, full)


def distort_points(pts, dist):
    raise NotImplementedError("einx: only pinhole cameras are supported: distort_points (radial / tangential distortion) is not provided")


def J_distort_points(pts, dist):
    raise NotImplementedError("einx: only pinhole cameras are supported: J_distort_points (radial / tangential distortion) is not provided")


def get_image_coords(img):
    """[1,H,W,2] float32 pixel centres (x + 0.5, y + 0.5) of an image [..., H, W], on its device"""
    h, w = img.shape[-2:]
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=img.device), torch.arange(w, dtype=torch.float32, device=img.device),
                          indexing="ij")
    return torch.stack([x, y], -1)[None] + 0.5
