"""Essential / fundamental matrices, epipolar distances and pose errors (reference core/geometry/epipolar.py): the same names,
signatures and defaults, written from their contracts.

sym_epipolar_distance_all is a kernel (einx_epipolar_all, csrc/geometry.hip: no [B,N,M] temporaries besides the result); the 3x3
and O(N) functions are plain torch on the caller's device."""
import torch

from ..metrics._native_metrics import epipolar_all
from .utils import skew_symmetric, to_homogeneous
from .wrappers import Camera, Pose  # noqa: F401


def T_to_E(T):
    """E = [t]x R of a Pose (batched)"""
    return skew_symmetric(T.t) @ T.R


def E_to_F(cam0, cam1, E):
    """F = K1^-T E K0^-1"""
    return cam1.calibration_matrix().inverse().transpose(-1, -2) @ E @ cam0.calibration_matrix().inverse()


def T_to_F(cam0, cam1, T_0to1):
    return E_to_F(cam0, cam1, T_to_E(T_0to1))


def F_to_E(cam0, cam1, F):
    """E = K1^T F K0"""
    return cam1.calibration_matrix().transpose(-1, -2) @ F @ cam0.calibration_matrix()


def _hom(p):
    return p if p.shape[-1] == 3 else to_homogeneous(p)


def sym_epipolar_distance(p0, p1, E, squared=True):
    """p0, p1 [..., N, 2|3] paired points, E [..., 3, 3] from view 0 to view 1 -> [..., N].  With s = p1^T E p0 and the squared norms
    d0, d1 of the first two coefficients of the lines E p0 and E^T p1 (each clamped to >= 1e-6): s^2 (1 / d0 + 1 / d1), or with
    squared=False |s| (1 / sqrt(d0) + 1 / sqrt(d1)) / 2.  No points: zeros."""
    if p0.shape[-2] != p1.shape[-2]:
        raise AssertionError("einx: sym_epipolar_distance takes the same number of points on both sides")
    if p0.shape[-2] == 0:
        return torch.zeros(p0.shape[:-1]).to(p0)
    p0, p1 = _hom(p0), _hom(p1)
    line1 = p0 @ E.transpose(-1, -2)  # rows E p0
    line0 = p1 @ E                    # rows E^T p1
    s = (p1 * line1).sum(-1)
    d0 = (line1[..., 0] ** 2 + line1[..., 1] ** 2).clamp(min=1e-6)
    d1 = (line0[..., 0] ** 2 + line0[..., 1] ** 2).clamp(min=1e-6)
    if squared:
        return s ** 2 * (1 / d0 + 1 / d1)
    return s.abs() * (1 / d0.sqrt() + 1 / d1.sqrt()) / 2


def sym_epipolar_distance_all(p0, p1, E, eps=1e-15):
    """p0 [..., N, 2|3], p1 [..., M, 2|3], E [..., 3, 3] -> [..., N, M] float32: the mean of the distances of p1[m] to the line
    E p0[n] and of p0[n] to the line E^T p1[m] (eps under the roots), on the device"""
    lead = p0.shape[:-2]
    N, M = p0.shape[-2], p1.shape[-2]
    B = 1
    for s in lead:
        B *= s
    if B == 0:
        return p0.new_zeros(lead + (N, M), dtype=torch.float32)
    out = epipolar_all(p0.reshape(B, N, p0.shape[-1]), p1.reshape(B, M, p1.shape[-1]), E.expand(lead + (3, 3)).reshape(B, 3, 3), eps)
    return out.reshape(lead + (N, M))


def generalized_epi_dist(kpts0, kpts1, cam0, cam1, T_0to1, all=True, essential=True):
    """the epipolar distance of keypoints under a pose: in normalised coordinates under E (essential) or in pixels under
    F = K1^-T E K0^-1; all pairs [..., N, M] or paired points [..., N] (unsquared).  The all=True, essential=True arm is a
    TypeError, as it is in the reference, whose call there passes an aggregation argument its own function does not take."""
    E = T_to_E(T_0to1)
    if essential:
        if all:
            raise TypeError("sym_epipolar_distance_all() got an unexpected keyword argument 'agg'")
        return sym_epipolar_distance(cam0.image2cam(kpts0), cam1.image2cam(kpts1), E, squared=False)
    F = E_to_F(cam0, cam1, E)
    if all:
        return sym_epipolar_distance_all(kpts0, kpts1, F)
    return sym_epipolar_distance(kpts0, kpts1, F, squared=False)


def decompose_essential_matrix(E):
    """E [..., 3, 3] -> (R1, R2, t): the two rotations U W V^T and U W^T V^T of its SVD (U and V^T made proper by negating their last
    column / row) and the translation direction, U's last column"""
    U, _, V = torch.svd(E)
    Vt = V.transpose(-2, -1)
    flip = torch.ones_like(E)
    flip[..., :, -1] = -1.0
    U = torch.where((torch.det(U) < 0.0)[..., None, None], U * flip, U)
    Vt = torch.where((torch.det(Vt) < 0.0)[..., None, None], Vt * flip.transpose(-2, -1), Vt)
    W = E.new_tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])[None]
    return U @ W @ Vt, U @ W.transpose(-2, -1) @ Vt, U[..., -1]


def angle_error_mat(R1, R2):
    """the angle of R1^T R2 in degrees (3x3 matrices)"""
    cos = torch.clip((torch.trace(R1.T @ R2) - 1) / 2, -1.0, 1.0)
    return torch.rad2deg(torch.abs(torch.arccos(cos)))


def angle_error_vec(v1, v2, eps=1e-10):
    """the angle between two vectors in degrees; the product of the norms is kept >= eps"""
    n = torch.clip(v1.norm(dim=-1) * v2.norm(dim=-1), min=eps)
    return torch.rad2deg(torch.arccos(torch.clip((v1 * v2).sum(dim=-1) / n, -1.0, 1.0)))


def relative_pose_error(T_0to1, R, t, ignore_gt_t_thr=0.0, eps=1e-10):
    """(t_err, r_err) in degrees of an estimate (R, t) against T_0to1 (a Pose or a 4x4 tensor).  The translation is compared up to
    sign (an essential matrix leaves it open); below ignore_gt_t_thr of true translation t_err is 0."""
    if torch.is_tensor(T_0to1):
        R_gt, t_gt = T_0to1[:3, :3], T_0to1[:3, 3]
    else:
        R_gt, t_gt = T_0to1.R, T_0to1.t
    R_gt, t_gt = torch.squeeze(R_gt), torch.squeeze(t_gt)
    t_err = angle_error_vec(t, t_gt, eps)
    t_err = torch.minimum(t_err, 180 - t_err)
    if t_gt.norm() < ignore_gt_t_thr:
        t_err = 0
    return t_err, angle_error_mat(R, R_gt)
