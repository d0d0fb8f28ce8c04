"""Validation pairs by covisibility: the selection of the reference's
datasets/generate_MVSEC_relative_pose_val.py::check_indices (:194-346) on the device.

check_indices labels every pixel centre of both views against each other with gt_matches_from_pose_depth and keeps a pair when
0.4 < #(matches0 > -1) / min(#visible0, #visible1) < 0.8.  Here the depth frames and poses of a sequence are uploaded once, the
index pairs go through einx_gt_dense in batches (frames picked by index on the device: no per-pair depth copies, no label
buffers), and each batch costs one host read-back."""
import numpy as np
import torch

from ..core.geometry.gt_generation import valid_ratio
from ..core.metrics._native_metrics import geom_dense_warp, gt_matches_dense, relative_pose


def grid_keypoints(H, W, ordering="yx", device=None):
    """[H W, 2] float32 pixel centres in raster order (keypoint y W + x is the pixel (x, y)): (y + 0.5, x + 0.5) for "yx", which is
    the grid check_indices labels, or (x + 0.5, y + 0.5) for "xy" """
    if ordering not in ("yx", "xy"):
        raise ValueError("ordering must be 'yx' or 'xy'")
    i = torch.arange(H * W, device=device)
    y, x = torch.div(i, W, rounding_mode="floor"), i % W
    return torch.stack([y, x] if ordering == "yx" else [x, y], 1).float() + 0.5


def covisibility(depth0, depth1, K0, K1, T_0to1, T_1to0=None, pos_th=3, neg_th=5, idx0=None, idx1=None):
    """Counts and ratio only (no label buffers), no host sync: {"counts": [B,4] int32 = #(matches0 > -1), #(matches1 > -1),
    #visible0, #visible1, "valid_ratio": [B] float32}.  Arguments as gt_matches_dense."""
    c = gt_matches_dense(depth0, depth1, K0, K1, T_0to1, T_1to0, pos_th=pos_th, neg_th=neg_th, idx0=idx0, idx1=idx1, labels=False)["counts"]
    return {"counts": c, "valid_ratio": valid_ratio(c)}


def pair_overlap(depth0, depth1, K0, K1, T_0to1, T_1to0=None, cc_th=None):
    """[B,2] float32 overlap of each pair, no host sync: column 0 the share of view 0's valid pixels (depth > 0) that view 1 sees,
    column 1 the same for view 1, from the counts of one dense-warp launch over both directions (einx_geom_dense_warp, DESIGN.md
    8t).  cc_th (None: off) bounds the SQUARED cycle distance in pixels^2, so that a pixel hidden behind a nearer surface of the
    other view is not counted as seen.  A view without a valid pixel gives NaN (0 / 0).  depth [B,H,W], K [B,3,3], T [B,4,4]
    (T_1to0 None: the inverse of T_0to1, taken in the kernel)."""
    c = geom_dense_warp(depth0, depth1, K0, K1, T_0to1, T_1to0, cc_bound=cc_th, both=True)["counts"].to(torch.float32)
    return c[:, :, 1] / c[:, :, 0]


def rigid_inverse(T):
    """[..., 4, 4] float64 -> (R^T, -R^T t): the closed-form inverse of a rigid transform"""
    T = np.asarray(T, np.float64)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -np.einsum("...rk,...k->...r", Rt, T[..., :3, 3])
    out[..., 3, 3] = 1.0
    return out


def relative_transforms(poses, pairs):
    """T_0to1 = pose1 pose0^-1 and T_1to0 = pose0 pose1^-1 for index pairs [P,2] into world poses [F,4,4], in float64 with the rigid
    closed-form inverse, then cast to float32"""
    poses = np.asarray(poses, np.float64)
    inv = rigid_inverse(poses)
    i0, i1 = pairs[:, 0], pairs[:, 1]
    return (poses[i1] @ inv[i0]).astype(np.float32), (poses[i0] @ inv[i1]).astype(np.float32)


def _verify(depth, K, T01, T10, pair, pos_th, neg_th):
    """check_indices :277-293 for one kept pair: relative_pose on kpts0[matches0 > -1] and their partners -> (R_err, t_err, inliers)"""
    H, W = depth.shape[-2:]
    r = gt_matches_dense(depth, depth, K[None], K[None], T01[None], T10[None], pos_th=pos_th, neg_th=neg_th, idx0=pair[:1], idx1=pair[1:])
    m0 = r["matches0"][0]
    kp = grid_keypoints(H, W, "yx", depth.device)
    sel = m0 > -1
    mk0, mk1 = kp[sel], kp[m0[sel]]
    if mk0.shape[0] == 0:
        return (float("inf"),) * 3
    n = torch.tensor([mk0.shape[0]], dtype=torch.int32, device=depth.device)
    _, _, _, status, rows = relative_pose(mk0[None].contiguous(), mk1[None].contiguous(), n, K[None], K[None], T01[None], thresh=1.0,
                                          conf=0.999, ordering="yx")
    if int(status[0]) < 0:
        return (float("inf"),) * 3
    rows = rows[0].tolist()
    return rows[0], rows[1], rows[3]


@torch.no_grad()
def select_pairs(depth_frames, K, poses, indices, ratio_range=(0.4, 0.8), pos_th=3, neg_th=5, batch=64, verify=False, device="cuda"):
    """check_indices' selection.  depth_frames [F,H,W] are uploaded once (a tensor already on `device` is used as it is); the world
    poses [F,4,4] and `indices` [P,2] are read on the host (numpy, lists, or tensors on any device, which are copied back once);
    K [3,3] is the one camera of both views.  The index pairs are processed `batch` at a time with one host read-back each.  index0 == index1 is skipped, as in the reference.  A pair is kept when lo < valid_ratio < hi, both strict; a
    NaN ratio (no visible pixel on a side) is never kept.

    T_0to1 = pose1 pose0^-1 and T_1to0 = pose0 pose1^-1 are formed in float64 with the rigid closed-form inverse (R^T, -R^T t) and
    cast to float32.  The reference uses np.linalg.inv; the two can differ in the last float32 bit.

    Returns a dict: "pairs" [n,2] int64, the kept index pairs in input order; "candidates" [P',2] int64, the pairs that were
    evaluated (input order, without index0 == index1); and per candidate "counts" [P',4] int32, "valid_ratio" [P'] float32, "kept"
    [P'] bool.  With `verify`, per kept pair also "R_err", "t_err" (degrees) and "inliers" (ratio) of relative_pose on the dense
    matches (threshold 1.0, confidence 0.999; inf where no pose is found): reporting only, as in the reference, it never
    affects the selection."""
    lo, hi = ratio_range
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
    pairs, poses = host(indices).astype(np.int64).reshape(-1, 2), host(poses).astype(np.float64)
    depth = torch.as_tensor(depth_frames).to(device, torch.float32)
    F = depth.shape[0]
    if pairs.size and (pairs.min() < 0 or pairs.max() >= F):
        raise IndexError(f"einx: select_pairs: an index outside [0, {F})")
    if poses.shape != (F, 4, 4):
        raise ValueError("einx: select_pairs: poses must be [F,4,4], one per depth frame")
    cand = pairs[pairs[:, 0] != pairs[:, 1]]
    T01, T10 = relative_transforms(poses, cand)
    Kd = torch.as_tensor(K).to(device, torch.float32).reshape(3, 3)
    counts, ratio = np.zeros((len(cand), 4), np.int32), np.zeros(len(cand), np.float32)
    for s in range(0, len(cand), batch):
        e = min(s + batch, len(cand))
        idx = torch.from_numpy(cand[s:e].astype(np.int32)).to(device)
        Kb = Kd.expand(e - s, 3, 3)
        r = covisibility(depth, depth, Kb, Kb, torch.from_numpy(T01[s:e]).to(device), torch.from_numpy(T10[s:e]).to(device), pos_th=pos_th,
                         neg_th=neg_th, idx0=idx[:, 0].contiguous(), idx1=idx[:, 1].contiguous())
        # counts and the ratio's bits in one int32 tensor: the batch's one read-back
        back = torch.cat([r["counts"].to(torch.int32), r["valid_ratio"].to(torch.float32).view(torch.int32)[:, None]], 1).cpu().numpy()
        counts[s:e], ratio[s:e] = back[:, :4], back[:, 4].copy().view(np.float32)
    with np.errstate(invalid="ignore"):
        kept = (ratio > lo) & (ratio < hi)  # NaN compares false
    out = {"pairs": cand[kept], "candidates": cand, "counts": counts, "valid_ratio": ratio, "kept": kept}
    if verify:
        rep = [_verify(depth, Kd, torch.from_numpy(T01[i]).to(device), torch.from_numpy(T10[i]).to(device),
                       torch.from_numpy(cand[i].astype(np.int32)).to(device), pos_th, neg_th) for i in np.nonzero(kept)[0]]
        rep = np.asarray(rep, np.float64).reshape(-1, 3)
        out.update(R_err=rep[:, 0], t_err=rep[:, 1], inliers=rep[:, 2])
    return out
