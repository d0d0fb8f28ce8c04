"""Batched device-side evaluation metrics (csrc/metrics.hip)."""
import ctypes

import torch

from ..._native import on_input_device
from ... import _native as N
from ..._lib import HomographyParams, MetricParams, PoseParams, check


def metric_names(mma_thr=(1, 3), vdd_thr=(1, 3), prefix_vdd="VDD"):
    names = ["MR"] + [f"MMA@{t}" for t in mma_thr]
    for t in vdd_thr:
        names += [f"{prefix_vdd}_Repeatability@{t}", f"{prefix_vdd}_ValidDistance@{t}", f"{prefix_vdd}_Angle@{t}"]
    return names


@on_input_device
def pair_metrics(kpts0, desc0, n, kpts1, desc1, m, mk0, mk1, nmatch, size0, size1, homography=None, mma_thr=(1, 3), vdd_thr=(1, 3),
                 ordering="yx", rep_nan_if_empty=False):
    """All tensors on the device: kpts [B,cap,3], desc [B,cap,D], counts int32 [B], matched keypoints
    [B,cap0,cols] + nmatch.  Returns float64 [B, 1+len(mma_thr)+3*len(vdd_thr)] (see metric_names)."""
    B, cap0, _ = kpts0.shape
    cap1 = kpts1.shape[1]
    p = MetricParams()
    p.B, p.cap0, p.cap1, p.D, p.cols = B, cap0, cap1, desc0.shape[-1], mk0.shape[-1]
    p.H0, p.W0, p.H1, p.W1 = int(size0[0]), int(size0[1]), int(size1[0]), int(size1[1])
    p.kp_yx = int(ordering == "yx")
    p.n_mma, p.n_vdd = len(mma_thr), len(vdd_thr)
    p.rep_nan_if_empty = int(bool(rep_nan_if_empty))
    for i, t in enumerate(mma_thr):
        p.mma_thr[i] = float(t)
    for i, t in enumerate(vdd_thr):
        p.vdd_thr[i] = float(t)
    L = N.lib()
    dev = kpts0.device
    hom = None
    if homography is not None:
        hom = homography.to(dev, torch.float32).reshape(B, 9).contiguous()
    ws = N._workspace(L.einx_metrics_ws_bytes(ctypes.byref(p)), dev)
    out = torch.empty((B, 1 + p.n_mma + 3 * p.n_vdd), dtype=torch.float64, device=dev)
    N._dev_check(kpts0, kpts1, desc0, desc1, mk0, mk1)
    N._dev_check(n, m, nmatch, dt=torch.int32)
    check(L.einx_pair_metrics(ctypes.byref(p), N._ptr(kpts0), N._ptr(kpts1), N._ptr(desc0), N._ptr(desc1), N._ptr(n), N._ptr(m), N._ptr(mk0),
                              N._ptr(mk1), N._ptr(nmatch), N._ptr(hom), N._ptr(ws), N._ptr(out), N._stream(kpts0)), "einx_pair_metrics")
    return out


@on_input_device
def batch_metrics(ev, im, mr, homography=None, mma_thr=(1, 3), vdd_thr=(1, 3)):
    """Metrics for a whole EIM.forward_batched result (BatchedFeats x2 + MatchResult), no host sync."""
    return pair_metrics(ev.det.positions, ev.sparse_desc, ev.det.counts, im.det.positions, im.sparse_desc, im.det.counts, mr.mk0, mr.mk1,
                        mr.nmatch, ev.image_size, im.image_size, homography, mma_thr, vdd_thr, ordering=ev.ordering)


def _pad3(k):
    if k.shape[-1] == 3:
        return k
    return torch.cat([k, k.new_zeros(k.shape[0], 3 - k.shape[-1])], 1)


def single_pair(points1, points2, desc1, desc2, matched1, matched2, size0, size1, homography, mma_thr, vdd_thr, ordering="yx",
                rep_nan_if_empty=False):
    """update_one-style entry: per-pair tensors of any length -> dict of python floats."""
    dev = points1.device
    k0, k1 = _pad3(points1.float())[None].contiguous(), _pad3(points2.float())[None].contiguous()
    M = int(matched1.shape[0]) if matched1 is not None else 0
    cap0, cap1 = max(k0.shape[1], M, 1), max(k1.shape[1], 1)  # matched rows share image 0's capacity in the ABI
    D = desc1.shape[-1] if desc1 is not None else 4

    def fit(t, cap, width):
        out = torch.zeros((1, cap, width), dtype=torch.float32, device=dev)
        if t is not None and t.numel():
            out[0, :t.shape[0], :t.shape[1]] = t
        return out
    k0, k1 = fit(k0[0], cap0, 3), fit(k1[0], cap1, 3)
    d0, d1 = fit(desc1, cap0, D), fit(desc2, cap1, D)
    cols = matched1.shape[-1] if matched1 is not None and matched1.numel() else 3
    mk0, mk1 = fit(matched1, cap0, cols), fit(matched2, cap0, cols)
    cnt = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)  # noqa: E731
    hom = None if homography is None else homography.reshape(1, 3, 3)
    out = pair_metrics(k0, d0, cnt(points1.shape[0]), k1, d1, cnt(points2.shape[0]), mk0, mk1, cnt(M), size0, size1, hom, mma_thr, vdd_thr,
                       ordering, rep_nan_if_empty=rep_nan_if_empty)
    return dict(zip(metric_names(mma_thr, vdd_thr), out[0].tolist()))


POSE_SEED = 0x5EED0F5E
POSE_STATUS = {-1: "few", -2: "noE", -3: "cheir"}  # einx.h: >= 0 pose found, negative: why not


def _ransac_call(params, ws_bytes, mk0, mk1, nmatch, thresh, conf, ordering, max_iters, seed, row_width, **fields):
    """What a call of either RANSAC estimator starts with: the params struct (the fields both structs have; `fields` are the
    estimator's own), the input checks, and the workspace / mask / status / rows it writes.  Returns (p, ws, mask, status, rows)."""
    B, cap, cols = mk0.shape
    dev = mk0.device
    p = params()
    p.struct_size = ctypes.sizeof(params)
    p.B, p.cap, p.cols, p.kp_yx, p.max_iters = B, cap, cols, int(ordering == "yx"), int(max_iters)
    p.thresh, p.conf, p.seed = float(thresh), float(conf), int(seed)
    for k, v in fields.items():
        setattr(p, k, v)
    N._dev_check(mk0, mk1)
    N._dev_check(nmatch, dt=torch.int32)
    ws = N._workspace(ws_bytes(ctypes.byref(p)), dev)
    mask = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    rows = torch.empty((B, row_width), dtype=torch.float64, device=dev)
    return p, ws, mask, status, rows


@on_input_device
def relative_pose(mk0, mk1, nmatch, K0, K1, T_0to1=None, thresh=1.0, conf=0.999, ordering="yx", max_iters=1000, seed=POSE_SEED):
    """RANSAC essential matrix + recoverPose + update_one's errors for a batch (csrc/pose.hip), no host sync.
    mk0 / mk1 [B,cap,2|3] float32 and nmatch int32 [B] on the device, K0 / K1 [B,3,3] float32 or float64 (numpy's dtype rules
    follow K's), T_0to1 [B,4,4] or None.  Returns device tensors (R [B,3,3] f64, t [B,3] f64, mask [B,cap] bool,
    status [B] int32, rows [B,4] f64 = R_err, t_err, pose_err, inlier ratio)."""
    B, dev = mk0.shape[0], mk0.device
    k_f64 = K0.dtype == torch.float64 or K1.dtype == torch.float64
    kdt = torch.float64 if k_f64 else torch.float32
    K0 = K0.to(dev, kdt).reshape(B, 9).contiguous()
    K1 = K1.to(dev, kdt).reshape(B, 9).contiguous()
    T = None if T_0to1 is None else T_0to1.to(dev, torch.float64).reshape(B, 16).contiguous()
    L = N.lib()
    p, ws, mask, status, rows = _ransac_call(PoseParams, L.einx_relative_pose_ws_bytes, mk0, mk1, nmatch, thresh, conf, ordering, max_iters,
                                             seed, 4, k_f64=int(k_f64))
    R = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((B, 3), dtype=torch.float64, device=dev)
    check(L.einx_relative_pose(ctypes.byref(p), N._ptr(mk0), N._ptr(mk1), N._ptr(nmatch), N._ptr(K0), N._ptr(K1), N._ptr(T), N._ptr(ws),
                               N._ptr(R), N._ptr(t), N._ptr(mask), N._ptr(status), N._ptr(rows), N._stream(mk0)), "einx_relative_pose")
    return R, t, mask.bool(), status, rows


@on_input_device
def batch_relative_pose(mr, K0, K1, T_0to1=None, thresh=1.0, conf=0.999, ordering="yx"):
    """relative_pose of an EIM match result (MatchResult: mk0 / mk1 / nmatch), no host sync"""
    return relative_pose(mr.mk0, mr.mk1, mr.nmatch, K0, K1, T_0to1, thresh, conf, ordering)


@on_input_device
def essential_5pt(x1, x2):
    """the minimal solver alone (test aid): x1 / x2 [n,5,2] float64 -> (E [n,10,3,3], n_solutions [n] int32)"""
    n = x1.shape[0]
    x1 = x1.to(torch.float64).contiguous()
    x2 = x2.to(torch.float64).contiguous()
    E = torch.zeros((n, 10, 3, 3), dtype=torch.float64, device=x1.device)
    ns = torch.empty((n,), dtype=torch.int32, device=x1.device)
    check(N.lib().einx_essential_5pt(N._ptr(x1), N._ptr(x2), n, N._ptr(E), N._ptr(ns), N._stream(x1)), "einx_essential_5pt")
    return E, ns


HOMOGRAPHY_STATUS = {-1: "few", -2: "noH"}  # einx.h: >= 0 the chosen RANSAC iteration, negative: why there is no homography


@on_input_device
def homography(mk0, mk1, nmatch, img_shape=None, H_true=None, thresh=3.0, conf=0.995, ordering="yx", max_iters=2000, he_thr=(3, 5, 10),
               seed=POSE_SEED):
    """RANSAC homography + refit + LM polish + update_one's corner error for a batch (csrc/homography.hip), no host
    sync.  mk0 / mk1 [B,cap,2|3] float32 and nmatch int32 [B] on the device; img_shape (H, W) for every pair or [B,2], H_true
    [B,3,3] (cast to float32 as update_one does), or None for both.  Returns device tensors (H [B,3,3] f64, mask [B,cap] bool,
    status [B] int32, rows [B,len(he_thr)+2] f64 = (error <= t) per threshold, mean corner error, inlier ratio)."""
    B, dev = mk0.shape[0], mk0.device
    he_thr = tuple(he_thr)
    if len(he_thr) > 4:
        raise ValueError("at most 4 correctness thresholds")
    if img_shape is not None:
        img_shape = torch.as_tensor(img_shape).to(dev, torch.int32)
        img_shape = (img_shape.reshape(1, 2).expand(B, 2) if img_shape.numel() == 2 else img_shape.reshape(B, 2)).contiguous()
    Ht = None if H_true is None else H_true.to(dev, torch.float32).reshape(B, 9).contiguous()
    L = N.lib()
    p, ws, mask, status, rows = _ransac_call(HomographyParams, L.einx_homography_ws_bytes, mk0, mk1, nmatch, thresh, conf, ordering,
                                             max_iters, seed, len(he_thr) + 2, n_thr=len(he_thr))
    for i, t in enumerate(he_thr):
        p.he_thr[i] = float(t)
    H = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    check(L.einx_homography(ctypes.byref(p), N._ptr(mk0), N._ptr(mk1), N._ptr(nmatch), N._ptr(img_shape), N._ptr(Ht), N._ptr(ws), N._ptr(H),
                            N._ptr(mask), N._ptr(status), N._ptr(rows), N._stream(mk0)), "einx_homography")
    return H, mask.bool(), status, rows


@on_input_device
def batch_homography(mr, img_shape=None, H_true=None, thresh=3.0, conf=0.995, ordering="yx", he_thr=(3, 5, 10)):
    """homography of an EIM match result (MatchResult: mk0 / mk1 / nmatch), no host sync"""
    return homography(mr.mk0, mr.mk1, mr.nmatch, img_shape, H_true, thresh, conf, ordering, he_thr=he_thr)


@on_input_device
def homography_dlt(x1, x2):
    """the normalised DLT alone (test aid): x1 / x2 [n,npts,2] float64 -> (H [n,3,3] float64, ok [n] int32)"""
    n, npts = x1.shape[0], x1.shape[1]
    x1 = x1.to(torch.float64).contiguous()
    x2 = x2.to(torch.float64).contiguous()
    H = torch.zeros((n, 3, 3), dtype=torch.float64, device=x1.device)
    ok = torch.empty((n,), dtype=torch.int32, device=x1.device)
    check(N.lib().einx_homography_dlt(N._ptr(x1), N._ptr(x2), n, npts, N._ptr(H), N._ptr(ok), N._stream(x1)), "einx_homography_dlt")
    return H, ok
