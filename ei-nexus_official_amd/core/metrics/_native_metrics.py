"""Batched device-side evaluation metrics (csrc/metrics.hip)."""
import ctypes

import torch

from ..._native import on_input_device
from ... import _native as N
from ..._lib import AbsPoseParams, GeomDenseParams, GeomProjectParams, GtDenseParams, GtMatchesParams, HomographyParams, MetricParams, PoseMetricParams, PoseParams, PoseRefineParams, check


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


def pose_metric_names(mma_thr=(1, 3), vdd_thr=(1, 3), epi_thr=()):
    """the columns of pair_metrics_pose: DT_ for what is measured through depth and motion, EPI@t for the motion alone"""
    names = ["MR"] + [f"DT_MMA@{t}" for t in mma_thr] + ["DT_judged_ratio"]
    for t in vdd_thr:
        names += [f"DT_Repeatability@{t}", f"DT_ValidDistance@{t}", f"DT_Angle@{t}"]
    return names + [f"EPI@{t}" for t in epi_thr]


@on_input_device
def pair_metrics_pose(kpts0, desc0, n, kpts1, desc1, m, mk0, mk1, nmatch, size0, size1, K0, K1, T_0to1, T_1to0=None, depth0=None,
                      depth1=None, mma_thr=(1, 3), vdd_thr=(1, 3), epi_thr=(), occlusion_th=None, ordering="yx"):
    """pair_metrics for a pair related by depth and motion instead of a homography (einx_pair_metrics_pose), no host
    sync.  Keypoints, descriptors, counts and matched rows as pair_metrics takes them; size0 / size1 the image sizes (H, W);
    K0 / K1 [B,3,3], T_0to1 [B,4,4] (T_1to0 None: inverted in the kernel); depth0 [B,dH0,dW0] and depth1 [B,dH1,dW1], both or
    neither -- without them only MR and EPI@t are finite.  occlusion_th (pixels; None or <= 0: off) drops what the other view's depth
    map says is hidden.  Returns float64 [B, 2 + len(mma_thr) + 3 * len(vdd_thr) + len(epi_thr)] (see pose_metric_names)."""
    if (depth0 is None) != (depth1 is None):
        raise ValueError("einx: pair_metrics_pose takes both depth maps or neither")
    mma_thr, vdd_thr, epi_thr = tuple(mma_thr), tuple(vdd_thr), tuple(epi_thr)
    if max(len(mma_thr), len(vdd_thr), len(epi_thr)) > 4:
        raise ValueError("einx: at most 4 thresholds per metric")
    B, cap0, _ = kpts0.shape
    dev = kpts0.device
    p = PoseMetricParams()
    p.struct_size = ctypes.sizeof(PoseMetricParams)
    p.B, p.cap0, p.cap1, p.D, p.cols = B, cap0, kpts1.shape[1], desc0.shape[-1], mk0.shape[-1]
    p.H0, p.W0, p.H1, p.W1 = int(size0[0]), int(size0[1]), int(size1[0]), int(size1[1])
    p.kp_yx = int(ordering == "yx")
    p.n_mma, p.n_vdd, p.n_epi = len(mma_thr), len(vdd_thr), len(epi_thr)
    for dst, thr in ((p.mma_thr, mma_thr), (p.vdd_thr, vdd_thr), (p.epi_thr, epi_thr)):
        for i, t in enumerate(thr):
            dst[i] = float(t)
    p.occlusion_th = 0.0 if occlusion_th is None else float(occlusion_th)
    d0 = d1 = None
    if depth0 is not None:
        d0, d1 = (d.to(dev, torch.float32).reshape(B, d.shape[-2], d.shape[-1]).contiguous() for d in (depth0, depth1))
        p.dH0, p.dW0, p.dH1, p.dW1 = d0.shape[1], d0.shape[2], d1.shape[1], d1.shape[2]
    K0, K1, T01 = _f32c(K0, dev, (B, 9)), _f32c(K1, dev, (B, 9)), _f32c(T_0to1, dev, (B, 16))
    T10 = None if T_1to0 is None else _f32c(T_1to0, dev, (B, 16))
    L = N.lib()
    nbytes = L.einx_pair_metrics_pose_ws_bytes(ctypes.byref(p))
    if nbytes == 0:
        raise ValueError("einx: pair_metrics_pose: bad shape (sizes must be positive, matched rows have 2 or 3 columns)")
    ws = N._workspace(nbytes, dev)
    out = torch.empty((B, 2 + p.n_mma + 3 * p.n_vdd + p.n_epi), dtype=torch.float64, device=dev)
    N._dev_check(kpts0, kpts1, desc0, desc1, mk0, mk1)
    N._dev_check(n, m, nmatch, dt=torch.int32)
    P = N._ptr
    check(L.einx_pair_metrics_pose(ctypes.byref(p), P(kpts0), P(kpts1), P(desc0), P(desc1), P(n), P(m), P(mk0), P(mk1), P(nmatch), P(d0), P(d1),
                                   P(K0), P(K1), P(T01), P(T10), P(ws), P(out), N._stream(kpts0)), "einx_pair_metrics_pose")
    return out


@on_input_device
def batch_metrics_pose(ev, im, mr, K0, K1, T_0to1, depth=None, T_1to0=None, mma_thr=(1, 3), vdd_thr=(1, 3), epi_thr=(), occlusion_th=None):
    """pair_metrics_pose for a whole EIM.forward_batched result (BatchedFeats x2 + MatchResult; events = view 0, image = view 1),
    depth = (depth0, depth1) or None, no host sync."""
    d0, d1 = depth if depth is not None else (None, None)
    return pair_metrics_pose(ev.det.positions, ev.sparse_desc, ev.det.counts, im.det.positions, im.sparse_desc, im.det.counts, mr.mk0, mr.mk1,
                             mr.nmatch, ev.image_size, im.image_size, K0, K1, T_0to1, T_1to0, d0, d1, mma_thr, vdd_thr, epi_thr, occlusion_th,
                             ordering=ev.ordering)


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


def _check_refine(who, refine, rounds, iters, rounds_name="refine_rounds", iters_name="refine_iters"):
    """the refinement's options: rounds 1..4, iterations 1..50, and neither given without the refinement"""
    for name, v, lo, hi in ((rounds_name, rounds, 1, 4), (iters_name, iters, 1, 50)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"einx: {who}: {name} is an integer of {lo}..{hi}, not {v!r}")
    if not refine and (int(rounds), int(iters)) != (2, 10):
        raise ValueError(f"einx: {who}: {rounds_name} / {iters_name} are options of the refinement: pass refine=True with them")


def _pose_inputs_k(mk0, K0, K1, T_0to1):
    B, dev = mk0.shape[0], mk0.device
    k_f64 = K0.dtype == torch.float64 or K1.dtype == torch.float64
    kdt = torch.float64 if k_f64 else torch.float32
    K0 = K0.to(dev, kdt).reshape(B, 9).contiguous()
    K1 = K1.to(dev, kdt).reshape(B, 9).contiguous()
    T = None if T_0to1 is None else T_0to1.to(dev, torch.float64).reshape(B, 16).contiguous()
    return k_f64, K0, K1, T


@on_input_device
def relative_pose(mk0, mk1, nmatch, K0, K1, T_0to1=None, thresh=1.0, conf=0.999, ordering="yx", max_iters=1000, seed=POSE_SEED, refine=False,
                  refine_rounds=2, refine_iters=10):
    """RANSAC essential matrix + recoverPose + update_one's errors for a batch (csrc/pose.hip), no host sync.
    mk0 / mk1 [B,cap,2|3] float32 and nmatch int32 [B] on the device, K0 / K1 [B,3,3] float32 or float64 (numpy's dtype rules
    follow K's), T_0to1 [B,4,4] or None.  Returns device tensors (R [B,3,3] f64, t [B,3] f64, mask [B,cap] bool,
    status [B] int32, rows [B,4] f64 = R_err, t_err, pose_err, inlier ratio).  refine=True: the pose is then fitted to its inliers
    (refine_relative_pose) and R, t, mask and rows are those of the refinement; status is unchanged."""
    _check_refine("relative_pose", refine, refine_rounds, refine_iters)
    B, dev = mk0.shape[0], mk0.device
    k_f64, K0, K1, T = _pose_inputs_k(mk0, K0, K1, T_0to1)
    L = N.lib()
    p, ws, mask, status, rows = _ransac_call(PoseParams, L.einx_relative_pose_ws_bytes, mk0, mk1, nmatch, thresh, conf, ordering, max_iters,
                                             seed, 4, k_f64=int(k_f64))
    R = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((B, 3), dtype=torch.float64, device=dev)
    check(L.einx_relative_pose(ctypes.byref(p), N._ptr(mk0), N._ptr(mk1), N._ptr(nmatch), N._ptr(K0), N._ptr(K1), N._ptr(T), N._ptr(ws),
                               N._ptr(R), N._ptr(t), N._ptr(mask), N._ptr(status), N._ptr(rows), N._stream(mk0)), "einx_relative_pose")
    if refine:
        R, t, mask, _, rows, _ = refine_relative_pose(mk0, mk1, nmatch, K0, K1, R, t, mask, status, T, thresh, ordering, refine_rounds,
                                                      refine_iters)
        return R, t, mask, status, rows
    return R, t, mask.bool(), status, rows


REFINE_INFO = ("kept", "rounds", "accepted", "last_set")  # the columns of refine_relative_pose's info


@on_input_device
def refine_relative_pose(mk0, mk1, nmatch, K0, K1, R, t, mask, status, T_0to1=None, thresh=1.0, ordering="yx", rounds=2, lm_iters=10):
    """Fits the poses relative_pose returned to their inliers (csrc/pose.hip: pose_refine_kernel), no host sync:
    Levenberg-Marquardt on the Sampson distances over E = [t]x R, `rounds` rounds of inlier selection with at most `lm_iters`
    iterations each.  mk0 ... K1 and thresh / ordering as relative_pose took them; R [B,3,3], t [B,3], mask [B,cap], status [B] as it
    returned them.  Returns device tensors (R, t, mask [B,cap] bool, info [B,4] int32 = REFINE_INFO: kept (1 refined, 0 the input
    pose came back, -1 no pose), rounds run, steps accepted, size of the last round's set; rows [B,4] f64 as relative_pose's, of the
    returned pose; cost [B,2] f64: the mean squared residual over the last round's set before and after it, NaN without a round).
    The refined pose is kept only when its inlier count is not below the input's."""
    _check_refine("refine_relative_pose", True, rounds, lm_iters, "rounds", "lm_iters")
    B, cap, cols = mk0.shape
    dev = mk0.device
    k_f64, K0, K1, T = _pose_inputs_k(mk0, K0, K1, T_0to1)
    N._dev_check(mk0, mk1)
    N._dev_check(nmatch, status, dt=torch.int32)
    R_in = R.to(dev, torch.float64).reshape(B, 9).contiguous()
    t_in = t.to(dev, torch.float64).reshape(B, 3).contiguous()
    mask_in = mask.to(dev, torch.uint8).reshape(B, cap).contiguous()
    p = PoseRefineParams()
    p.struct_size = ctypes.sizeof(PoseRefineParams)
    p.B, p.cap, p.cols, p.kp_yx, p.k_f64, p.rounds, p.lm_iters = B, cap, cols, int(ordering == "yx"), int(k_f64), int(rounds), int(lm_iters)
    p.thresh = float(thresh)
    L = N.lib()
    ws = N._workspace(L.einx_relative_pose_refine_ws_bytes(ctypes.byref(p)), dev)
    R_out = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    t_out = torch.empty((B, 3), dtype=torch.float64, device=dev)
    mask_out = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    rows = torch.empty((B, 4), dtype=torch.float64, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    cost = torch.empty((B, 2), dtype=torch.float64, device=dev)
    P = N._ptr
    check(L.einx_relative_pose_refine(ctypes.byref(p), P(mk0), P(mk1), P(nmatch), P(K0), P(K1), P(R_in), P(t_in), P(mask_in), P(status), P(T),
                                      P(ws), P(R_out), P(t_out), P(mask_out), P(rows), P(info), P(cost), N._stream(mk0)),
          "einx_relative_pose_refine")
    return R_out, t_out, mask_out.bool(), info, rows, cost


@on_input_device
def batch_relative_pose(mr, K0, K1, T_0to1=None, thresh=1.0, conf=0.999, ordering="yx", refine=False, refine_rounds=2, refine_iters=10):
    """relative_pose of an EIM match result (MatchResult: mk0 / mk1 / nmatch), no host sync"""
    if not refine:
        _check_refine("batch_relative_pose", refine, refine_rounds, refine_iters)
        return relative_pose(mr.mk0, mr.mk1, mr.nmatch, K0, K1, T_0to1, thresh, conf, ordering)
    return relative_pose(mr.mk0, mr.mk1, mr.nmatch, K0, K1, T_0to1, thresh, conf, ordering, refine=True, refine_rounds=refine_rounds,
                         refine_iters=refine_iters)


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


ABS_POSE_STATUS = {-1: "few", -2: "none"}  # einx.h: >= 0: 4 * iteration + solution of the chosen model, negative: why there is no pose
ABS_POSE_ROWS = ("R_errs", "t_errs", "t_angles", "inliers", "usable")


@on_input_device
def absolute_pose(mk0, mk1, nmatch, K0, K1, depth0=None, d0=None, valid0=None, T_0to1=None, thresh=8.0, conf=0.99, ordering="yx",
                  max_iters=100, seed=POSE_SEED, refine=True):
    """Metric pose of view 1 in view 0's frame from matches and view 0's depth for a batch (csrc/abs_pose.hip, DESIGN.md 8u: P3P
    RANSAC, an LM refit on the inliers, the pose errors), no host sync.  mk0 / mk1 [B,cap,2|3] float32 and nmatch int32 [B] on the
    device; the depth of view 0 as a map depth0 [B,H,W] (sampled at the keypoints like gt_project does) or per match as d0 [B,cap]
    with valid0 [B,cap]: exactly one of the two; K0 / K1 [B,3,3]; T_0to1 [B,4,4] or None.  The defaults are solvePnPRansac's.
    Returns device tensors (R [B,3,3] f64, t [B,3] f64, mask [B,cap] bool, status [B] int32 (ABS_POSE_STATUS), rows [B,5] f64 =
    R_err (degrees), |t - t_gt|, angle of t against t_gt (degrees), inliers / usable, usable / matches)."""
    if (depth0 is None) == (d0 is None) or (d0 is None) != (valid0 is None):
        raise ValueError("einx: absolute_pose takes view 0's depth either as a map (depth0) or per match (d0 with valid0), not both and not neither")
    B, cap, cols = mk0.shape
    dev = mk0.device
    if cols not in (2, 3):
        raise ValueError("einx: absolute_pose: matched rows have 2 or 3 columns")
    K0, K1 = _f32c(K0, dev, (B, 9)), _f32c(K1, dev, (B, 9))
    T = None if T_0to1 is None else T_0to1.to(dev, torch.float64).reshape(B, 16).contiguous()
    H = W = 0
    dm = dk = vk = None
    if depth0 is not None:
        dm = depth0.to(dev, torch.float32).reshape(B, depth0.shape[-2], depth0.shape[-1]).contiguous()
        H, W = dm.shape[1], dm.shape[2]
    else:
        dk = d0.to(dev, torch.float32).reshape(B, cap).contiguous()
        vk = valid0.to(dev, torch.uint8).reshape(B, cap).contiguous()
    L = N.lib()
    p, ws, mask, status, rows = _ransac_call(AbsPoseParams, L.einx_absolute_pose_ws_bytes, mk0, mk1, nmatch, thresh, conf, ordering, max_iters,
                                             seed, 5, H=H, W=W, refine=int(bool(refine)))
    R = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((B, 3), dtype=torch.float64, device=dev)
    P = N._ptr
    check(L.einx_absolute_pose(ctypes.byref(p), P(mk0), P(mk1), P(nmatch), P(dm), P(dk), P(vk), P(K0), P(K1), P(T), P(ws), P(R), P(t), P(mask),
                               P(status), P(rows), N._stream(mk0)), "einx_absolute_pose")
    return R, t, mask.bool(), status, rows


@on_input_device
def batch_absolute_pose(mr, K0, K1, depth0=None, d0=None, valid0=None, T_0to1=None, thresh=8.0, conf=0.99, ordering="yx"):
    """absolute_pose of an EIM match result (MatchResult: mk0 / mk1 / nmatch), no host sync"""
    return absolute_pose(mr.mk0, mr.mk1, mr.nmatch, K0, K1, depth0, d0, valid0, T_0to1, thresh, conf, ordering)


@on_input_device
def p3p(X, f):
    """the minimal solver alone (test aid): X [n,3,3] points, f [n,3,3] unit bearings, float64 -> (R [n,4,3,3], t [n,4,3],
    n_solutions [n] int32)"""
    n = X.shape[0]
    X = X.to(torch.float64).contiguous()
    f = f.to(X.device, torch.float64).contiguous()
    R = torch.zeros((n, 4, 3, 3), dtype=torch.float64, device=X.device)
    t = torch.zeros((n, 4, 3), dtype=torch.float64, device=X.device)
    ns = torch.empty((n,), dtype=torch.int32, device=X.device)
    check(N.lib().einx_p3p(N._ptr(X), N._ptr(f), n, N._ptr(R), N._ptr(t), N._ptr(ns), N._stream(X)), "einx_p3p")
    return R, t, ns


# ---- ground-truth matches and matcher precision / recall (csrc/gt_matches.hip) ------------------------------------
MATCH_PR_NAMES = ("match_recall", "match_precision", "accuracy", "average_precision")


def _counts(c, B, cap, dev):
    if c is None:
        return torch.full((B,), cap, dtype=torch.int32, device=dev)
    N._dev_check(c, dt=torch.int32)
    return c


def _gt_params(kp0, kp1, ordering, pos_th, neg_th, homography=False, size0=(0, 0), size1=(0, 0)):
    p = GtMatchesParams()
    p.struct_size = ctypes.sizeof(GtMatchesParams)
    p.B, p.cap0, p.cols0 = kp0.shape
    p.cap1, p.cols1 = kp1.shape[1], kp1.shape[2]
    p.kp_yx = int(ordering == "yx")
    p.H0, p.W0, p.H1, p.W1 = int(size0[0]), int(size0[1]), int(size1[0]), int(size1[1])
    p.homography = int(homography)
    p.pos_sq, p.neg_sq = float(pos_th ** 2), float(neg_th ** 2)
    if kp1.shape[0] != p.B:
        raise ValueError("einx: kp0 and kp1 differ in batch size")
    return p


def _f32c(t, dev, shape):
    return t.to(dev, torch.float32).reshape(shape).contiguous()


def _gt_stage_a_outputs(B, cap0, cap1, dev, pose_form=True):
    o = {"proj_0to1": torch.empty((B, cap0, 2), dtype=torch.float32, device=dev),
         "proj_1to0": torch.empty((B, cap1, 2), dtype=torch.float32, device=dev)}
    if pose_form:
        for side, cap in ((0, cap0), (1, cap1)):
            o[f"depth_keypoints{side}"] = torch.empty((B, cap), dtype=torch.float32, device=dev)
            o[f"valid{side}"] = torch.empty((B, cap), dtype=torch.uint8, device=dev)
            o[f"visible{side}"] = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    return o


def _gt_label_outputs(B, cap0, cap1, dev):
    return {"matches0": torch.empty((B, cap0), dtype=torch.int64, device=dev), "matches1": torch.empty((B, cap1), dtype=torch.int64, device=dev),
            "matching_scores0": torch.empty((B, cap0), dtype=torch.float32, device=dev),
            "matching_scores1": torch.empty((B, cap1), dtype=torch.float32, device=dev),
            "pos0": torch.empty((B, cap0), dtype=torch.int32, device=dev)}


def _pose_inputs(B, dev, depth0, depth1, K0, K1, T_0to1, T_1to0, precomputed):
    a = {"K0": _f32c(K0, dev, (B, 9)), "K1": _f32c(K1, dev, (B, 9)), "T01": _f32c(T_0to1, dev, (B, 16)),
         "T10": None if T_1to0 is None else _f32c(T_1to0, dev, (B, 16)), "d0": None, "d1": None, "pre": (None,) * 4, "size0": (0, 0), "size1": (0, 0)}
    if precomputed is not None:
        d0, v0, d1, v1 = precomputed
        a["pre"] = (d0.to(dev, torch.float32).contiguous(), d1.to(dev, torch.float32).contiguous(), v0.to(dev, torch.uint8).contiguous(),
                    v1.to(dev, torch.uint8).contiguous())
    else:
        a["d0"], a["d1"] = (d.to(dev, torch.float32).reshape(B, d.shape[-2], d.shape[-1]).contiguous() for d in (depth0, depth1))
        a["size0"], a["size1"] = a["d0"].shape[1:], a["d1"].shape[1:]
    return a


def _bools(o):
    for k in ("valid0", "valid1", "visible0", "visible1"):
        if k in o:
            o[k] = o[k].bool()
    return o


@on_input_device
def gt_project(kp0, kp1, n, m, depth0, depth1, K0, K1, T_0to1, T_1to0=None, ordering="yx", precomputed=None):
    """stage A, pose form: kp [B,cap,cols>=2] float32, n / m int32 [B] or None (= cap), depth [B,H,W], K [B,3,3], T [B,4,4]
    (T_1to0 None: inverted in the kernel), precomputed = (d0, valid0, d1, valid1) [B,cap] instead of the depth maps.
    Returns proj_0to1 / proj_1to0 [B,cap,2] (x, y), depth_keypoints*, valid*, visible* (bool)."""
    B, dev = kp0.shape[0], kp0.device
    N._dev_check(kp0, kp1)
    n, m = _counts(n, B, kp0.shape[1], dev), _counts(m, B, kp1.shape[1], dev)
    a = _pose_inputs(B, dev, depth0, depth1, K0, K1, T_0to1, T_1to0, precomputed)
    p = _gt_params(kp0, kp1, ordering, 0, 0, False, a["size0"], a["size1"])
    o = _gt_stage_a_outputs(B, p.cap0, p.cap1, dev)
    P = N._ptr
    check(N.lib().einx_gt_project(ctypes.byref(p), P(kp0), P(kp1), P(n), P(m), P(a["d0"]), P(a["d1"]), P(a["K0"]), P(a["K1"]), P(a["T01"]),
                                  P(a["T10"]), *[P(t) for t in a["pre"]], P(o["depth_keypoints0"]), P(o["depth_keypoints1"]), P(o["valid0"]),
                                  P(o["valid1"]), P(o["proj_0to1"]), P(o["proj_1to0"]), P(o["visible0"]), P(o["visible1"]), N._stream(kp0)),
          "einx_gt_project")
    return _bools(o)


@on_input_device
def gt_warp(kp0, kp1, n, m, homography, ordering="xy"):
    """stage A, homography form: H [B,3,3] (or [3,3]) -> proj_0to1 = H kp0, proj_1to0 = H^-1 kp1, [B,cap,2] (x, y)"""
    B, dev = kp0.shape[0], kp0.device
    N._dev_check(kp0, kp1)
    n, m = _counts(n, B, kp0.shape[1], dev), _counts(m, B, kp1.shape[1], dev)
    H = _f32c(homography.expand(B, 3, 3) if homography.dim() == 2 else homography, dev, (B, 9))
    p = _gt_params(kp0, kp1, ordering, 0, 0, True)
    o = _gt_stage_a_outputs(B, p.cap0, p.cap1, dev, pose_form=False)
    check(N.lib().einx_gt_warp(ctypes.byref(p), N._ptr(kp0), N._ptr(kp1), N._ptr(n), N._ptr(m), N._ptr(H), N._ptr(o["proj_0to1"]),
                               N._ptr(o["proj_1to0"]), N._stream(kp0)), "einx_gt_warp")
    return o


@on_input_device
def gt_label(kp0, kp1, n, m, proj_0to1, proj_1to0, visible0=None, visible1=None, valid0=None, valid1=None, pos_th=3, neg_th=5, ordering="yx"):
    """stage B from given projections [B,cap,2] (x, y) and visibility / validity [B,cap] (bool or uint8; None: all true, the
    homography form) -> matches0 / matches1 int64, matching_scores0 / 1 float32, pos0 int32"""
    B, dev = kp0.shape[0], kp0.device
    N._dev_check(kp0, kp1, proj_0to1, proj_1to0)
    n, m = _counts(n, B, kp0.shape[1], dev), _counts(m, B, kp1.shape[1], dev)
    u8 = lambda t: None if t is None else t.to(dev, torch.uint8).contiguous()  # noqa: E731
    vis0, vis1, val0, val1 = u8(visible0), u8(visible1), u8(valid0), u8(valid1)
    p = _gt_params(kp0, kp1, ordering, pos_th, neg_th, visible0 is None)
    L = N.lib()
    ws = N._workspace(L.einx_gt_matches_ws_bytes(ctypes.byref(p)), dev)
    o = _gt_label_outputs(B, p.cap0, p.cap1, dev)
    P = N._ptr
    check(L.einx_gt_label(ctypes.byref(p), P(kp0), P(kp1), P(n), P(m), P(proj_0to1), P(proj_1to0), P(vis0), P(vis1), P(val0), P(val1), P(ws),
                          P(o["matches0"]), P(o["matches1"]), P(o["matching_scores0"]), P(o["matching_scores1"]), P(o["pos0"]), N._stream(kp0)),
          "einx_gt_label")
    return o


@on_input_device
def gt_matches(kp0, kp1, n=None, m=None, depth0=None, depth1=None, K0=None, K1=None, T_0to1=None, T_1to0=None, homography=None, pos_th=3,
               neg_th=5, ordering="yx", precomputed=None):
    """stages A + B in one call (einx_gt_matches), no host sync: the pose form (depth maps or `precomputed` depths, K, T) or, with
    `homography`, the homography form.  kp [B,cap,cols>=2], n / m int32 [B] or None (= cap).  Returns every tensor of gt_project /
    gt_warp and gt_label in one dict."""
    B, dev = kp0.shape[0], kp0.device
    kp0, kp1 = kp0.float().contiguous(), kp1.float().contiguous()
    N._dev_check(kp0, kp1)
    n, m = _counts(n, B, kp0.shape[1], dev), _counts(m, B, kp1.shape[1], dev)
    hom = homography is not None
    if hom:
        a = {"K0": None, "K1": None, "T01": None, "T10": None, "d0": None, "d1": None, "pre": (None,) * 4, "size0": (0, 0), "size1": (0, 0)}
        H = _f32c(homography.expand(B, 3, 3) if homography.dim() == 2 else homography, dev, (B, 9))
    else:
        a = _pose_inputs(B, dev, depth0, depth1, K0, K1, T_0to1, T_1to0, precomputed)
        H = None
    p = _gt_params(kp0, kp1, ordering, pos_th, neg_th, hom, a["size0"], a["size1"])
    L = N.lib()
    ws = N._workspace(L.einx_gt_matches_ws_bytes(ctypes.byref(p)), dev)
    o = _gt_stage_a_outputs(B, p.cap0, p.cap1, dev, pose_form=not hom)
    o.update(_gt_label_outputs(B, p.cap0, p.cap1, dev))
    P = N._ptr
    check(L.einx_gt_matches(ctypes.byref(p), P(kp0), P(kp1), P(n), P(m), P(a["d0"]), P(a["d1"]), P(a["K0"]), P(a["K1"]), P(a["T01"]), P(a["T10"]),
                            *[P(t) for t in a["pre"]], P(H), P(ws), P(o.get("depth_keypoints0")), P(o.get("depth_keypoints1")), P(o.get("valid0")),
                            P(o.get("valid1")), P(o["proj_0to1"]), P(o["proj_1to0"]), P(o.get("visible0")), P(o.get("visible1")), P(o["matches0"]),
                            P(o["matches1"]), P(o["matching_scores0"]), P(o["matching_scores1"]), P(o["pos0"]), N._stream(kp0)), "einx_gt_matches")
    return _bools(o)


def _frame_index(idx, B, F, dev, name):
    """int32 [B] frame indices on the device, or None.  Host-visible indices (a list, numpy, a CPU tensor) are checked against the
    stack here; indices already on the device are not read back: the kernel clamps them to [0, F)."""
    if idx is None:
        if F < B:
            raise ValueError(f"einx: {name} is None (pair b reads frame b), but the stack has {F} frames for {B} pairs")
        return None
    if not (torch.is_tensor(idx) and idx.device.type == "cuda"):
        idx = torch.as_tensor(idx).reshape(-1).to(torch.int64)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= F):
            raise IndexError(f"einx: {name} holds a frame outside [0, {F})")
    idx = idx.to(dev, torch.int32).reshape(-1).contiguous()
    if idx.numel() != B:
        raise ValueError(f"einx: {name} must hold one frame index per pair ({B})")
    return idx


@on_input_device
def gt_matches_dense(depth0, depth1, K0, K1, T_0to1, T_1to0=None, pos_th=3, neg_th=5, idx0=None, idx1=None, labels=True):
    """gt_matches with every pixel centre of both depth maps as a keypoint (einx_gt_dense), no host sync: keypoint
    i = y W + x is (x + 0.5, y + 0.5).  depth0 [F0,H0,W0] / depth1 [F1,H1,W1] float32 on the device; idx0 / idx1 [B] pick each
    pair's frames (None: frame b; host-visible indices are range-checked, device ones are clamped by the kernel), B is that of K0
    [B,3,3].  Returns counts [B,4] int32 = #(matches0 > -1), #(matches1 > -1), #visible0, #visible1 and, with `labels`, every
    O(N) tensor of gt_matches for those keypoints, bit for bit, at (2 pos_th + 3)^2 instead of H W candidates per pixel."""
    pos_sq = float(pos_th) ** 2
    if not (0.0 < pos_sq < float("inf")):
        raise ValueError("einx: pos_th must be finite and > 0")
    dev = depth0.device
    d0, d1 = (d.to(dev, torch.float32).reshape(-1, d.shape[-2], d.shape[-1]).contiguous() for d in (depth0, depth1))
    N._dev_check(d0, d1)
    B = K0.reshape(-1, 9).shape[0]
    p = GtDenseParams()
    p.struct_size = ctypes.sizeof(GtDenseParams)
    p.B, p.F0, p.F1 = B, d0.shape[0], d1.shape[0]
    p.H0, p.W0, p.H1, p.W1 = d0.shape[1], d0.shape[2], d1.shape[1], d1.shape[2]
    p.pos_sq, p.neg_sq = pos_sq, float(neg_th) ** 2
    idx0, idx1 = _frame_index(idx0, B, p.F0, dev, "idx0"), _frame_index(idx1, B, p.F1, dev, "idx1")
    K0, K1, T01 = _f32c(K0, dev, (B, 9)), _f32c(K1, dev, (B, 9)), _f32c(T_0to1, dev, (B, 16))
    T10 = None if T_1to0 is None else _f32c(T_1to0, dev, (B, 16))
    L = N.lib()
    nbytes = L.einx_gt_dense_ws_bytes(ctypes.byref(p))
    if nbytes == 0:
        raise ValueError("einx: gt_matches_dense: bad shape or thresholds")
    ws = N._workspace(nbytes, dev)
    n0, n1 = p.H0 * p.W0, p.H1 * p.W1
    o = {"counts": torch.empty((B, 4), dtype=torch.int32, device=dev)}
    if labels:
        o.update(_gt_stage_a_outputs(B, n0, n1, dev))
        o.update(_gt_label_outputs(B, n0, n1, dev))
        del o["pos0"]
    P = N._ptr
    g = o.get
    check(L.einx_gt_dense(ctypes.byref(p), P(d0), P(d1), P(idx0), P(idx1), P(K0), P(K1), P(T01), P(T10), P(ws), P(g("depth_keypoints0")),
                          P(g("depth_keypoints1")), P(g("valid0")), P(g("valid1")), P(g("proj_0to1")), P(g("proj_1to0")), P(g("visible0")),
                          P(g("visible1")), P(g("matches0")), P(g("matches1")), P(g("matching_scores0")), P(g("matching_scores1")),
                          P(o["counts"]), N._stream(d0)), "einx_gt_dense")
    return _bools(o)


@on_input_device
def batch_gt_matches(ev_batched, im_batched, depth0, depth1, K0, K1, T_0to1, T_1to0=None, pos_th=3, neg_th=5, cc_th=None):
    """gt_matches of the keypoints of an EIM.forward_batched result (BatchedFeats x2: positions [B,cap,3] + counts), no host sync.
    cc_th (a bound on the SQUARED cycle distance; None: off, the calls are those of gt_matches) labels through
    gt_matches_cc: keypoints the other view's depth map says are hidden stop being visible."""
    if cc_th is not None:
        return gt_matches_cc(ev_batched.det.positions, im_batched.det.positions, ev_batched.det.counts, im_batched.det.counts, depth0, depth1,
                             K0, K1, T_0to1, T_1to0, cc_th=cc_th, pos_th=pos_th, neg_th=neg_th, ordering=ev_batched.ordering)
    return gt_matches(ev_batched.det.positions, im_batched.det.positions, ev_batched.det.counts, im_batched.det.counts, depth0, depth1, K0, K1,
                      T_0to1, T_1to0, pos_th=pos_th, neg_th=neg_th, ordering=ev_batched.ordering)


@on_input_device
def match_pr(mr, gt_m0, n=None, scores0=None):
    """matcher_metrics per pair over its first n[b] rows (n None: every row).  `mr`: a MatchResult (its matches0 / scores0 are
    taken) or the matches0 tensor [B,cap] int64 with `scores0` [B,cap] float32 beside it; gt_m0 [B,cap] int64.
    Returns [B,4] float64 = MATCH_PR_NAMES (NaN for a pair without rows)."""
    if isinstance(mr, N.MatchResult):
        mr, scores0 = mr.matches0, mr.scores0
    if scores0 is None:
        raise ValueError("einx: match_pr needs a MatchResult, or matches0 with scores0=")
    B, cap = mr.shape
    dev = mr.device
    if cap == 0:
        return torch.full((B, 4), float("nan"), dtype=torch.float64, device=dev)
    matches0, gt_m0 = mr.to(torch.int64).contiguous(), gt_m0.to(dev, torch.int64).contiguous()
    scores0 = scores0.to(dev, torch.float32).contiguous()
    if gt_m0.shape != matches0.shape or scores0.shape != matches0.shape:
        raise ValueError("einx: matches0, scores0 and gt_m0 must have one shape [B,cap]")
    n = _counts(n, B, cap, dev)
    out = torch.empty((B, 4), dtype=torch.float64, device=dev)
    check(N.lib().einx_match_pr(N._ptr(matches0), N._ptr(scores0), N._ptr(gt_m0), N._ptr(n), B, cap, N._ptr(out), N._stream(matches0)),
          "einx_match_pr")
    return out


# ---- core.geometry.depth / .epipolar on the device (csrc/geometry.hip) --------------------------------------------
def _map3(d, B, dev):
    return None if d is None else d.to(dev, torch.float32).reshape(B, d.shape[-2], d.shape[-1]).contiguous()


def _geom_side(B, dev, kp, count, K, K_other, T, T_other, depth=None, d=None, valid=None, depth_other=None, dj=None, validj=None):
    """one direction of einx_geom_project: the tensors it reads (kept alive by the returned dict) and the ones it writes"""
    N._dev_check(kp)
    cap = kp.shape[1]
    f = lambda t: None if t is None else t.to(dev, torch.float32).reshape(B, cap).contiguous()  # noqa: E731
    u8 = lambda t: None if t is None else t.to(dev, torch.uint8).reshape(B, cap).contiguous()  # noqa: E731
    if (T is None) and (T_other is None):
        raise ValueError("einx: a projection needs the motion of its direction or of the other one")
    if (d is None) != (valid is None) or (dj is None) != (validj is None):
        raise ValueError("einx: given depths come with their validity")
    if d is None and depth is None:
        raise ValueError("einx: a projection needs this view's depth map or the points' depths")
    return {"kp": kp, "count": None if count is None else _counts(count, B, cap, dev), "depth": None if d is not None else _map3(depth, B, dev),
            "d_in": f(d), "valid_in": u8(valid), "depth_other": None if dj is not None else _map3(depth_other, B, dev), "dj_in": f(dj),
            "validj_in": u8(validj), "K": _f32c(K, dev, (B, 9)), "K_other": _f32c(K_other, dev, (B, 9)),
            "T": None if T is None else _f32c(T, dev, (B, 16)), "T_other": None if T_other is None else _f32c(T_other, dev, (B, 16)),
            "d_out": torch.empty((B, cap), dtype=torch.float32, device=dev), "valid_out": torch.empty((B, cap), dtype=torch.uint8, device=dev),
            "proj": torch.empty((B, cap, 2), dtype=torch.float32, device=dev), "visible": torch.empty((B, cap), dtype=torch.uint8, device=dev)}


def _geom_project_sides(sides, cc_bound, ordering):
    """einx_geom_project for one or two prepared sides (one launch); cc_bound None: no cycle check"""
    kp = sides[0]["kp"]
    p = GeomProjectParams()
    p.struct_size = ctypes.sizeof(GeomProjectParams)
    p.B, p.sides, p.kp_yx = kp.shape[0], len(sides), int(ordering == "yx")
    p.cc, p.cc_bound = int(cc_bound is not None), 0.0 if cc_bound is None else float(cc_bound)
    for k, s in enumerate(sides):
        if p.cc and s["depth_other"] is None and s["dj_in"] is None:
            raise ValueError("einx: the cycle check needs the other view's depth map or its depths under the projections")
        c = p.side[k]
        for name in c._ptrs:
            setattr(c, name, N._ptr(s[name]))
        c.cap, c.cols = s["kp"].shape[1], s["kp"].shape[2]
        if s["depth"] is not None:
            c.H, c.W = s["depth"].shape[1:]
        if s["depth_other"] is not None:
            c.Ho, c.Wo = s["depth_other"].shape[1:]
    check(N.lib().einx_geom_project(ctypes.byref(p), N._stream(kp)), "einx_geom_project")


@on_input_device
def geom_project(kp, K_i, K_j, T_itoj=None, T_jtoi=None, depth_i=None, d=None, valid=None, depth_j=None, dj=None, validj=None, count=None,
                 cc_bound=None, ordering="xy"):
    """depth.py's project for one direction (einx_geom_project), no host sync.  kp [B,cap,cols>=2] float32, K [B,3,3],
    T_itoj [B,4,4] (None: the inverse of T_jtoi, taken in the kernel); the points' depths d / valid [B,cap], or depth_i [B,H,W] to
    sample them from; count int32 [B] or None.  cc_bound None: no cycle check.  Otherwise it bounds the SQUARED cycle distance
    (strictly) and needs depth_j [B,Hj,Wj], or dj / validj [B,cap]: the other view's depth under each projection, for a caller that
    samples it its own way between two calls.  Returns proj [B,cap,2] (x, y), visible, depth, valid (bool)."""
    B, dev = kp.shape[0], kp.device
    s = _geom_side(B, dev, kp, count, K_i, K_j, T_itoj, T_jtoi, depth_i, d, valid, depth_j, dj, validj)
    _geom_project_sides([s], cc_bound, ordering)
    return {"proj": s["proj"], "visible": s["visible"].bool(), "depth": s["d_out"], "valid": s["valid_out"].bool()}


@on_input_device
def gt_matches_cc(kp0, kp1, n=None, m=None, depth0=None, depth1=None, K0=None, K1=None, T_0to1=None, T_1to0=None, cc_th=None, pos_th=3,
                  neg_th=5, ordering="yx"):
    """gt_matches (pose form, depth maps) whose visibility also asks the other view's depth map: stage A with the
    cycle check for both sides in one launch (einx_geom_project), then the unchanged stage B (einx_gt_label).  cc_th bounds the
    SQUARED cycle distance in pixels^2, strictly, as the reference's project(ccth=) does (a caller thinking in pixels passes
    th ** 2); None: no check, and every tensor equals gt_matches'.  Returns the same dict as gt_matches."""
    B, dev = kp0.shape[0], kp0.device
    kp0, kp1 = kp0.float().contiguous(), kp1.float().contiguous()
    if kp1.shape[0] != B:
        raise ValueError("einx: kp0 and kp1 differ in batch size")
    if depth0 is None or depth1 is None:
        raise ValueError("einx: gt_matches_cc needs both depth maps")
    n, m = _counts(n, B, kp0.shape[1], dev), _counts(m, B, kp1.shape[1], dev)
    s0 = _geom_side(B, dev, kp0, n, K0, K1, T_0to1, T_1to0, depth=depth0, depth_other=depth1)
    s1 = _geom_side(B, dev, kp1, m, K1, K0, T_1to0, T_0to1, depth=depth1, depth_other=depth0)
    _geom_project_sides([s0, s1], cc_th, ordering)
    o = {"proj_0to1": s0["proj"], "proj_1to0": s1["proj"], "depth_keypoints0": s0["d_out"], "depth_keypoints1": s1["d_out"],
         "valid0": s0["valid_out"], "valid1": s1["valid_out"], "visible0": s0["visible"], "visible1": s1["visible"]}
    o.update(gt_label(kp0, kp1, n, m, o["proj_0to1"], o["proj_1to0"], o["visible0"], o["visible1"], o["valid0"], o["valid1"], pos_th, neg_th,
                      ordering))
    return _bools(o)


@on_input_device
def geom_dense_warp(depth_i, depth_j, K_i, K_j, T_itoj=None, T_jtoi=None, cc_bound=None, both=False):
    """depth.py's dense_warp_consistency on raw tensors (einx_geom_dense_warp), no host sync: every pixel centre of
    depth_i [B,Hi,Wi] at its own depth into view j; cc_bound as geom_project (it needs depth_j [B,Hj,Wj]).  Returns warp
    [B,Hi,Wi,2] (x, y), visible [B,Hi,Wi] bool and counts int32 [B,2] = #(depth > 0), #visible.  With `both`, the other direction
    rides on the same launch: warp1 / visible1 over depth_j's pixels, counts [B,2,2]."""
    dev = depth_i.device
    B = K_i.reshape(-1, 9).shape[0]
    di, dj = _map3(depth_i, B, dev), _map3(depth_j, B, dev)
    N._dev_check(di, dj)
    if (cc_bound is not None or both) and dj is None:
        raise ValueError("einx: the cycle check and the second direction need depth_j")
    if T_itoj is None and T_jtoi is None:
        raise ValueError("einx: a projection needs the motion of its direction or of the other one")
    Ki, Kj = _f32c(K_i, dev, (B, 9)), _f32c(K_j, dev, (B, 9))
    Tij = None if T_itoj is None else _f32c(T_itoj, dev, (B, 16))
    Tji = None if T_jtoi is None else _f32c(T_jtoi, dev, (B, 16))
    p = GeomDenseParams()
    p.struct_size = ctypes.sizeof(GeomDenseParams)
    p.B, p.sides = B, 2 if both else 1
    p.cc, p.cc_bound = int(cc_bound is not None), 0.0 if cc_bound is None else float(cc_bound)
    counts = torch.empty((B, p.sides, 2), dtype=torch.int32, device=dev)
    p.counts = N._ptr(counts)
    out = {}
    keep = []
    for k, (ds, do, Ks, Ko, T, To) in enumerate(((di, dj, Ki, Kj, Tij, Tji), (dj, di, Kj, Ki, Tji, Tij))[:p.sides]):
        warp = torch.empty(ds.shape + (2,), dtype=torch.float32, device=dev)
        vis = torch.empty(ds.shape, dtype=torch.uint8, device=dev)
        c = p.side[k]
        for name, t in zip(c._ptrs, (ds, do, Ks, Ko, T, To, warp, vis)):
            setattr(c, name, N._ptr(t))
        c.H, c.W = ds.shape[1:]
        if do is not None:
            c.Ho, c.Wo = do.shape[1:]
        keep.append((warp, vis))
    check(N.lib().einx_geom_dense_warp(ctypes.byref(p), N._stream(di)), "einx_geom_dense_warp")
    out = {"warp": keep[0][0], "visible": keep[0][1].bool(), "counts": counts if both else counts[:, 0]}
    if both:
        out.update(warp1=keep[1][0], visible1=keep[1][1].bool())
    return out


@on_input_device
def geom_sample(pts, fmap, depth_rule=False):
    """depth.py's sample_fmap (einx_geom_sample): fmap [B,C,H,W] at pts [B,N,2] (x, y) -> [B,N,C] with stage A's depth
    sampler per channel, a hole being a NaN.  depth_rule (C == 1): a hole is <= 0 or NaN as in sample_depth; returns (out, valid
    [B,N] bool)."""
    B, C, H, W = fmap.shape
    dev = fmap.device
    fmap = fmap.to(torch.float32).contiguous()
    pts = pts.to(dev, torch.float32).contiguous()
    N._dev_check(fmap, pts)
    if pts.dim() != 3 or pts.shape[0] != B or pts.shape[2] != 2:
        raise ValueError("einx: pts is [B,N,2] with the map's batch size")
    if depth_rule and C != 1:
        raise ValueError("einx: the depth rule samples one channel")
    n = pts.shape[1]
    out = torch.empty((B, n, C), dtype=torch.float32, device=dev)
    valid = torch.empty((B, n), dtype=torch.uint8, device=dev) if depth_rule else None
    check(N.lib().einx_geom_sample(N._ptr(fmap), B, C, H, W, N._ptr(pts), n, int(depth_rule), N._ptr(out), N._ptr(valid), N._stream(fmap)),
          "einx_geom_sample")
    return (out, valid.bool()) if depth_rule else out


@on_input_device
def epipolar_all(p0, p1, E, eps=1e-15):
    """epipolar.py's sym_epipolar_distance_all (einx_epipolar_all): p0 [B,N,2|3], p1 [B,M,2|3], E [B,3,3] -> [B,N,M]
    float32, no host sync"""
    B, dev = p0.shape[0], p0.device
    p0, p1 = p0.to(torch.float32).contiguous(), p1.to(dev, torch.float32).contiguous()
    N._dev_check(p0, p1)
    if p0.dim() != 3 or p1.dim() != 3 or p1.shape[0] != B or p0.shape[2] not in (2, 3) or p1.shape[2] not in (2, 3):
        raise ValueError("einx: p0 is [B,N,2|3] and p1 [B,M,2|3]")
    E = _f32c(E, dev, (B, 9))
    out = torch.empty((B, p0.shape[1], p1.shape[1]), dtype=torch.float32, device=dev)
    check(N.lib().einx_epipolar_all(N._ptr(p0), p0.shape[2], N._ptr(p1), p1.shape[2], N._ptr(E), B, p0.shape[1], p1.shape[1], float(eps),
                                    N._ptr(out), N._stream(p0)), "einx_epipolar_all")
    return out
