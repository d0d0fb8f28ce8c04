"""Rectification of raw recordings on the device: what the reference's two preparation scripts do on the host with
OpenCV and numpy before any of its dataset classes can run.

    datasets/MVSEC_rectify.py   cv.fisheye.initUndistortRectifyMap (:91-106)     fisheye_rectify_map
                                cv.remap per frame (:16-21)                     remap
                                map lookup per event + bounds filter (:23-45)   rectify_events(..., rule="mvsec")
    datasets/rectify_ec.py      cv.undistort per frame (:48-50)                 remap with radtan_rectify_map(K, D, size)
                                cv.undistortPoints + rint per event (:70-78)    radtan_undistort_points_map (one evaluation per PIXEL)
                                bounds filter (:80-83)                          rectify_events(..., rule="ec")

Maps are pairs of [H, W] float32 tensors on the device.  The definitions are those of include/einx.h; two of them depart from
OpenCV on purpose: `remap` interpolates at the map's own coordinate (OpenCV first quantises it to 1/32 px), and `rectify_events`
refuses a raw coordinate outside the map (numpy raises for one >= W and WRAPS a negative one).  Agreement with OpenCV itself has
not been measured: the tests compare with a float64 restatement of the same definitions."""
import numpy as np
import torch

from .. import _native as N
from .sequence import EventSequence

RULES = ("mvsec", "ec")


def _intrinsics(K):
    """(fx, fy, cx, cy) from a 3x3 camera matrix or from the four values"""
    k = np.asarray(K, np.float64)
    if k.shape == (3, 3):
        return np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if k.shape == (4,):
        return k
    raise ValueError(f"rectify: K must be a 3x3 matrix or (fx, fy, cx, cy), got shape {k.shape}")


def _matrix3(M, what, allow_3x4=False):
    m = np.asarray(M, np.float64)
    if m.shape == (3, 3) or (allow_3x4 and m.shape == (3, 4)):
        return np.ascontiguousarray(m[:, :3])
    raise ValueError(f"rectify: {what} must be 3x3{' or 3x4' if allow_3x4 else ''}, got shape {m.shape}")


def _coeffs(D, n):
    d = np.asarray(D, np.float64).reshape(-1)
    if d.size != n:
        raise ValueError(f"rectify: D must hold {n} distortion coefficients, got {d.size}")
    return d


def _size(size):
    try:
        W, H = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"rectify: size must be (W, H), got {size!r}") from None
    if W <= 0 or H <= 0:
        raise ValueError(f"rectify: size must be positive, got {(W, H)}")
    return W, H


def _camera_matrix(k):
    return np.array([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])


def fisheye_rectify_map(K, D, R, P, size, device="cuda"):
    """cv.fisheye.initUndistortRectifyMap(K, D, R, P, size, CV_32FC1) (datasets/MVSEC_rectify.py:91-106): (map_x, map_y), where a
    pixel of the rectified frame lies in the raw one.  K: 3x3 or (fx, fy, cx, cy); D: (k1, k2, k3, k4); R: 3x3; P: 3x3 or 3x4;
    size: (W, H), as the calibration files give it."""
    k, d, r, p = _intrinsics(K), _coeffs(D, 4), _matrix3(R, "R"), _matrix3(P, "P", True)
    W, H = _size(size)
    return N.rectify_map("fisheye", k, d, r, p, H, W, device)


def radtan_rectify_map(K, D, size, R=None, P=None, device="cuda"):
    """cv.initUndistortRectifyMap(K, D, R, P, size, CV_32FC1) for the radial-tangential model, D = (k1, k2, p1, p2, k3) in the
    order of EC's calib.txt.  R = None: the identity; P = None: K -- the map cv.undistort(img, K, D) samples with
    (datasets/rectify_ec.py:48-50)."""
    k, d = _intrinsics(K), _coeffs(D, 5)
    r = np.eye(3) if R is None else _matrix3(R, "R")
    p = _camera_matrix(k) if P is None else _matrix3(P, "P", True)
    W, H = _size(size)
    return N.rectify_map("radtan", k, d, r, p, H, W, device)


def radtan_undistort_points_map(K, D, size, P=None, iters=5, rint=True, device="cuda"):
    """cv.undistortPoints(pixel, K, D, P=P) evaluated once for every integer pixel of the sensor (datasets/rectify_ec.py:70-78):
    (map_x, map_y), where a raw pixel lies after undistortion -- the event-side map rectify_events reads.  P = None: K, the
    reference's call.  iters: fixed-point iterations (5: the call's default criteria); rint: store np.rint of the result (:78)."""
    k, d = _intrinsics(K), _coeffs(D, 5)
    p = _camera_matrix(k) if P is None else _matrix3(P, "P", True)
    W, H = _size(size)
    if int(iters) < 0:
        raise ValueError(f"rectify: iters must not be negative, got {iters}")
    return N.rectify_map("points", k, d, None, p, H, W, device, iters=int(iters), round_out=bool(rint))


def _check_maps(map_x, map_y):
    if not (torch.is_tensor(map_x) and torch.is_tensor(map_y)):
        raise ValueError("rectify: map_x and map_y must be tensors (the map builders return them)")
    if map_x.dim() != 2 or map_x.shape != map_y.shape or map_x.numel() == 0:
        raise ValueError(f"rectify: map_x and map_y must be two [H, W] maps of one shape, got {tuple(map_x.shape)} and {tuple(map_y.shape)}")
    if map_x.dtype != torch.float32 or map_y.dtype != torch.float32:
        raise ValueError(f"rectify: maps must be float32, got {map_x.dtype} and {map_y.dtype}")
    if map_x.device != map_y.device:
        raise ValueError(f"rectify: map_x lies on {map_x.device}, map_y on {map_y.device}")
    return map_x.contiguous(), map_y.contiguous()


def remap(images, map_x, map_y):
    """cv.remap(frame, map_x, map_y, cv.INTER_LINEAR) for every frame in one launch (datasets/MVSEC_rectify.py:16-21; with
    radtan_rectify_map: cv.undistort, datasets/rectify_ec.py:48-50).  images: [F, Hs, Ws] or [Hs, Ws], uint8 or float32; a numpy
    array is uploaded to the maps' device, a tensor must lie there already and is used as it is (a non-contiguous one is copied
    once).  Returns [F, H, W] (or [H, W]) of the same type on the device.  Bilinear at the map's own coordinate, taps outside the
    source read 0, a map entry that is not finite gives 0 (include/einx.h: einx_remap_bilinear)."""
    map_x, map_y = _check_maps(map_x, map_y)
    if isinstance(images, np.ndarray):
        if images.dtype not in (np.uint8, np.float32):
            raise ValueError(f"rectify: frames must be uint8 or float32, got {images.dtype}")
        src = torch.from_numpy(np.ascontiguousarray(images))
        if src.dim() not in (2, 3):
            raise ValueError(f"rectify: frames must be [F, Hs, Ws] or [Hs, Ws], got {tuple(src.shape)}")
        src = src.to(map_x.device)
    elif torch.is_tensor(images):
        src = images
        if src.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"rectify: frames must be uint8 or float32, got {src.dtype}")
        if src.dim() not in (2, 3):
            raise ValueError(f"rectify: frames must be [F, Hs, Ws] or [Hs, Ws], got {tuple(src.shape)}")
        if src.device != map_x.device:
            raise ValueError(f"rectify: the frames lie on {src.device}, the maps on {map_x.device}")
    else:
        raise ValueError(f"rectify: frames must be a numpy array or a tensor, got {type(images).__name__}")
    if src.shape[-1] * src.shape[-2] == 0:
        raise ValueError(f"rectify: empty frames {tuple(src.shape)}")
    single = src.dim() == 2
    out = N.remap_bilinear((src[None] if single else src).contiguous(), map_x, map_y)
    return out[0] if single else out


def _bounds(rule, H, W):
    if isinstance(rule, str):
        if rule == "mvsec":  # MVSEC_rectify.py:37-43
            return float(W - 1), float(H - 1)
        if rule == "ec":  # rectify_ec.py:80-83
            return float(W), float(H)
        raise ValueError(f"rectify: rule must be one of {RULES} or (x_hi, y_hi), got {rule!r}")
    try:
        x_hi, y_hi = (float(v) for v in rule)
    except (TypeError, ValueError):
        raise ValueError(f"rectify: rule must be one of {RULES} or (x_hi, y_hi), got {rule!r}") from None
    return x_hi, y_hi


class RectifiedSequence(EventSequence):
    """the EventSequence rectify_events returns: `kept` events of the raw stream remain, `dropped` left the bounds"""
    kept = 0
    dropped = 0


def rectify_events(events, map_x, map_y, rule):
    """Rectify a whole event stream on the device (datasets/MVSEC_rectify.py:23-45; datasets/rectify_ec.py:70-83 with the map of
    radtan_undistort_points_map): event k moves to (map_x[oy, ox], map_y[oy, ox]) with ox = np.round(x[k]), oy = np.round(y[k])
    and stays iff 0 <= x' < x_hi and 0 <= y' < y_hi; t and p are copied.  The kept events keep their order, so the result is a
    time-sorted EventSequence again (with `.kept` and `.dropped`), ready for `.windows(...)`.

    events: an EventSequence (nothing of the stream leaves the device but the kept stamps, which `windows` searches on the host:
    ONE read-back that also brings the two counts) or the reference's dict of numpy arrays (uploaded once, to the maps' device).
    rule: "mvsec" (x_hi, y_hi = W - 1, H - 1), "ec" (W, H) or an explicit (x_hi, y_hi); [H, W] is the maps' shape.

    Cost: the number kept is only known on the device, so the one read-back brings all 2 + N eight-byte words, the unused tail
    behind the kept stamps included: its time follows N, not the number kept (140 ms for 10^8 events, of which the kernels are
    2.4 ms).  The result's x / y / t / p are views of the N-sized output buffers and keep those alive; `.clone()` them to give
    the tails back.

    IndexError: some raw coordinate rounds to a pixel outside the map or is not finite.  numpy raises for a coordinate >= W
    too, but WRAPS a negative one to the other side of the map; here both are refused, with the number of such events."""
    map_x, map_y = _check_maps(map_x, map_y)
    H, W = (int(v) for v in map_x.shape)
    x_hi, y_hi = _bounds(rule, H, W)
    if isinstance(events, EventSequence):
        seq = events
        if seq.t.device != map_x.device:  # (the arrays' device: `seq.device` may be an un-indexed "cuda", a map's never is)
            raise ValueError(f"rectify: the event sequence lies on {seq.t.device}, the maps on {map_x.device}")
    elif isinstance(events, dict):
        seq = EventSequence(events, device=map_x.device)
    else:
        raise ValueError(f"rectify: events must be an EventSequence or a dict of numpy arrays, got {type(events).__name__}")
    ox, oy, ot, op, head = N.events_remap(seq.x, seq.y, seq.t, seq.p, map_x, map_y, x_hi, y_hi)
    host = head.cpu().numpy()  # the one read-back: (kept, out of map) and the stamps behind them
    kept, outside = int(host[0]), int(host[1])
    if outside != 0:
        raise IndexError(f"rectify_events: {outside} of {len(seq)} events have a raw coordinate outside the {H} x {W} map (or not finite)")
    # a subsequence of sorted stamps is sorted: nothing to check again
    out = RectifiedSequence._from_parts(ox[:kept], oy[:kept], ot[:kept], op[:kept], host[2:2 + kept].view(np.float64), check=False)
    out.kept, out.dropped = kept, len(seq) - kept
    return out
