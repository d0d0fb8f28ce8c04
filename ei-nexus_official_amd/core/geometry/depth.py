"""Depth sampling, projection between two views and the dense warp with its cycle-consistency check, on the device
(csrc/geometry.hip).

Drop-in for reference core/geometry/depth.py:9-89: the same names, signatures and defaults; every function below is one kernel
launch (two for a caller-supplied sampler) and nothing synchronises with the host.  Cameras and poses are those of
core.geometry.wrappers (or K [B,3,3] / T [B,4,4] tensors).

The quirk kept from the reference: `ccth` is compared with the SQUARED cycle distance (pixels^2) although it reads like pixels;
it is passed through as given."""
import torch

from ..metrics._native_metrics import geom_dense_warp, geom_project, geom_sample
from .gt_generation import _calibration, _matrix
from .wrappers import Camera, Pose  # noqa: F401


def sample_fmap(pts, fmap):
    """fmap [B,C,H,W] at pts [B,N,2] (x, y in pixels, pixel centres at .5) -> [B,N,C]: bilinear with zero padding; where a NaN sits
    under a tap that counts, the nearest pixel instead"""
    return geom_sample(pts, fmap)


def sample_depth(pts, depth_):
    """depth_ [B,H,W] at pts [B,N,2] -> (depth [B,N], valid [B,N]): sample_fmap on the map with everything <= 0 made a hole;
    valid = not NaN and > 0"""
    out, valid = geom_sample(pts, depth_[:, None], depth_rule=True)
    return out[..., 0], valid


def sample_normals_from_depth(pts, depth, K):
    raise NotImplementedError("einx: sample_normals_from_depth needs kornia (kornia.geometry.depth.depth_to_normals), which this "
                              "package does not depend on")


def _batched(t, B, tail):
    t = t.reshape((-1,) + tail)
    return t.expand((B,) + tail) if t.shape[0] != B else t


def project(kpi, di, depthj, camera_i, camera_j, T_itoj, validi, ccth=None, sample_depth_fun=sample_depth, sample_depth_kwargs=None):
    """kpi [B,N,2] (x, y) with depths di [B,N] and validity validi [B,N], seen from view j -> (kpi_j [B,N,2], visible [B,N]).
    visible = validi, in front of and inside camera j.  With depthj [B,Hj,Wj] AND ccth (either None: no check) also the cycle
    check: depthj sampled at kpi_j must be valid, the way back through T_itoj.inv() must end in front of and inside camera i, and
    |kpi - back|^2 < ccth, strictly.  A sampler other than sample_depth runs between two launches."""
    B = di.shape[0]
    kp = _batched(kpi.float(), B, tuple(kpi.shape[-2:])).contiguous()
    Ki, Kj = _batched(_calibration(camera_i), B, (3, 3)), _batched(_calibration(camera_j), B, (3, 3))
    T = _batched(_matrix(T_itoj), B, (4, 4))
    if depthj is None or ccth is None:
        r = geom_project(kp, Ki, Kj, T, d=di, valid=validi)
    elif sample_depth_fun is sample_depth and not sample_depth_kwargs:
        r = geom_project(kp, Ki, Kj, T, d=di, valid=validi, depth_j=depthj, cc_bound=ccth)
    else:
        first = geom_project(kp, Ki, Kj, T, d=di, valid=validi)
        dj, validj = sample_depth_fun(first["proj"], depthj, **(sample_depth_kwargs or {}))
        r = geom_project(kp, Ki, Kj, T, d=di, valid=validi, dj=dj, validj=validj, cc_bound=ccth)
    return r["proj"], r["visible"]


def dense_warp_consistency(depthi, depthj, T_itoj, camerai, cameraj, **kwargs):
    """every pixel centre of depthi [B,Hi,Wi], at the pixel's own depth, seen from view j -> (warp [B,Hi,Wi,2], visible shaped
    like depthj [B,Hj,Wj]); kwargs are project's (ccth, sample_depth_fun, sample_depth_kwargs).  As in the reference the
    visibility is reshaped with depthj's size, so both maps must hold the same number of pixels."""
    if depthj is None:
        raise ValueError("einx: dense_warp_consistency needs depthj (its shape is the visibility map's)")
    unknown = set(kwargs) - {"ccth", "sample_depth_fun", "sample_depth_kwargs"}
    if unknown:
        raise TypeError(f"project() got an unexpected keyword argument {sorted(unknown)[0]!r}")
    Hi, Wi = depthi.shape[-2:]
    Hj, Wj = depthj.shape[-2:]
    if Hi * Wi != Hj * Wj:
        raise RuntimeError(f"einx: dense_warp_consistency shapes the visibility of depthi's {Hi}x{Wi} pixels like depthj ({Hj}x{Wj}): "
                           "both maps must hold the same number of pixels")
    B = depthi.reshape(-1, Hi, Wi).shape[0]
    if kwargs.get("sample_depth_fun", sample_depth) is not sample_depth or kwargs.get("sample_depth_kwargs"):
        from .utils import get_image_coords
        di = depthi.reshape(B, Hi * Wi)
        warp, vis = project(get_image_coords(depthi).reshape(1, Hi * Wi, 2), di, depthj, camerai, cameraj, T_itoj, di > 0, **kwargs)
    else:
        r = geom_dense_warp(depthi, depthj, _batched(_calibration(camerai), B, (3, 3)), _batched(_calibration(cameraj), B, (3, 3)),
                            _batched(_matrix(T_itoj), B, (4, 4)), cc_bound=kwargs.get("ccth"))
        warp, vis = r["warp"], r["visible"]
    return warp.reshape(B, Hi, Wi, 2), vis.reshape(B, Hj, Wj)
