"""A recording's pose track on the device: the reference's datasets/Interpolator.py::PoseInterpolator, which its
datasets call on the host for every view of every sample (datasets/MVSEC.py:795, datasets/EC.py:264-289,
generate_MVSEC_relative_pose_val.py:232-234), plus the two host steps around it:

    PoseInterpolator(timestamp, t, R, quat_R)        PoseTrack(timestamps, t, R, quat_R)      one upload
    interpolator.interpolate(t) per query            track.interpolate(ts)                    one launch for all queries
    get_relative_pose, twice per pair (:818-830)     track.relative(ts0, ts1)                 one launch for all pairs
    |outer difference|.argmin (:364-366)             nearest_index(stamps, queries)           no F x Q matrix

The definitions are those of include/einx.h (einx_pose_interp, einx_pose_relative, einx_nearest_stamp): float64 throughout, the
knot interval and the translation in scipy's order of operations, the rotation by quaternion slerp on the shorter arc.  Two
departures from the reference, both on purpose: the relative transforms are formed in float64 with the closed-form rigid inverse
and cast to float32 once (the rule of datasets/pairs.py; the reference multiplies float32 casts through np.linalg.inv, which can
differ in the last float32 bit), and of a query outside the track only interp1d's ValueError is reproduced, not the line the
reference prints before it.  scipy is not needed."""
import numpy as np
import torch

from .. import _native as N


def _nearest_rotations(M):
    """[N,3,3] float64 -> the nearest rotation of every matrix: the polar factor U V^T of its SVD, with the determinant fixed
    (what scipy's Rotation.from_matrix computes for a matrix that is not orthogonal)"""
    U, _, Vt = np.linalg.svd(M)
    R = U @ Vt
    flip = np.linalg.det(R) < 0
    U[flip, :, 2] *= -1.0
    R[flip] = U[flip] @ Vt[flip]
    return R


def _quats_from_rotations(R):
    """[N,3,3] -> [N,4] unit quaternions (x, y, z, w), each from the largest of (m00, m11, m22, trace): the choice that divides by
    the largest component"""
    n = R.shape[0]
    dec = np.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2], (R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]], 1)
    choice = dec.argmax(1)
    q = np.empty((n, 4))
    rows = np.arange(n)
    for c in range(3):
        s = rows[choice == c]
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[s, i] = 1.0 - dec[s, 3] + 2.0 * R[s, i, i]
        q[s, j] = R[s, j, i] + R[s, i, j]
        q[s, k] = R[s, k, i] + R[s, i, k]
        q[s, 3] = R[s, k, j] - R[s, j, k]
    s = rows[choice == 3]
    q[s, 0] = R[s, 2, 1] - R[s, 1, 2]
    q[s, 1] = R[s, 0, 2] - R[s, 2, 0]
    q[s, 2] = R[s, 1, 0] - R[s, 0, 1]
    q[s, 3] = 1.0 + dec[s, 3]
    return q / np.sqrt((q * q).sum(1, keepdims=True))


class PoseTrack:
    """PoseInterpolator(timestamp, t, R, quat_R, mode="linear") with its knots resident on `device`.  timestamps [N]; t [N,3]; R
    [N,3,3] rotation matrices, or [N,4] quaternions (x, y, z, w) with quat_R=True (the reference's default is True; its datasets
    pass matrices).  Only the linear mode exists.

    Construction runs once on the host in float64: every matrix knot is replaced by its nearest rotation and turned into a unit
    quaternion, quaternion knots are normalised; then stamps, translations and quaternions are uploaded, once.  ValueError, as scipy
    raises: fewer than two knots, stamps that are not strictly increasing, a NaN anywhere, a zero quaternion, shapes that do not
    match.

    `out_of_range`: the device counter (int32 [1]) of the last interpolate / relative call."""

    def __init__(self, timestamps, t, R, quat_R=False, device="cuda"):
        ts = np.asarray(timestamps, np.float64)
        p = np.asarray(t, np.float64)
        r = np.asarray(R, np.float64)
        if ts.ndim != 1:
            raise ValueError(f"PoseTrack: timestamps must be [N], got shape {ts.shape}")
        n = ts.shape[0]
        if p.shape != (n, 3):
            raise ValueError(f"PoseTrack: t must be [N,3] with N = {n} stamps, got shape {p.shape}")
        want = (n, 4) if quat_R else (n, 3, 3)
        if r.shape != want:
            raise ValueError(f"PoseTrack: R must be {'[N,4] quaternions' if quat_R else '[N,3,3] matrices'} with N = {n} stamps, got shape "
                             f"{r.shape}")
        if n < 2:
            raise ValueError(f"PoseTrack: at least 2 knots are needed to interpolate, got {n}")
        if np.isnan(ts).any() or np.isnan(p).any() or np.isnan(r).any():
            raise ValueError("PoseTrack: timestamps, t or R contain a NaN")
        if not (ts[1:] > ts[:-1]).all():
            k = int(np.argmin(ts[1:] > ts[:-1]))
            raise ValueError(f"PoseTrack: timestamps must be strictly increasing (timestamps[{k + 1}] <= timestamps[{k}])")
        if quat_R:
            norm = np.sqrt((r * r).sum(1, keepdims=True))
            if (norm == 0.0).any():
                raise ValueError("PoseTrack: found a zero-norm quaternion")
            q = r / norm
        else:
            q = _quats_from_rotations(_nearest_rotations(r))
        self.device = torch.device(device)
        self.t_host = ts.copy()  # the range host queries are checked against
        self.stamps, self.trans, self.quats = (torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (ts, p, q))
        self.out_of_range = None

    def __len__(self):
        return int(self.t_host.shape[0])

    @property
    def range(self):
        return float(self.t_host[0]), float(self.t_host[-1])

    def _queries(self, ts):
        """(queries [Q] float64 on the device, whether `ts` was a single number).  A device tensor is used as it is, without a look
        at its values; anything else is checked against the track's range on the host first."""
        if torch.is_tensor(ts) and ts.device.type == "cuda":
            if ts.device != self.stamps.device:
                raise ValueError(f"PoseTrack: the queries lie on {ts.device}, the track on {self.stamps.device}")
            return ts.detach().to(torch.float64).reshape(-1).contiguous(), ts.dim() == 0
        a = np.asarray(ts.detach().numpy() if torch.is_tensor(ts) else ts, np.float64)
        lo, hi = self.t_host[0], self.t_host[-1]
        flat = a.reshape(-1)
        if np.isnan(flat).any():
            raise ValueError(f"A value (nan) in x_new is not a number; the interpolation range is [{lo}, {hi}].")
        if (flat < lo).any():  # interp1d's messages (scipy/interpolate/_interpolate.py: _check_bounds)
            raise ValueError(f"A value ({flat[flat < lo][0]}) in x_new is below the interpolation range's minimum value ({lo}).")
        if (flat > hi).any():
            raise ValueError(f"A value ({flat[flat > hi][0]}) in x_new is above the interpolation range's maximum value ({hi}).")
        return torch.from_numpy(np.ascontiguousarray(flat)).to(self.stamps.device), a.ndim == 0

    def interpolate(self, ts, dtype=torch.float32, inverse=True):
        """PoseInterpolator.interpolate for every query at once: [Q,4,4] of `dtype` (float32 or float64) on the device ([4,4] for a
        single number).  inverse=True (default): T_j_W, what the reference returns; False: T_W_j.

        ts on the host (a number, a list, a numpy array, a CPU tensor): a value outside the track raises ValueError before anything
        is launched, in the words of interp1d's error.  ts as a device tensor: no host synchronisation; the rows of queries outside
        the track (or NaN) are all NaN, and `out_of_range` counts them on the device."""
        q, single = self._queries(ts)
        out, self.out_of_range = N.pose_interp(self.stamps, self.trans, self.quats, q, inverse=inverse, dtype=dtype)
        return out[0] if single else out

    def relative(self, ts0, ts1):
        """(T_0to1, T_1to0), [P,4,4] float32 each: T_0to1 = T_1_W T_W_0 between the poses at ts0[k] and ts1[k], formed in float64 with
        the closed-form rigid inverse and cast once (MVSEC.py:1081-1085 in the rule of datasets/pairs.py).  Queries as in
        `interpolate`; with device tensors a pair with a query outside the track has NaN in both matrices."""
        q0, s0 = self._queries(ts0)
        q1, s1 = self._queries(ts1)
        if q0.numel() != q1.numel():
            raise ValueError(f"PoseTrack: relative takes as many ts0 as ts1, got {q0.numel()} and {q1.numel()}")
        t01, t10, self.out_of_range = N.pose_relative(self.stamps, self.trans, self.quats, q0, q1)
        return (t01[0], t10[0]) if s0 and s1 else (t01, t10)


def nearest_index(stamps, queries, device="cuda"):
    """np.abs(np.subtract.outer(stamps, queries)).argmin(axis=0) (datasets/MVSEC.py:364-366) on the device without the F x Q matrix:
    int64 [Q], the FIRST index whose |stamps[i] - query| (in float64) is minimal.  stamps must be sorted (non-decreasing; equal
    stamps are fine).  Host arrays are checked (ValueError: no stamps, a NaN stamp, stamps that decrease) and uploaded to `device`;
    device tensors are used as they are."""
    def put(a, what, check):
        if torch.is_tensor(a) and a.device.type == "cuda":
            return a.detach().to(torch.float64).reshape(-1).contiguous()
        h = np.asarray(a.detach().numpy() if torch.is_tensor(a) else a, np.float64).reshape(-1)
        if check:
            if np.isnan(h).any():
                raise ValueError(f"nearest_index: {what} contain a NaN")
            if (h[1:] < h[:-1]).any():
                raise ValueError(f"nearest_index: {what} must be sorted")
        return torch.from_numpy(np.ascontiguousarray(h)).to(device)

    s = put(stamps, "stamps", True)
    if s.numel() == 0:
        raise ValueError("nearest_index: no stamps")
    q = put(queries, "queries", False)
    if q.device != s.device:
        raise ValueError(f"nearest_index: the stamps lie on {s.device}, the queries on {q.device}")
    return N.nearest_stamp(s, q)
