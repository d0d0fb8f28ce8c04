"""Ground-truth matches from depth + pose or from a homography, on the device (csrc/gt_matches.hip).

Drop-in for gt_matches_from_pose_depth / gt_matches_from_homography (reference core/geometry/gt_generation.py:15-224): the same
signatures, defaults and dict keys.  Everything the consumers read is O(N + M) and comes from the kernels; the dense `assignment`
and `reward` are entries of the dict from the start whose values are built with plain torch operators on the device when they are
first read (the FeatsDict pattern of the extractors' dense maps)."""
import torch

from ..._extract import FeatsDict, _Lazy
from ..metrics._native_metrics import gt_matches, gt_matches_dense
from .wrappers import Camera, Pose  # noqa: F401

IGNORE_FEATURE = -2
UNMATCHED_FEATURE = -1


def _empty(kp0, kp1):
    """a pair without keypoints on either side is answered with a TUPLE, not a dict: an all-false assignment [B,N,M] and
    UNMATCHED_FEATURE for every keypoint there is (8e: n == 0 or m == 0)"""
    B, N, M = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    dev = kp0.device
    return (torch.zeros((B, N, M), dtype=torch.bool, device=dev), torch.full((B, N), UNMATCHED_FEATURE, dtype=torch.int64, device=dev),
            torch.full((B, M), UNMATCHED_FEATURE, dtype=torch.int64, device=dev))


def _assignment(pos0, M):
    """8e: `assignment` is a scatter of pos0 (a spare column takes the rows without a positive)"""
    a = torch.zeros(pos0.shape + (M + 1,), dtype=torch.bool, device=pos0.device)
    a.scatter_(-1, torch.where(pos0 >= 0, pos0, pos0.new_tensor(M)).long().unsqueeze(-1), True)
    return a[..., :M]


class _LazyAssignment(_Lazy):
    """the lazy `assignment` entry: besides the function that builds the dense matrix it keeps pos0, which is all that the
    consumers on the device need of it (LightGlue.loss)"""
    __slots__ = ("pos0",)

    def __init__(self, pos0, M):
        super().__init__(lambda d: _assignment(pos0, M))
        self.pos0 = pos0


def lazy_pos0(data, key="assignment"):
    """pos0 [B,N] int32 behind data[key] while that entry is still lazy (the entry stays lazy); None once it is a tensor"""
    v = dict.get(data, key) if isinstance(data, dict) else None
    return v.pos0 if isinstance(v, _LazyAssignment) else None


def prefixed(gt, prefix="gt_"):
    """the dict under the keys the matcher's loss reads (val_matcher.py:82 builds {f"gt_{k}": v} through .items(), which
    resolves the dense entries): the same renaming with the lazy entries kept lazy"""
    out = FeatsDict()
    for k in dict.keys(gt):
        dict.__setitem__(out, prefix + k, dict.__getitem__(gt, k))
    return out


def _sq(a, b):
    """[B,N,M] squared distances of a [B,N,2] to b [B,M,2]: x and y terms squared and added unfused, as stage B does"""
    dx = a[:, :, None, 0] - b[:, None, :, 0]
    dy = a[:, :, None, 1] - b[:, None, :, 1]
    return dx * dx + dy * dy


def _dist(kp0, kp1, p01, p10):
    """8e: dist = max(dist0, dist1), dist0 from (p01, kp1), dist1 from (kp0, p10)"""
    return torch.maximum(_sq(p01, kp1), _sq(kp0, p10))


def _matrix(data):
    return data.to_4x4mat() if isinstance(data, Pose) else data


def _calibration(camera):
    if isinstance(camera, Camera):
        return camera.calibration_matrix()
    if torch.is_tensor(camera) and camera.shape[-2:] == (3, 3):
        return camera
    raise NotImplementedError("einx: camera must be a pinhole core.geometry.wrappers.Camera (no distortion parameters) or K [B,3,3]")


def _pinhole_inverse(K):
    """closed-form inverse of [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]"""
    fx, fy, cx, cy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    z, o = torch.zeros_like(fx), torch.ones_like(fx)
    return torch.stack([1 / fx, z, -cx / fx, z, 1 / fy, -cy / fy, z, z, o], -1).reshape(-1, 3, 3)


def _epipolar(kp0, kp1, K0, K1, T):
    """[B,N,M] symmetric point-to-epipolar-line distance in pixels, mean of the two views, under F = K1^-T [t]x R K0^-1: with
    homogeneous points as rows, l1 = p0 F^T are the lines in view 1, l0 = p1 F those in view 0, e = |l1 p1^T| the algebraic
    residual; each distance is e over the norm of the line's first two coefficients (1e-15 under the root)."""
    R, t = T[:, :3, :3], T[:, :3, 3]
    cross = torch.zeros_like(R)  # [t]x
    cross[:, 0, 1], cross[:, 0, 2], cross[:, 1, 2] = -t[:, 2], t[:, 1], -t[:, 0]
    cross = cross - cross.mT
    F = _pinhole_inverse(K1).mT @ cross @ R @ _pinhole_inverse(K0)
    hom = lambda k: torch.cat([k, torch.ones_like(k[..., :1])], -1)  # noqa: E731
    p0, p1 = hom(kp0), hom(kp1)
    l1, l0 = p0 @ F.mT, p1 @ F
    e = (l1 @ p1.mT).abs()
    n1 = torch.sqrt(l1[..., 0] * l1[..., 0] + l1[..., 1] * l1[..., 1] + 1e-15)[:, :, None]
    n0 = torch.sqrt(l0[..., 0] * l0[..., 0] + l0[..., 1] * l0[..., 1] + 1e-15)[:, None, :]
    return 0.5 * (e / n1 + e / n0)


@torch.no_grad()
def gt_matches_from_pose_depth(kp0, kp1, camera0, camera1, depth0, depth1, T_0to1, T_1to0, pos_th=3, neg_th=5, ordering="yx", epi_th=None,
                               cc_th=None, **kw):
    """kp0 [B,N,2], kp1 [B,M,2], depth [B,H,W], cameras / poses of core.geometry.wrappers (or K [B,3,3] / T [B,4,4] tensors);
    T_1to0 may be None: the kernel inverts T_0to1.  Returns the reference's 12-key dict (int64 matches, float32 scores, bool
    visibility); the tuple (assignment, m0, m1) when N == 0 or M == 0.  epi_th / cc_th are refused (no caller passes them)."""
    if epi_th is not None:
        raise NotImplementedError("einx: gt_matches_from_pose_depth(epi_th=...) is not supported (DESIGN.md 8)")
    if cc_th is not None:
        raise NotImplementedError("einx: gt_matches_from_pose_depth(cc_th=...) is not supported (DESIGN.md 8)")
    if kp0.shape[1] == 0 or kp1.shape[1] == 0:
        return _empty(kp0, kp1)
    K0, K1 = _calibration(camera0), _calibration(camera1)
    T01 = _matrix(T_0to1)
    T10 = None if T_1to0 is None else _matrix(T_1to0)
    pre = None
    if "depth_keypoints0" in kw and "depth_keypoints1" in kw:
        pre = (kw["depth_keypoints0"], kw["valid_depth_keypoints0"], kw["depth_keypoints1"], kw["valid_depth_keypoints1"])
    elif depth0 is None or depth1 is None:
        raise ValueError("einx: gt_matches_from_pose_depth needs depth0 and depth1, or the depth_keypoints* keywords")
    r = gt_matches(kp0, kp1, None, None, depth0, depth1, K0, K1, T01, T10, pos_th=pos_th, neg_th=neg_th, ordering=ordering, precomputed=pre)
    M = kp1.shape[1]
    cols = [1, 0] if ordering == "yx" else [0, 1]

    def reward(d):
        x0, x1 = kp0[..., cols].float(), kp1[..., cols].float()
        dist = _dist(x0, x1, d["proj_0to1"], d["proj_1to0"])
        dist = torch.where(d["visible0"].unsqueeze(-1) & d["visible1"].unsqueeze(-2), dist, dist.new_tensor(float("inf")))
        epi = _epipolar(x0, x1, K0.float().reshape(-1, 3, 3), K1.float().reshape(-1, 3, 3), T01.float().reshape(-1, 4, 4))
        return (dist < pos_th ** 2).float() - (epi > neg_th).float()

    out = FeatsDict()
    out.update({
        "assignment": _LazyAssignment(r["pos0"], M),
        "reward": _Lazy(reward),
        "matches0": r["matches0"], "matches1": r["matches1"],
        "matching_scores0": r["matching_scores0"], "matching_scores1": r["matching_scores1"],
        "depth_keypoints0": r["depth_keypoints0"], "depth_keypoints1": r["depth_keypoints1"],
        "proj_0to1": r["proj_0to1"], "proj_1to0": r["proj_1to0"],
        "visible0": r["visible0"], "visible1": r["visible1"],
    })
    return out


@torch.no_grad()
def gt_matches_from_homography(kp0, kp1, H, pos_th=3, neg_th=6, **kw):
    """kp0 [B,N,2], kp1 [B,M,2] in (x, y), H [B,3,3] or [3,3].  Returns the reference's 8-key dict; the tuple for N == 0 or M == 0."""
    if kp0.shape[1] == 0 or kp1.shape[1] == 0:
        return _empty(kp0, kp1)
    r = gt_matches(kp0, kp1, None, None, homography=H, pos_th=pos_th, neg_th=neg_th, ordering="xy")
    M = kp1.shape[1]

    def reward(d):
        dist = _dist(kp0[..., :2].float(), kp1[..., :2].float(), d["proj_0to1"], d["proj_1to0"])
        return (dist < pos_th ** 2).float() - (dist > neg_th ** 2).float()

    out = FeatsDict()
    out.update({
        "assignment": _LazyAssignment(r["pos0"], M),
        "reward": _Lazy(reward),
        "matches0": r["matches0"], "matches1": r["matches1"],
        "matching_scores0": r["matching_scores0"], "matching_scores1": r["matching_scores1"],
        "proj_0to1": r["proj_0to1"], "proj_1to0": r["proj_1to0"],
    })
    return out


DENSE_GRID_KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1", "depth_keypoints0", "depth_keypoints1", "proj_0to1",
                   "proj_1to0", "visible0", "visible1")


def valid_ratio(counts):
    """check_indices' ratio from einx_gt_dense's counts [B,4]: #(matches0 > -1) / min(#visible0, #visible1) in float32; 0 / 0 is NaN"""
    c = counts.to(torch.float32)
    return c[:, 0] / torch.minimum(c[:, 2], c[:, 3])


@torch.no_grad()
def gt_matches_dense_grid(camera0, camera1, depth0, depth1, T_0to1, T_1to0=None, pos_th=3, neg_th=5):
    """gt_matches_from_pose_depth with every pixel centre of both depth maps as a keypoint (the call of the reference's
    datasets/generate_MVSEC_relative_pose_val.py:250-259): kp = grid + 0.5 in raster order, ordering "yx".  depth [B,H,W] per side
    (the sides may differ in size and intrinsics).  Returns the ten O(N) keys of the 12-key dict with its dtypes -- equal, bit for
    bit, to gt_matches_from_pose_depth on those keypoints -- plus num_matches0 / num_matches1 / num_visible0 / num_visible1 (int32
    [B]) and valid_ratio (float32 [B]).  The dense `assignment` / `reward` are not offered."""
    K0, K1 = _calibration(camera0), _calibration(camera1)
    T10 = None if T_1to0 is None else _matrix(T_1to0)
    r = gt_matches_dense(depth0, depth1, K0, K1, _matrix(T_0to1), T10, pos_th=pos_th, neg_th=neg_th)
    out = {k: r[k] for k in DENSE_GRID_KEYS}
    c = r["counts"]
    out.update(num_matches0=c[:, 0], num_matches1=c[:, 1], num_visible0=c[:, 2], num_visible1=c[:, 3], valid_ratio=valid_ratio(c))
    return out
