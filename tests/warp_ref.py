"""Yardstick of the perspective warp (include/einx.h: einx_warp_perspective) and the cases both warp test modules use.

The source point of every destination pixel is computed here in numpy float64 in the documented order (numpy rounds every
elementwise operation as it is written), from the same H^-1 the package forms (datasets.warp.invert_homography on the host).
Values are sampled by torch's own F.grid_sample on the CPU in float64 (`padding_mode="zeros"`, `align_corners=False`, whose
un-normalisation ((g + 1) W - 1) / 2 of g = 2 qx / W - 1 is the package's convention: index coordinate qx - 0.5) and compared only
where the validity rule, evaluated here, holds.

The a-priori bound on a float32 bilinear value, u = 2^-24 the unit roundoff of float32, M = max |tap|:
  * the fraction fx is a float64 difference rounded to float32: |dfx| <= u / 2 (fx < 1); gx = fl(1 - fx) adds another u / 2 at
    most: |dgx| <= u.  The same in y.
  * a weight is fl(a b) with a in {fx, gx}, b in {fy, gy}: |dw| <= a |db| + b |da| + u a b.  Summed over the four weights
    (fx + gx = fy + gy = 1 up to u): (|dfy| + |dgy|) + (|dfx| + |dgx|) + u <= 1.5 u + 1.5 u + u = 4 u.
  * a product fl(w I) and the three additions of ((p00 + p01) + p10) + p11 put at most four factors (1 + e), |e| <= u, on a term:
    <= 4 u sum |w I| <= 4 u M.
  Together |v - V| <= 8 u M to first order in u -- the figure the contract expects; the terms in u^2 are 2^-24 of that, and the
  yardstick's own float64 error (a few 2^-53 M, Ws times that in the position) is smaller still.  No slack is added."""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24


def source_points(Hinv, Hd, Wd):
    """Hinv [B,3,3] float64 -> (qx, qy, w) [B,Hd,Wd] float64 in the documented order"""
    h = np.asarray(Hinv, np.float64).reshape(-1, 9)[:, :, None, None]
    x = (np.arange(Wd, dtype=np.float64) + 0.5)[None, None, :]
    y = (np.arange(Hd, dtype=np.float64) + 0.5)[None, :, None]
    X = (h[:, 0] * x + h[:, 1] * y) + h[:, 2]
    Y = (h[:, 3] * x + h[:, 4] * y) + h[:, 5]
    w = (h[:, 6] * x + h[:, 7] * y) + h[:, 8]
    with np.errstate(divide="ignore", invalid="ignore"):
        return X / w, Y / w, w + np.zeros_like(X)


def valid_rule(qx, qy, w, Hs, Ws):
    with np.errstate(invalid="ignore"):
        return np.isfinite(w) & (w > 0) & (qx >= 0.5) & (qx <= Ws - 0.5) & (qy >= 0.5) & (qy <= Hs - 0.5)


def near_boundary(qx, qy, w, Hs, Ws, eps=1e-9):
    """pixels whose validity a last-place difference could flip: q within eps of an edge of the valid rectangle, or w of 0"""
    with np.errstate(invalid="ignore"):
        near = np.abs(w) < eps
        for q, hi in ((qx, Ws - 0.5), (qy, Hs - 0.5)):
            near |= (np.abs(q - 0.5) < eps) | (np.abs(q - hi) < eps)
    return near & np.isfinite(w)


def yardstick(src, Hinv, out_shape, mode="bilinear"):
    """src [B,C,Hs,Ws] (any real dtype, CPU) -> (values float64 [B,C,Hd,Wd], valid bool [B,Hd,Wd]); values hold only where valid"""
    Hs, Ws = src.shape[-2:]
    Hd, Wd = out_shape
    qx, qy, w = source_points(Hinv, Hd, Wd)
    valid = valid_rule(qx, qy, w, Hs, Ws)
    gx = np.where(valid, 2.0 * qx / Ws - 1.0, -3.0)  # an invalid pixel samples far outside: zeros
    gy = np.where(valid, 2.0 * qy / Hs - 1.0, -3.0)
    grid = torch.from_numpy(np.stack([gx, gy], -1))
    out = F.grid_sample(src.double(), grid, mode=mode, padding_mode="zeros", align_corners=False)
    return out, torch.from_numpy(valid)


def gather_exact(src, Hinv, out_shape):
    """for a homography that takes pixel centres to pixel centres exactly: the permutation, by integer indexing.  Asserts that
    every source point is a pixel centre; -> (values of src's dtype with 0 where invalid, valid)"""
    Hs, Ws = src.shape[-2:]
    qx, qy, w = source_points(np.broadcast_to(np.asarray(Hinv).reshape(-1, 3, 3), (src.shape[0], 3, 3)), *out_shape)
    assert np.array_equal(qx - 0.5, np.rint(qx - 0.5)) and np.array_equal(qy - 0.5, np.rint(qy - 0.5))
    valid = valid_rule(qx, qy, w, Hs, Ws)
    ix = torch.from_numpy(np.where(valid, qx - 0.5, 0).astype(np.int64))
    iy = torch.from_numpy(np.where(valid, qy - 0.5, 0).astype(np.int64))
    b = torch.arange(src.shape[0])[:, None, None]
    out = src[b, :, iy, ix].permute(0, 3, 1, 2)  # [B,Hd,Wd,C] -> [B,C,Hd,Wd]
    v = torch.from_numpy(valid)
    return torch.where(v[:, None], out, torch.zeros_like(out)), v


def bound(src):
    """8 u max |tap| (module docstring), over the finite values of the source"""
    s = src.double()
    return 8.0 * U32 * float(s[torch.isfinite(s)].abs().max())


# ------------------------------------------------------------------------------------------ homographies of the cases
def translation(tx, ty):
    return np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1.0]])


def rot180(Hs, Ws):
    """about the image centre: pixel (r, c) -> pixel (Hs - 1 - r, Ws - 1 - c)"""
    return np.array([[-1.0, 0, Ws], [0, -1.0, Hs], [0, 0, 1.0]])


def rot90(Hs):
    """(x, y) -> (Hs - y, x): pixel (r, c) of an Hs x Ws image -> pixel (c, Hs - 1 - r) of a Ws x Hs image"""
    return np.array([[0.0, -1.0, Hs], [1.0, 0, 0], [0, 0, 1.0]])


def w_sign_change(Hs, Ws):
    """H whose inverse has w = 1.3 - 2 x / Ws: positive on the left 65 % of the destination, negative on the right"""
    M = np.array([[0.9, 0.05, 0.7], [-0.04, 1.1, 0.4], [-2.0 / Ws, 0.0, 1.3]])
    return np.linalg.inv(M)


def sampled(sample_homographies, B, Hs, Ws, seed, difficulty=0.7):
    return sample_homographies(B, (Ws, Hs), rng=np.random.RandomState(seed), difficulty=difficulty)


SIZES = [  # (Hs, Ws) -> (Hd, Wd)
    ((13, 19), (13, 19)),
    ((13, 19), (11, 23)),
    ((65, 346), (65, 346)),  # a row spans more than a wave, the grid more than a block
]
B = 3
SAMPLED_SEED = {(13, 19): 31, (65, 346): 32}


def inexact_cases(sample_homographies):
    """name -> (H [B,3,3], (Hs, Ws), (Hd, Wd)) of every case whose source points are rounded: the CPU module checks that none of
    their pixels lies within 1e-9 of the validity boundary (so `valid` is compared exactly, everywhere).  The sampler maps a
    quadrilateral INSIDE the source onto the whole destination, so a sampled case is valid everywhere; the inverse of a sampled
    homography (`mixed`, sample 1) shows the source as a quadrilateral inside the destination, invalid around it"""
    out = {}
    for (Hs, Ws), dst in SIZES:
        s = sampled(sample_homographies, B, Hs, Ws, SAMPLED_SEED[(Hs, Ws)])
        tag = f"{Hs}x{Ws}->{dst[0]}x{dst[1]}"
        out[f"sampled {tag}"] = (s, (Hs, Ws), dst)
        out[f"wsign {tag}"] = (np.tile(w_sign_change(Hs, Ws), (B, 1, 1)), (Hs, Ws), dst)
        out[f"mixed {tag}"] = (np.stack([translation(-1.75, 0.625), np.linalg.inv(s[0]), s[1]]), (Hs, Ws), dst)
    return out


def image(seed, B, C, Hs, Ws):
    """float32 [B,C,Hs,Ws] in 0..255, seeded"""
    return torch.from_numpy(np.random.RandomState(seed).uniform(0, 255, size=(B, C, Hs, Ws)).astype(np.float32))
