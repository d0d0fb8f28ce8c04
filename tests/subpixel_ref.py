"""Sub-pixel keypoints restated for the tests: the refinement rule in numpy, evaluated op by op in float32 (the
expected value of csrc/subpixel.hip, which performs the same IEEE operations in the same order) and in float64; the
float-position descriptor sampler as the reference's own torch calls in float64 (extract_ref.sample_raw / normalize:
F.grid_sample(bilinear, align_corners=False, zero padding) + F.normalize); the a-priori error bound of the kernel's sampler,
derived from its operation sequence and fitted to no run; and the constructed inputs of tests/test_subpixel_cpu.py and
tests/test_subpixel_gpu.py.  Not collected by pytest (no test_ prefix)."""
import numpy as np
import torch
import torch.nn.functional as F

import extract_ref as er

U = er.U
F64 = torch.float64
DMAX = 0.5 - 2.0 ** -10          # exact in float32 and float64
MAX_SIDE = 8192


# ------------------------------------------------------------------------------------------ the rule
def offset(l, c, r, dtype=np.float32):
    """vertex of the parabola through (-1, l), (0, c), (+1, r) relative to the centre, elementwise on arrays, every operation
    rounded once in `dtype` in the stated order; 0 unless l < c and r < c (ties, NaN); clamped to +-DMAX"""
    l, c, r = (np.asarray(v, dtype) for v in (l, c, r))
    half, dmax = dtype(0.5), dtype(DMAX)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (l < c) & (r < c)
        a = l - c
        b = r - c
        den = a + b
        num = l - r
        delta = (half * num) / den
        delta = np.minimum(np.maximum(delta, -dmax), dmax)
    return np.where(ok, delta, dtype(0.0)).astype(dtype)


def refine(score, indices, pads=(0, 0, 0, 0), dtype=np.float32):
    """score [Hp,Wp] float32, indices [n] flat -> (positions [n,2] (y, x) in the un-padded frame, padded-frame positions [n,2],
    offsets [n,2] (dy, dx)), all in `dtype`: an axis whose neighbour lies outside the map keeps offset 0"""
    Hp, Wp = score.shape
    w0, _, h0, _ = pads
    idx = np.asarray(indices, np.int64)
    y, x = idx // Wp, idx % Wp
    s = np.asarray(score, np.float32)
    c = s[y, x]
    inx, iny = (x > 0) & (x < Wp - 1), (y > 0) & (y < Hp - 1)
    xl, xr = np.clip(x - 1, 0, Wp - 1), np.clip(x + 1, 0, Wp - 1)
    yu, yd = np.clip(y - 1, 0, Hp - 1), np.clip(y + 1, 0, Hp - 1)
    dx = np.where(inx, offset(s[y, xl], c, s[y, xr], dtype), dtype(0.0)).astype(dtype)
    dy = np.where(iny, offset(s[yu, x], c, s[yd, x], dtype), dtype(0.0)).astype(dtype)
    py = (y.astype(dtype) + dtype(0.5)) + dy
    px = (x.astype(dtype) + dtype(0.5)) + dx
    padded = np.stack([py, px], 1).astype(dtype)
    pos = np.stack([py - dtype(h0), px - dtype(w0)], 1).astype(dtype)
    return pos, padded, np.stack([dy, dx], 1).astype(dtype)


# ------------------------------------------------------------------------------------------ the sampler: statement and bound
def sample(raw, positions, image_size, scale):
    """the reference's sparsify_low_resolution_descriptors for any positions: list over images of [n_i,D] float64"""
    return er.sample_low(raw, positions, image_size, scale)


def sample_value_bound(raw_b, positions, image_size):
    """|kernel's un-normalised sample - extract_ref.sample_raw| for subpixel.hip's sampler at float positions -> ([n,D] float64
    samples, [n,D] bound).  The derivation is extract_ref.sample_value_bound's, extended to positions outside the image:
      the grid value g = 2 ((p - 0.5) / (size - 1)) - 1 is computed by the kernel with the same float32 IEEE operations as the
        statement's `_grid`, so both start from the SAME float32 number (the refined position itself is a float32 the kernel
        wrote, the statement reads it back);
      i = ((g + 1) * size - 1) / 2 in float32 against float64, with G = max(2, |g + 1|) (2 inside the image, above it for a
        position beyond the far edge): fl(g + 1) carries G U, the product with size that times size plus its own rounding
        G size U, the subtraction of 1 at most (G size + 1) U, the halving nothing: |di| <= (3 G size + 1) U / 2 per axis;
        `w = i - floor(i)` is exact for i >= 0 and rounds by at most U / 2 for -1 < i < 0: one more U on the coordinate;
      the sample is continuous and piecewise linear in i, zero beyond (-1, size) on both sides (the kernel's float test of i
        against that window cuts it where the statement's weights reach the zero ring), so a shift of i moves it by at most
        |di| times the channel's largest step between neighbouring taps along the axis, the step to the zero ring included;
      arithmetic as in desc_sample_kernel: 7 U sum |weight * tap|."""
    hc, wc = raw_b.shape[-2:]
    v, a = er.sample_raw(raw_b, positions, image_size)
    g = er._grid(positions, image_size).double()[0, 0]  # [n,2] (x, y)
    Gx = (g[:, 0] + 1).abs().clamp_min(2.0)
    Gy = (g[:, 1] + 1).abs().clamp_min(2.0)
    m = F.pad(er._t(raw_b, F64), (1, 1, 1, 1))
    step_x = (m[:, :, 1:] - m[:, :, :-1]).abs().amax(dim=(1, 2))
    step_y = (m[:, 1:, :] - m[:, :-1, :]).abs().amax(dim=(1, 2))
    dix = ((3 * Gx * wc + 1) / 2 + 1)[:, None]
    diy = ((3 * Gy * hc + 1) / 2 + 1)[:, None]
    return v, 7 * U * a + U * (dix * step_x[None, :] + diy * step_y[None, :])


def sample_bound(raw_b, positions, image_size, scale):
    """-> (expected [n,D] float64 normalised descriptors, bound [n,D]) for one image"""
    D = raw_b.shape[0]
    v, E = sample_value_bound(raw_b, positions, image_size)
    return er.normalize(v, scale, dim=1), er.normalized_bound(v, E, er.norm_terms_wave(D), scale, dim=1)


# ------------------------------------------------------------------------------------------ inputs: descriptor sampling
SAMPLE_MAP = (5, 6)        # hc, wc
SAMPLE_PADDED = (40, 48)   # Hp, Wp
SAMPLE_D = (8, 68, 256)
SAMPLE_CAPS = (1, 4, 5, 9)  # four keypoints per workgroup: a partial, a full, a full + a partial, two full + a partial


def sample_raw_map(D, seed=0):
    hc, wc = SAMPLE_MAP
    return er.desc_values(900 + D + seed, (2, D, hc, wc), -2.0, 2.0)


def centre_indices(cap):
    """flat padded indices of `cap` pixels: the corners first, then interior pixels"""
    Hp, Wp = SAMPLE_PADDED
    pts = [(0, 0), (Hp - 1, Wp - 1), (0, Wp - 1), (Hp - 1, 0), (3, 4), (20, 24), (7, 41), (33, 9), (12, 12)]
    return np.array([y * Wp + x for y, x in pts[:cap]], np.int32)


def float_positions(seed=0):
    """[n,3] float32 (y, x, 0) in the padded frame: the exact corners (0, 0) and (Hp, Wp), positions on tap boundaries (map
    coordinate an integer: p = (k + 0.5) (size - 1) / cells + 0.5 where that is a float32), a band of 3 px outside the image on
    every side, far outside (all four taps in the zero ring), and random positions inside.  -> (positions, facts)"""
    Hp, Wp = SAMPLE_PADDED
    hc, wc = SAMPLE_MAP
    rng = np.random.default_rng(4100 + seed)
    rows = [(0.0, 0.0), (float(Hp), float(Wp)), (0.0, float(Wp)), (float(Hp), 0.0)]
    rows += [((k + 0.5) * (Hp - 1) / hc + 0.5, (j + 0.5) * (Wp - 1) / wc + 0.5) for k in range(hc) for j in (0, wc - 1)]
    n_band = 24
    for k in range(n_band):  # the band: one coordinate up to 3 px outside, the other anywhere from -3 to size + 3
        side = k % 4
        t = rng.uniform(0.0, 3.0)
        o = rng.uniform(-3.0, (Wp if side < 2 else Hp) + 3.0)
        rows.append([(-t, o), (Hp + t, o), (o, -t), (o, Wp + t)][side])
    far = [(-30.0, 10.0), (10.0, -40.0), (Hp + 25.0, 5.0), (5.0, Wp + 33.0), (-1e6, 1e6)]
    rows += far
    rows += [(rng.uniform(0, Hp), rng.uniform(0, Wp)) for _ in range(40)]
    p = np.zeros((len(rows), 3), np.float32)
    p[:, :2] = np.array(rows, np.float64).astype(np.float32)
    first_far = 4 + 2 * hc + n_band
    return p, {"far": list(range(first_far, first_far + len(far)))}


# ------------------------------------------------------------------------------------------ inputs: refinement
REFINE_MAP = (24, 32)
REFINE_PADS = (3, 2, 1, 2)  # w0, w1, h0, h1


def refine_case():
    """-> (score [3,24,32] float32, indices [3,cap] int32, counts [3], facts).  Image 0: constructed peaks (dyadic values, ties,
    map edges and corners, a NaN neighbour, offsets beyond the clamp on both sides, selections that are no maxima -- what a
    radius-0 detection emits); image 1: peaks with random float32 neighbours (the division's rounding); image 2: no keypoints."""
    Hp, Wp = REFINE_MAP
    s = np.zeros((3, Hp, Wp), np.float32)
    pts, facts = [], {}

    def put(name, y, x, c, l=None, r=None, u=None, d=None):
        s[0, y, x] = c
        for v, (yy, xx) in ((l, (y, x - 1)), (r, (y, x + 1)), (u, (y - 1, x)), (d, (y + 1, x))):
            if v is not None:
                s[0, yy, xx] = v
        facts[name] = len(pts)
        pts.append(y * Wp + x)

    put("dyadic", 5, 5, 1.0, l=0.5, r=0.75, u=0.25, d=0.75)           # dx = 1/6 rounded, dy = 0.25 exactly
    put("tie", 5, 12, 1.0, l=1.0, r=0.5, u=0.5, d=0.5)                 # a tie on x: 0; symmetric on y: 0
    put("row0", 0, 8, 1.0, l=0.5, r=0.25)                               # no row above: dy = 0, dx = -0.1
    put("col0", 10, 0, 1.0, u=0.5, d=0.25)
    put("last_row", Hp - 1, 20, 1.0, l=0.25, r=0.5)
    put("last_col", 12, Wp - 1, 1.0, u=0.25, d=0.5)
    put("corner", Hp - 1, Wp - 1, 1.0)
    put("corner0", 0, 0, 1.0)
    put("nan", 10, 10, 1.0, l=np.nan, r=0.5, u=0.5, d=0.25)            # NaN neighbour on x: 0; y refined
    put("clamp_neg", 15, 15, 1.0, l=1.0 - 2.0 ** -12, r=0.0, u=0.0, d=0.0)
    put("clamp_pos", 15, 22, 1.0, l=0.0, r=1.0 - 2.0 ** -12, u=0.0, d=1.0 - 2.0 ** -12)
    put("no_max", 19, 5, 0.5, l=0.75, r=0.25, u=0.25, d=0.25)          # a radius-0 selection on a slope
    put("valley", 19, 12, 0.25, l=0.5, r=0.5, u=0.5, d=0.5)            # a minimum
    rng = np.random.default_rng(77)
    rnd = []
    for y in range(3, Hp - 2, 4):
        for x in range(3, Wp - 2, 5):
            if len(rnd) < len(pts):
                s[1, y - 1:y + 2, x - 1:x + 2] = rng.uniform(0.0, 0.9, (3, 3)).astype(np.float32)
                s[1, y, x] = np.float32(rng.uniform(0.9, 1.0))
                rnd.append(y * Wp + x)
    cap = len(pts)
    assert cap % 4 != 0 and len(rnd) == cap
    idx = np.zeros((3, cap), np.int32)
    idx[0], idx[1] = pts, rnd
    return s, idx, np.array([cap, cap, 0], np.int32), facts


def detector_positions(indices, score, pads, ordering="yx"):
    """[B,cap,3] float32 as einx_detect writes them: (y + 0.5 - h0, x + 0.5 - w0, score) or (x.., y.., score)"""
    B, cap = indices.shape
    Hp, Wp = score.shape[-2:]
    w0, _, h0, _ = pads
    y, x = indices // Wp, indices % Wp
    py = (y.astype(np.float32) + np.float32(0.5)) - np.float32(h0)
    px = (x.astype(np.float32) + np.float32(0.5)) - np.float32(w0)
    sc = np.stack([score[b].reshape(-1)[indices[b]] for b in range(B)])
    cols = (px, py, sc) if ordering == "xy" else (py, px, sc)
    return np.stack(cols, -1).astype(np.float32)


# ------------------------------------------------------------------------------------------ inputs: the blob scene
BLOB_MAP = (64, 96)
BLOB_SIGMA = 1.5
BLOB_SPACING = 12
BLOB_IMAGES = 14   # 5 x 8 blobs per image: 560 blobs
BLOB_A = 0.05      # condition A: every refined keypoint within this of its blob's centre (px)
BLOB_B = 0.3       # condition B: the pixel centres are on average at least this far off (px)


def blob_scene():
    """-> (score [14,64,96] float32, centres [14,40,2] float64 (y, x)): Gaussian blobs of sigma 1.5 on a 12 px lattice, each
    centre moved by its own uniform offset in [0, 1)^2, sampled at the pixel centres (y + 0.5, x + 0.5)"""
    H, W = BLOB_MAP
    rng = np.random.default_rng(2024)
    gy, gx = np.meshgrid(np.arange(6, H - 5, BLOB_SPACING), np.arange(6, W - 5, BLOB_SPACING), indexing="ij")
    base = np.stack([gy.ravel(), gx.ravel()], 1).astype(np.float64)
    centres = base[None] + rng.uniform(0.0, 1.0, (BLOB_IMAGES, base.shape[0], 2))
    yy, xx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    s = np.zeros((BLOB_IMAGES, H, W), np.float64)
    for b in range(BLOB_IMAGES):
        for cy, cx in centres[b]:
            s[b] += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * BLOB_SIGMA ** 2))
    return s.astype(np.float32), centres


def blob_peaks(score, radius=4, thr=0.5):
    """flat indices of the strict radius-`radius` maxima above thr of one [H,W] map, in raster order (what einx_detect selects
    on this scene: no ties, peaks 12 px apart)"""
    H, W = score.shape
    p = np.pad(score, radius, constant_values=-np.inf)
    best = np.full_like(score, -np.inf)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            if (dy, dx) != (radius, radius):
                best = np.maximum(best, p[dy:dy + H, dx:dx + W])
    return np.flatnonzero(((score > best) & (score > thr)).ravel()).astype(np.int32)


def blob_errors(positions, indices, centres_b, W):
    """one image: keypoints (y, x) [n,>=2] with their flat indices against the blob centres -> (error of each blob's keypoint
    [40], error of its pixel centre [40]); every blob must own exactly one keypoint, on the pixel that holds its centre"""
    idx = np.asarray(indices, np.int64)
    own = np.floor(centres_b).astype(np.int64)
    flat = own[:, 0] * W + own[:, 1]
    assert sorted(idx.tolist()) == sorted(flat.tolist()), "the selected peaks are not the blobs' own pixels"
    order = np.array([int(np.flatnonzero(idx == f)[0]) for f in flat])
    p = np.asarray(positions, np.float64)[order, :2]
    err = np.sqrt(((p - centres_b) ** 2).sum(1))
    pix = np.sqrt((((own + 0.5) - centres_b) ** 2).sum(1))
    return err, pix
