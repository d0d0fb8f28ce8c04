"""The middle of the extractor -- score map with its events mask, descriptor normalisation, bilinear keypoint sampling, the
full-resolution gather, the dense upsample -- stated as the torch calls the reference makes (citations = reference file:line), on
the CPU, values in float64.  Independent of oracle/ and of oracle/torch_cpu.py: no hand-written index formula where torch has the
op (F.pad, F.conv2d, F.pixel_shuffle, F.normalize, F.grid_sample, F.interpolate, slice assignment).  Below the statement: the
error bounds of csrc/detect.hip K3 and csrc/desc.hip, derived from the kernels' operation sequences and fitted to no run, and the
constructed inputs of tests/test_extract_ref_cpu.py and tests/test_extract_ref_gpu.py, each returned together with the facts a
test asserts about it before it looks at a result.  Not collected by pytest (no test_ prefix)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24  # unit roundoff of float32: one rounding moves a value by at most U times its magnitude (one ulp <= 2 U)
F64 = torch.float64


def _t(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------------------------------ the statement: score map
def pad_mask(mask, pads):
    """Padder.pad (core/modules/utils/util.py:17-32): a bool tensor is padded with zeros, every other dtype by repeating its edge
    pixels.  pads = (w0, w1, h0, h1), the Padder's padding_size.  (torch's replicate padding takes floating tensors only; an integer
    mask goes through float64, which holds every int64 a mask can sensibly carry, and comes back in its own dtype.)"""
    mask = _t(mask)
    if mask.dtype == torch.bool:
        return F.pad(mask, pads, mode="constant")
    if mask.dtype.is_floating_point:
        return F.pad(mask, pads, mode="replicate")
    return F.pad(mask.to(F64), pads, mode="replicate").to(mask.dtype)


def visible(mask, pads, dilate):
    """[B,1,H,W] mask of any dtype -> [B,1,Hp,Wp] bool: the pixels whose score survives `score[~score_mask] = 0`.
    dilate (event side, EventExtractors.py:357-363 and :544-550): pad, `.float()`, F.conv2d with ones / 9 and padding=1, `> 0` -- in
    float32 as the reference runs it, because the outcome depends on underflow (a mask value of 1e-45 is not visible there) and on
    cancellation (+1 and -1 in one window).
    not dilate (image side, superpoint_extractor.py:383-384,411-412): the padded mask itself.  The reference applies `~` to it, which
    is defined as a mask for bool only (bitwise on integers: `~1 == 254` zeroes every pixel; a TypeError on floats); for the other
    dtypes this is the reading the event side gives them without its box filter, `padded != 0`."""
    p = pad_mask(mask, pads)
    if not dilate:
        return p if p.dtype == torch.bool else p != 0
    m = p.float()
    kernel = torch.ones((3, 3), dtype=m.dtype).unsqueeze(0).unsqueeze(0)
    kernel = kernel / kernel.sum()
    return F.conv2d(m, kernel, padding=1) > 0


def nonzero_mask(mask):
    """the package's reading of a mask that is not bool (stated departures): its non-zero pixels, in a dtype the
    Padder still replicates.  Equal to the mask itself under `visible` unless it holds negative or denormal values."""
    mask = _t(mask)
    return mask if mask.dtype == torch.bool else (mask != 0).to(torch.uint8)


def probability(logits):
    """logits_to_prob (core/modules/utils/detector_util.py:18-45) in float64: softmax over the 65 channels, or the logistic function
    for one channel"""
    x = _t(logits, F64)
    if x.shape[1] == 1:
        return 1 / (1 + torch.exp(-x))
    return torch.softmax(x, dim=1)


def remove_border(score, border):
    """remove_border_points (detector_util.py:138-164): four slice assignments, in place"""
    if border > 0:
        score[..., :, :border] = 0.0
        score[..., :, -border:] = 0.0
        score[..., :border, :] = 0.0
        score[..., -border:, :] = 0.0
    return score


def score_map(logits, mask=None, pads=(0, 0, 0, 0), dilate=False, border=0):
    """-> (probability [B,C,hc,wc], score [B,1,Hp,Wp], visible [B,1,Hp,Wp] bool or None), values in float64:
    logits_to_prob, the dustbin split off and F.pixel_shuffle(8) (depth_to_space, detector_util.py:48-77), `score[~visible] = 0`
    (EventExtractors.py:561-562), remove_border_points.  For cell-1 networks depth_to_space returns its input, so `probability` IS
    `score`, zeros included."""
    prob = probability(logits)
    if prob.shape[1] == 1:
        score = prob
    else:
        score = F.pixel_shuffle(prob[:, :-1], 8)
    vis = None
    if mask is not None:
        vis = visible(mask, pads, dilate)
        score[~vis] = 0.0
    remove_border(score, border)
    return prob, score, vis


def apply_mask_border(score, mask, pads, dilate, border):
    """the last two steps of score_map on a map that already exists (a forward's own pixel-shuffled probability), any dtype"""
    score = _t(score).clone()
    if mask is not None:
        score[~visible(mask, pads, dilate)] = 0.0
    return remove_border(score, border)


def unpad(x, pads):
    """Padder.unpad (util.py:34-50)"""
    w0, w1, h0, h1 = pads
    h, w = x.shape[-2:]
    return x[..., h0:h - h1, w0:w - w1].clone().contiguous()


def unpad_positions(positions, pads, ordering="yx"):
    """Padder.unpad_positions (util.py:52-66) on one [n,>=2] float32 array"""
    w0, w1, h0, h1 = pads
    new = _t(positions).clone()
    first, second = (w0, h0) if ordering == "xy" else (h0, w0)
    new[..., 0] = _t(positions)[..., 0] - first
    new[..., 1] = _t(positions)[..., 1] - second
    return new.numpy()


# ------------------------------------------------------------------------------------------ the statement: descriptors
def normalize(x, scale, dim=1):
    """normalize_descriptors (core/modules/utils/descriptor_util.py:21-28): scale * F.normalize(x, p=2, dim), eps 1e-12, in float64"""
    return scale * F.normalize(_t(x, F64), p=2, dim=dim)


def _grid(positions, image_size):
    """the reference's coordinate arithmetic (descriptor_util.py:81-111) on float32 tensors exactly as written: elementwise IEEE
    operations, the same on every machine"""
    image_size = torch.tensor(image_size, dtype=torch.float)
    pos = _t(positions, torch.float32)[:, :2]
    pos = pos - 0.5
    pos = 2.0 * (pos / (image_size - 1)) - 1.0
    pos = pos[:, [1, 0]]
    return pos[None, None, ...]


def sample_raw(raw_b, positions, image_size):
    """one image: F.grid_sample of the float64 map at the float32 grid -> ([n,D] samples, [n,D] sum of |weight * tap|: the same
    call on |map|, the weights being non-negative)"""
    n = int(positions.shape[0])
    grid = _grid(positions, image_size).double()
    m = _t(raw_b, F64)[None]
    v = F.grid_sample(m, grid, mode="bilinear", align_corners=False).view(-1, n).T
    a = F.grid_sample(m.abs(), grid, mode="bilinear", align_corners=False).view(-1, n).T
    return v, a


def sample_low(raw, positions, image_size, scale):
    """sparsify_low_resolution_descriptors (descriptor_util.py:74-128): per image grid_sample(bilinear, align_corners=False, zero
    padding) at the keypoints, then normalize; an image without keypoints gives the [0, D] zeros"""
    out = []
    for i, pos in enumerate(positions):
        n = int(pos.shape[0])
        if n == 0:
            out.append(torch.zeros((0, raw.shape[1]), dtype=F64))
            continue
        out.append(normalize(sample_raw(raw[i], pos, image_size)[0], scale, dim=1))
    return out


def gather_full(raw, positions, scale):
    """sparsify_full_resolution_descriptors (descriptor_util.py:50-71): `pos.floor().long()` indexing, then normalize"""
    out = []
    for i, pos in enumerate(positions):
        p = _t(pos)[:, :2].floor().long()
        out.append(normalize(_t(raw, F64)[i, :, p[:, 0], p[:, 1]].T, scale, dim=1))
    return out


def upsample_raw(raw, size):
    """-> (resized map, the same resize of |map| = sum of |weight * tap|).  upsample_descriptors (descriptor_util.py:131-138) calls
    torchvision's resize(interpolation=BILINEAR, antialias=None); for a float tensor that is this F.interpolate call.  torchvision
    is not installed where these tests run; tests/golden/_ref_stubs.py records the same reading, and tests/golden/desc.npz
    (dense_d16) holds the reference's own output of it."""
    m = _t(raw, F64)
    kw = dict(size=tuple(int(s) for s in size), mode="bilinear", align_corners=False, antialias=False)
    return F.interpolate(m, **kw), F.interpolate(m.abs(), **kw)


def upsample(raw, size, scale, pads=(0, 0, 0, 0)):
    """upsample_descriptors + normalize_descriptors, then the crop of Padder.unpad"""
    return unpad(normalize(upsample_raw(raw, size)[0], scale, dim=1), pads)


# ------------------------------------------------------------------------------------------ bounds (units of U = 2^-24)
# Every bound is |kernel - float64 statement| <= bound, element by element, first order in U with the factor SLACK for the
# second-order terms (the largest first-order total below is ~600 U = 4e-5, so 1 + 1e-3 covers its square with room).
SLACK = 1.0 + 1e-3


def prob_bound(logits, p64):
    """score65_kernel / orc_logits_to_score: mx = max_c v_c (exact); a_c = fl(v_c - mx) carries |a_c| U, which exp turns into a
    relative |a_c| U of e_c; einx_expf is within 2 ulp <= 4 U (tests/test_oracle_golden.py::test_math_contract_vs_libm); the
    sequential sum of the 65 non-negative e_c carries 65 U plus at most the largest relative error of a term, (max|a| + 4) U; the
    division one more U:   |dp_c| <= p_c (|a_c| + max_c|a_c| + 4 + 4 + 65 + 1) U.
    score1_kernel: einx_sigmoidf within 3 ulp <= 6 U of p.
    Both hold while nothing underflows: the callers keep |a| <= 60 (e >= 8e-27, a normal float32)."""
    x = _t(logits, F64)
    if x.shape[1] == 1:
        return 6 * U * SLACK * p64
    a = (x - x.max(dim=1, keepdim=True).values).abs()
    return (a + a.max(dim=1, keepdim=True).values + 74) * U * SLACK * p64


def norm_terms_map(D):
    """roundings on the longest path of the sum of squares: normalize_map_*_kernel / upsample_den_kernel walk one fmaf chain c = 0..D-1"""
    return D


def norm_terms_wave(D):
    """desc_sample_kernel / normalize_rows_kernel: lane l chains channels l, l + 64, ..., then a 6-step butterfly"""
    return -(-D // 64) + 6


def normalized_bound(t64, E, nsum, scale, dim):
    """out = fl(scale) * (t / max(sqrt(sum t^2), 1e-12f)) against scale * t / max(|t|, 1e-12) in float64, where the kernel's t
    already differs from t64 by at most E, element by element (E = 0 for values read from memory).
      n = sqrt(s): s is a sum of non-negative terms with `nsum` roundings on its longest path (a fused multiply-add rounds once), so
        relative nsum U, halved by the square root, plus its own U; the errors E move |t| by at most |E|_2.
      den = max(n, eps) moves by no more than n or eps does (max is 1-Lipschitz; float32(1e-12) is within U of 1e-12), so a pixel
        on either side of the clamp is covered.  A sum of squares in the denormal range (|t| < 1e-19) loses absolute, not
        relative, accuracy: its n is below 1e-18 while den >= 1e-12, far inside the U eps term.
      out: the division, the product with scale and float32(scale) against the Python float: 3 U.
    |d out_c| <= scale / den (E_c + |t_c| |E|_2 / den) + |out_c| (nsum / 2 + 1 + 1 + 3) U"""
    t64 = _t(t64, F64)
    E = torch.zeros_like(t64) if E is None else _t(E, F64)
    den = torch.linalg.vector_norm(t64, dim=dim, keepdim=True).clamp_min(1e-12)
    e2 = torch.linalg.vector_norm(E, dim=dim, keepdim=True)
    out = scale * t64 / den
    return (abs(scale) / den * (E + t64.abs() * e2 / den) + out.abs() * (nsum / 2 + 5) * U) * SLACK


def sample_value_bound(raw_b, abs_sample, hc, wc):
    """desc_sample_kernel<true>: the grid value g is the statement's own float32 number.  i = ((g + 1) * size - 1) / 2 in float32
    against float64: fl(g + 1) carries 2 U (|g + 1| <= 2), the product with size <= 2 size that and its own rounding 2 size U, the
    subtraction of 1 at most 2 size U, the halving nothing: |di| <= 3 size U per axis; `w = i - floor(i)` is exact for i >= 0 and
    rounds by at most U / 2 for -1 <= i < 0, which is one more shift of the coordinate: (3 size + 1) U.  The sample is continuous
    and piecewise linear in i (zero padding included), so that moves it by at most |di| times the largest step between neighbouring
    taps of the channel along that axis, the step to the zero ring included.
    Arithmetic: a weight is fl(fl(1 - w) * fl(1 - n)) (3 U), its product with the tap U, the three additions 3 U:
    7 U sum |weight * tap|.
    -> per channel E_c = 7 U sum|w tap| + U ((3 wc + 1) step_x + (3 hc + 1) step_y)"""
    m = F.pad(_t(raw_b, F64), (1, 1, 1, 1))  # the zero ring grid_sample reads outside the map
    step_x = (m[:, :, 1:] - m[:, :, :-1]).abs().amax(dim=(1, 2))
    step_y = (m[:, 1:, :] - m[:, :-1, :]).abs().amax(dim=(1, 2))
    return 7 * U * abs_sample + U * ((3 * wc + 1) * step_x + (3 * hc + 1) * step_y)[None, :]


def upsample_value_bound(raw, abs_up, hc, wc):
    """upsample_*_kernel: source coordinate f = fl(fl(Y + 0.5) * fl(hc / Hp)) - 0.5 in float32 against float64: the ratio carries U
    and the product its own, both of a value <= hc: 2 hc U; the subtraction is exact (Sterbenz above 0.25, clamped to 0 below).
    Linear in f between two taps: 2 U (hc |tap_y1 - tap_y0| + wc |tap_x1 - tap_x0|), with the channel's largest neighbour step for
    the tap differences.  Arithmetic: t = fl(1 - l) a + l b and v = fl(1 - l') t0 + l' t1, each (1 + 1 + 1) U: 6 U sum|weight * tap|,
    taken as 7."""
    m = _t(raw, F64)
    step_x = (m[..., :, 1:] - m[..., :, :-1]).abs().amax(dim=(2, 3)) if m.shape[-1] > 1 else torch.zeros(m.shape[:2], dtype=F64)
    step_y = (m[..., 1:, :] - m[..., :-1, :]).abs().amax(dim=(2, 3)) if m.shape[-2] > 1 else torch.zeros(m.shape[:2], dtype=F64)
    return 7 * U * abs_up + 2 * U * (wc * step_x + hc * step_y)[:, :, None, None]


_WORST = {}


def within(tag, got, exp, bound):
    """assert |got - exp| <= bound element by element; prints error, bound and their ratio at the worst element (pytest -s) and
    keeps the largest ratio per tag (worst_ratios)"""
    got, exp, bound = _t(got, F64), _t(exp, F64), _t(bound, F64).expand_as(_t(exp))
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    err = (got - exp).abs()
    if err.numel() == 0:
        return 0.0
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.tensor(math.inf, dtype=F64), torch.tensor(0.0, dtype=F64)))
    i = int(ratio.argmax())
    r = float(ratio.flatten()[i])
    print(f"{tag}: error {float(err.flatten()[i]):.3e}  bound {float(bound.flatten()[i]):.3e}  ratio {r:.3f}")
    op = tag.split("[")[0]
    _WORST[op] = max(_WORST.get(op, 0.0), r)
    assert bool(torch.isfinite(got).all()) and r <= 1.0, f"{tag}: error / bound = {r:.3f} at flat index {i}"
    return r


def worst_ratios():
    return dict(_WORST)


# ------------------------------------------------------------------------------------------ inputs: masks
MASK_DTYPES = {
    # name -> (torch dtype, value of a set pixel)
    "bool": (torch.bool, True),
    "u8_1": (torch.uint8, 1),
    "u8_255": (torch.uint8, 255),
    "i64": (torch.int64, 7),
    "f32_1": (torch.float32, 1.0),
    "f32_half": (torch.float32, 0.5),
    "f64": (torch.float64, 0.25),
}
MASK_PATTERNS = ("empty", "full", "corners", "edges", "random")


def mask_pattern(pattern, B, H, W, seed=0):
    """[B,1,H,W] bool.  corners: the four corner pixels (the pixels a replicate ring grows from); edges: edge midpoints and two
    interior pixels; random: 2 % (at least one pixel)"""
    m = np.zeros((B, 1, H, W), bool)
    if pattern == "full":
        m[:] = True
    elif pattern == "corners":
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            m[:, 0, y, x] = True
    elif pattern == "edges":
        for y, x in ((0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1), (H // 2, W // 2), (H // 3, W // 3)):
            m[:, 0, y, x] = True
    elif pattern == "random":
        rng = np.random.default_rng(1000 + seed)
        m[:, 0] = rng.random((B, H, W)) < 0.02
        m[:, 0, H // 2, W // 2] = True
    else:
        assert pattern == "empty"
    return m


def typed_mask(pattern_mask, name):
    dt, v = MASK_DTYPES[name]
    t = torch.from_numpy(pattern_mask)
    return t if dt == torch.bool else t.to(dt) * v


def ring(pads, Hp, Wp):
    """[Hp,Wp] bool: the padding ring"""
    w0, w1, h0, h1 = pads
    r = torch.ones((Hp, Wp), dtype=torch.bool)
    r[h0:Hp - h1, w0:Wp - w1] = False
    return r


def special_float_mask(H, W):
    """[1,1,H,W] float32 with the values whose visibility the reference decides in float32 arithmetic: 1e-45 alone (its ninth
    underflows to 0: not visible), +1 next to -1 (their window sums cancel), 0.5 and 1.0 (visible).  -> (mask, facts)"""
    assert H >= 12 and W >= 12
    m = torch.zeros((1, 1, H, W), dtype=torch.float32)
    m[0, 0, 2, 2] = 1e-45
    m[0, 0, 2, 8], m[0, 0, 2, 9] = 1.0, -1.0
    m[0, 0, 8, 2] = 0.5
    m[0, 0, 8, 8] = 1.0
    return m, {"denormal": (2, 2), "pair": ((2, 8), (2, 9)), "half": (8, 2), "one": (8, 8)}


# ------------------------------------------------------------------------------------------ inputs: score map
SCORE_SHAPES = [
    # id, C, hc, wc, pads (w0, w1, h0, h1)
    ("c65_3x5_deep_ring", 65, 3, 5, (3, 4, 3, 4)),   # the ring is deeper than the dilation
    ("c65_33x44", 65, 33, 44, (3, 3, 2, 2)),         # the shipped geometry: 1452 cells = 46 workgroups, the last one ragged
    ("c1_nopad", 1, 19, 27, (0, 0, 0, 0)),
    ("c1_pads", 1, 19, 27, (1, 2, 2, 1)),
]


def score_logits(C, hc, wc, B=len(MASK_PATTERNS), seed=0):
    """[B,C,hc,wc] float32, |v - max| well inside the range the bound is stated for"""
    rng = np.random.default_rng(7000 + 100 * C + hc + seed)
    x = (rng.standard_normal((B, C, hc, wc)) * 2).astype(np.float32)
    x[0, :, 0, 0] *= 4  # one cell with a wide spread of arguments
    return x


# ------------------------------------------------------------------------------------------ inputs: descriptors
def desc_values(seed, shape, lo=-3.0, hi=3.0):
    """float32 values with magnitudes 10^lo .. 10^hi and random signs: inside |x| in [1e-15, 1e15], where float32 neither
    overflows nor underflows in a sum of squares"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(lo, hi, size=shape)
    return (mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def normalize_input(D, P, B=2, seed=0):
    """[B,D,P] with a zero pixel (B 0, pixel 0) and a pixel of 1e-20 values (the last one of the last image): -> (x, facts)"""
    x = desc_values(300 + D * 7 + P + seed, (B, D, P), -2.0, 2.0)
    x[0, :, 0] = 0.0
    x[B - 1, :, P - 1] = np.float32(1e-20)
    n = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    return x, {"zero": (0, 0), "tiny": (B - 1, P - 1), "norms": n}


def range_edge_input(D, P):
    """[1,D,P] float32 at the range edges, compared with torch's CPU float32 op on the zero / inf pattern only: pixel 0 holds 1e30
    (the sum of squares overflows, the denominator is inf, the output 0), pixel 1 holds 1e-30 (the squares underflow to 0, the
    clamp divides: 1e-18), the others are ordinary"""
    x = desc_values(17, (1, D, P), -1.0, 1.0)
    x[0, :, 0] = np.float32(1e30)
    if P > 1:
        x[0, :, 1] = np.float32(1e-30)
    return x


SAMPLE_MAP = (3, 4)          # hc, wc
SAMPLE_PADDED = (24, 32)     # Hp, Wp


def sample_keypoints():
    """flat indices into the padded 24x32 image: four corners, every pixel of the edge rows and columns, an interior grid.
    -> (sorted unique int32 indices, facts: which of them have a tap outside the 3x4 map)"""
    Hp, Wp = SAMPLE_PADDED
    pts = {(0, 0), (0, Wp - 1), (Hp - 1, 0), (Hp - 1, Wp - 1)}
    pts |= {(0, x) for x in range(Wp)} | {(Hp - 1, x) for x in range(Wp)} | {(y, 0) for y in range(Hp)} | {(y, Wp - 1) for y in range(Hp)}
    pts |= {(y, x) for y in range(3, Hp - 1, 5) for x in range(2, Wp - 1, 7)}
    idx = np.array(sorted(y * Wp + x for y, x in pts), np.int32)
    return idx


def positions_of(idx, Wp):
    """keypoint rows (y + 0.5, x + 0.5, 0) of flat padded indices, as the detector emits them before unpad_positions"""
    idx = np.asarray(idx, np.int64)
    return np.stack([idx // Wp + 0.5, idx % Wp + 0.5, np.zeros(len(idx))], 1).astype(np.float32)


def taps_outside(positions, image_size, hc, wc):
    """[n] bool: one of the keypoint's four taps lies outside the [hc,wc] map and carries weight (from the statement's own grid,
    un-normalised the way grid_sample documents align_corners=False: i = ((g + 1) * size - 1) / 2)"""
    g = _grid(positions, image_size).double()[0, 0]
    ix, iy = ((g[:, 0] + 1) * wc - 1) / 2, ((g[:, 1] + 1) * hc - 1) / 2
    return ((ix < 0) | (ix > wc - 1) | (iy < 0) | (iy > hc - 1)).numpy()


UPSAMPLE_CASES = [
    # B, D, hc, wc, Hp, Wp, (h0, w0, H, W): the small geometries of test_desc_gpu.py::test_upsample_normalize_bands + the shipped one at D = 16
    (2, 16, 5, 7, 40, 56, (2, 3, 35, 50)),        # scale 1/8 with a crop window
    (2, 7, 5, 7, 33, 47, (0, 0, 33, 47)),         # non-integer scale, no crop
    (1, 9, 5, 7, 10, 14, (1, 2, 8, 11)),          # x2
    (1, 4, 8, 9, 8, 9, (0, 0, 8, 9)),             # identity size
    (1, 5, 6, 70, 120, 140, (3, 1, 110, 139)),    # 1/20 vertically: bands taller than one sweep; several column blocks
    (1, 6, 4, 60, 16, 360, (0, 0, 16, 360)),      # the LDS limit of the two-kernel path
    (1, 6, 4, 63, 16, 378, (0, 0, 16, 378)),      # one word more: the band kernel
    (1, 16, 33, 44, 264, 352, (2, 3, 260, 346)),  # the shipped geometry
]


def upsample_pads(case):
    B, D, hc, wc, Hp, Wp, (h0, w0, H, W) = case
    return (w0, Wp - w0 - W, h0, Hp - h0 - H)


# ------------------------------------------------------------------------------------------ shared case tables
BORDERS = (0, 1, 4)
NORMALIZE_D = (1, 7, 64, 65, 512, 513)   # 513: normalize_map_kernel, the fall-back past the LDS tile's 512 channels
NORMALIZE_P = (1, 31, 32, 33)            # around the 32-pixel tile
SAMPLE_D = (1, 63, 64, 65, 256, 512)
GATHER_CASE = (128, 5, 7, 1.41)          # D, H, W, scale


def score_geometry(C, hc, wc, pads):
    cell = 8 if C == 65 else 1
    Hp, Wp = hc * cell, wc * cell
    w0, w1, h0, h1 = pads
    return Hp, Wp, Hp - h0 - h1, Wp - w0 - w1


def pattern_batch(H, W):
    """[len(MASK_PATTERNS),1,H,W] bool: one image per pattern"""
    return np.concatenate([mask_pattern(p, 1, H, W) for p in MASK_PATTERNS], 0)


def sample_case(D, seed=0):
    """-> (raw [2,D,3,4], [idx lists of the two launches], cap): counts (cap, 0) and (5, cap - 1), cap no multiple of 4"""
    hc, wc = SAMPLE_MAP
    raw = desc_values(500 + D + seed, (2, D, hc, wc), -2.0, 2.0)
    idx = sample_keypoints()
    if len(idx) % 4 == 0:
        idx = idx[:-1]
    cap = len(idx)
    return raw, [[idx, idx[:0]], [idx[:5], idx[1:]]], cap


def gather_positions(H, W):
    """every pixel of the map, at fractional offsets that floor() removes: [n,3] float32 (y, x, 0)"""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    frac_y = np.linspace(0.0, 0.96875, H * W).reshape(H, W)
    frac_x = frac_y[::-1, ::-1]
    return np.stack([(ys + frac_y).ravel(), (xs + frac_x).ravel(), np.zeros(H * W)], 1).astype(np.float32)


def filter_positions(positions, image_size, ordering="yx"):
    """filter_sparse_feats (EventExtractors.py:496-515): the keypoints inside the un-padded image"""
    p = _t(positions)
    h, w = image_size
    y, x = (p[:, 1], p[:, 0]) if ordering == "xy" else (p[:, 0], p[:, 1])
    valid = ((x >= 0) & (x < w)) & ((y >= 0) & (y < h))
    return p[valid].numpy()


def zero_inf_pattern(x):
    """what the range-edge cases compare: where a result is 0, infinite or NaN"""
    x = _t(x)
    return torch.stack([x == 0, torch.isinf(x), torch.isnan(x)]).numpy()


# ------------------------------------------------------------------------------------------ one forward per extractor family
def forward_case(G, side):
    """the cell-8 small case of tests/golden/conv.npz (37x45 images: every pad exceeds remove_borders = 0), its mask replaced by a
    uint8 {0, 1} one that is visible everywhere but in two blocks, so that the padding ring inherits the image edge.
    -> (case, state dict of the side's extractor, kind, config section, input, mask, pads)"""
    from helpers import state_dict_for, sub_dict, synth
    c = G.cases["vgg5_small"]
    H, W = c.get("H", 260), c.get("W", 346)
    kind = c["cfg"][f"{side}_extractor"]["type"]
    sec = c["cfg"][f"{side}_extractor"][kind]
    sd = sub_dict(state_dict_for(c, G), f"{side}_extractor.extractor.")
    x = synth.synth_events(c["iseed"], c["B"], c["ce"], H, W)[0] if side == "event" else synth.synth_image(c["iseed"], c["B"], H, W)
    m = np.ones((c["B"], 1, H, W), np.uint8)
    m[:, 0, 10:18, 20:30] = 0
    m[-1, 0, 25:, :9] = 0
    w0, w1, h0, h1 = (lambda hp, wp: (wp // 2, wp - wp // 2, hp // 2, hp - hp // 2))((((H // 8) + 1) * 8 - H) % 8, (((W // 8) + 1) * 8 - W) % 8)
    return c, sd, kind, sec, x, m, (w0, w1, h0, h1)


def forward_chain(probability, mask, pads, kind, sec, image_size, border=0):
    """what a forward's `score`, `nms` and `sparse_positions` are, from its own `probability`: pixel shuffle, the statement's mask
    and border, detect_ref.nms_torch, detect_ref.select_torch on the padded map, unpad_positions and the in-image filter"""
    import detect_ref as dr
    p = _t(probability)
    shuf = F.pixel_shuffle(p[:, :-1], 8) if p.shape[1] == 65 else p
    s = apply_mask_border(shuf, mask, pads, dilate=kind in ("vgg", "vgg_np"), border=border)
    nms, _ = dr.nms_torch(s[:, 0].numpy(), sec["nms_radius"])
    kept, pos, _, _ = dr.select_torch(nms, sec["detection_top_k"], sec["detection_threshold"], ordering=sec.get("ordering", "yx"))
    pos = [filter_positions(unpad_positions(q, pads, sec.get("ordering", "yx")), image_size, sec.get("ordering", "yx")) for q in pos]
    return {"score": unpad(s, pads).numpy(), "nms": unpad(_t(kept), pads).numpy(), "sparse_positions": pos}
