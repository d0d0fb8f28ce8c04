"""The detector tail's rules (fix-point NMS, quantile threshold, raster compaction), stated twice and independently of oracle/:
`nms_ref` in exact NumPy comparisons, `nms_torch` / `select_torch` in torch's own CPU operations (unfold / argmax / fold,
torch.quantile), plus the constructed inputs of tests/test_detect_paths_cpu.py and tests/test_detect_paths_gpu.py.  Every input
builder returns the map together with the facts a test asserts about it before it looks at a result -- the facts are what routes
the input down one path of csrc/detect.hip.  Not collected by pytest (no test_ prefix)."""
import numpy as np
import torch
import torch.nn.functional as F

from helpers import synth

# the constants of csrc/detect.hip that decide a path
NMS_TH, NMS_TW = 32, 64      # NMS tile
NMS_FIN_MAXT = 2048          # tiles the finisher tracks individually
SEL_LCAP = 6144              # candidates the selection kernel keeps in LDS
SEL_SLICE = 256              # a wave's slice of the map is a multiple of 64 lanes x 4 values
SEL_WAVES = 16


# ------------------------------------------------------------------------------------------ the rules
def _padded(a, R, fill):
    B, H, W = a.shape
    p = np.full((B, H + 2 * R, W + 2 * R), fill, a.dtype)
    p[:, R:R + H, R:R + W] = a
    return p


def is_max(m, R):
    """a pixel is a maximum iff every earlier raster tap of its zero-padded window is < it and every later tap is <= it"""
    B, H, W = m.shape
    p = _padded(m, R, 0)
    ok = np.ones(m.shape, bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy == 0 and dx == 0:
                continue
            tap = p[:, R + dy:R + dy + H, R + dx:R + dx + W]
            ok &= (tap < m) if (dy < 0 or (dy == 0 and dx < 0)) else (tap <= m)
    return ok


def max_elsewhere(peak, R):
    """pixels that have a maximum in their window at another position than their own"""
    B, H, W = peak.shape
    p = _padded(peak, R, False)
    near = np.zeros(peak.shape, bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy or dx:
                near |= p[:, R + dy:R + dy + H, R + dx:R + dx + W]
    return near


def nms_ref(m, R):
    """[B,H,W] float32 -> (suppressed map, passes).  The count of maxima is taken over the WHOLE batch; the loop ends when it
    repeats, otherwise every pixel with a maximum elsewhere in its window becomes 0."""
    m = np.array(m, np.float32)
    assert m.ndim == 3
    if R == 0:
        return m, 0
    count, passes = None, 0
    while True:
        peak = is_max(m, R)
        n = int(peak.sum())
        if n == count:
            return m, passes
        count = n
        m[max_elsewhere(peak, R)] = 0.0
        passes += 1


def nms_per_image_fixpoint(m, R, positive_only=False):
    """how the kernels iterate: per image, until a pass changes nothing (the reference stops the whole batch when the count of
    maxima repeats).  positive_only = the rule the kernels had before their is-max test lost its `centre > 0` term; kept so that
    the CPU suite shows which sign inputs tell the two rules apart (the GPU rows built on them fail with the term back)."""
    m = np.array(m, np.float32)
    for b in range(m.shape[0]):
        x = m[b:b + 1]
        while True:
            peak = is_max(x, R)
            if positive_only:
                peak &= x > 0
            kill = max_elsewhere(peak, R) & (x != 0)
            if not kill.any():
                break
            x[kill] = 0.0
    return m


def border_ref(m, border):
    """remove_border_points: a frame of `border` pixels set to 0 (slices, so a frame wider than the map clears all of it)"""
    m = np.array(m, np.float32)
    if border > 0:
        m[..., :, :border] = 0.0
        m[..., :, -border:] = 0.0
        m[..., :border, :] = 0.0
        m[..., -border:, :] = 0.0
    return m


def nms_torch(m, R):
    """the same loop in torch's CPU operations: unfold the zero-padded map into window columns, a pixel is a maximum when argmax
    (first maximum) over its column is the centre tap; fold the maxima back over their windows without the centre tap to find
    the pixels they suppress.  Unfolding costs (2R+1)^2 copies of the map: small maps only."""
    x = torch.from_numpy(np.array(m, np.float32))[:, None]
    if R == 0:
        return x[:, 0].numpy(), 0
    B, _, H, W = x.shape
    k = 2 * R + 1
    taps, centre = k * k, (k * k) // 2
    count, passes = None, 0
    while True:
        cols = F.unfold(x, kernel_size=k, padding=R)              # [B, taps, H*W]
        peak = cols.argmax(dim=1) == centre                       # [B, H*W]
        n = int(peak.sum())
        if n == count:
            return x[:, 0].numpy(), passes
        count = n
        spread = peak.to(torch.float32)[:, None, :].repeat(1, taps, 1)
        spread[:, centre] = 0.0
        near = F.fold(spread, output_size=(H, W), kernel_size=k, padding=R) > 0
        x = x.masked_fill(near, 0.0)
        passes += 1


def select_torch(m, top_k, det_thr, pads=(0, 0, 0, 0), ordering="yx"):
    """[B,Hp,Wp] float32 (NMS already done) -> (nms [B,H,W], positions list, flat padded indices list, thr [B]) in float32 torch:
    thr = min(midpoint quantile at (N - k) / N, det_thr), zeros instead of the quantile when k >= N, det_thr alone without k."""
    t = torch.from_numpy(np.array(m, np.float32))
    B, Hp, Wp = t.shape
    N = Hp * Wp
    thr = torch.full((B,), float(det_thr), dtype=torch.float32)
    if top_k:
        if top_k >= N:
            tk = torch.zeros((B,), dtype=torch.float32)
        else:
            q = (N - torch.tensor(int(top_k))) / N  # integer tensor / Python int: float32
            assert q.dtype == torch.float32
            tk = t.reshape(B, -1).quantile(q, dim=1, interpolation="midpoint")
        thr = torch.minimum(tk, thr)
    kept = torch.where(t > thr[:, None, None], t, torch.tensor(0.0))
    w0, w1, h0, h1 = pads
    crop = kept[:, h0:Hp - h1, w0:Wp - w1]
    pos, idx = [], []
    for b in range(B):
        yx = torch.nonzero(crop[b] > 0)  # raster order
        v = crop[b][yx[:, 0], yx[:, 1]]
        fy, fx = yx[:, 0].to(torch.float32) + 0.5, yx[:, 1].to(torch.float32) + 0.5
        first, second = (fx, fy) if ordering == "xy" else (fy, fx)
        pos.append(torch.stack([first, second, v], 1).numpy())
        idx.append(((yx[:, 0] + h0) * Wp + yx[:, 1] + w0).to(torch.int32).numpy())
    return crop.contiguous().numpy(), pos, idx, thr.numpy()


def quantile_ranks(N, k):
    """the two sorted positions torch.quantile(interpolation='midpoint') really reads at the reference's q: the midpoint quantile
    of arange(N) is (lo + hi) / 2, 'lower' is lo and 'higher' is hi.  float32 like the maps, so that torch computes the rank in
    the arithmetic it uses for them; integers and half-integers below 2^23 are exact there."""
    assert N < (1 << 23)
    q = (N - torch.tensor(int(k))) / N
    a = torch.arange(N, dtype=torch.float32)
    lo, hi = float(a.quantile(q, interpolation="lower")), float(a.quantile(q, interpolation="higher"))
    assert float(a.quantile(q, interpolation="midpoint")) == (lo + hi) / 2
    return int(lo), int(hi)


# ------------------------------------------------------------------------------------------ facts about an input
def ntiles(H, W):
    return -(-H // NMS_TH) * -(-W // NMS_TW)


def sign_of(m):
    """'nonneg' (no value below 0), 'neg' (all below 0), 'nonpos' (none above 0, some exact zeros) or 'mixed'"""
    if float(m.min()) >= 0:
        return "nonneg"
    return "neg" if float(m.max()) < 0 else ("nonpos" if float(m.max()) == 0 else "mixed")


def nz_per_image(m):
    return [int(np.count_nonzero(x)) for x in m]


# ------------------------------------------------------------------------------------------ NMS inputs
NMS_SIZES = [
    # H, W, what the size routes to in nms4_tile / nms_pass_kernel<R>, the condition (asserted by the test on H, W)
    (1, 1, "map smaller than every radius", lambda H, W: max(H, W) == 1),
    (1, 9, "one row: no tap above or below is in the image", lambda H, W: H == 1 and W > 4),
    (9, 1, "one column, Wp & 3 != 0: scalar stores", lambda H, W: W == 1 and H > 4),
    (3, 3, "map smaller than radius 3 and 4", lambda H, W: max(H, W) <= 3),
    (31, 63, "one partial tile, Wp & 3 != 0: scalar stores", lambda H, W: ntiles(H, W) == 1 and H < NMS_TH and W < NMS_TW and W & 3),
    (32, 64, "exactly one tile: vector stores only", lambda H, W: (H, W) == (NMS_TH, NMS_TW)),
    (33, 65, "four tiles, three of them one pixel wide or high", lambda H, W: ntiles(H, W) == 4 and H % NMS_TH == 1 and W % NMS_TW == 1),
    (40, 67, "Wp & 3 != 0: every store scalar, two tiles per row", lambda H, W: (W & 3) != 0 and W > NMS_TW),
    (32, 68, "aligned rows, last 8-column group crosses Wp", lambda H, W: (W & 3) == 0 and W % 8 != 0),
    (70, 130, "3 x 3 tiles, partial in both directions", lambda H, W: ntiles(H, W) == 9 and H % NMS_TH and W % NMS_TW),
]


def nms_size_map(H, W):
    """B = 2: image 0 holds 8 levels (ties everywhere: several passes, first raster wins), image 1 distinct peaky values"""
    u = synth.uniform01(4100 + 131 * H + W, (2, H, W))
    m = u.copy()
    m[0] = np.floor(u[0] * np.float32(8)) / np.float32(8)
    m[1] = u[1] ** 4
    return m.astype(np.float32)


SEAM_H, SEAM_W = 2 * NMS_TH, 2 * NMS_TW
DIRS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]


def _pair(R, d, dist):
    """two pixels `dist` apart along direction d = (dy, dx), on either side of the tile seam(s) the direction crosses"""
    def start(s, seam, free):
        if s > 0:
            return seam - 1 - dist // 2
        if s < 0:
            return seam + dist // 2
        return free
    ya, xa = start(d[0], NMS_TH, 12), start(d[1], NMS_TW, 20)
    return (ya, xa), (ya + d[0] * dist, xa + d[1] * dist)


def nms_seam_maps(R):
    """64 x 128 = 2 x 2 tiles, seams at x = 63|64 and y = 31|32.  -> (maps [19,64,128], facts): images 0-7 an equal-valued pair at
    Chebyshev distance R across the seam in each of the eight directions (first raster wins), 8-15 the same at distance R + 1 (both
    survive), 16 / 17 a strictly increasing ramp crossing the vertical seam left-to-right / right-to-left, 18 a constant plateau
    over the corner where the four tiles meet."""
    m = np.zeros((19, SEAM_H, SEAM_W), np.float32)
    near, far = [], []
    for i, d in enumerate(DIRS):
        a, b = _pair(R, d, R)
        m[i][a] = m[i][b] = 0.5
        near.append((a, b))
        a, b = _pair(R, d, R + 1)
        m[8 + i][a] = m[8 + i][b] = 0.5
        far.append((a, b))
    xs = np.arange(NMS_TW - 30, NMS_TW + 30)
    ramp = (np.arange(60, dtype=np.float32) + 1) / np.float32(61)
    m[16, 10, xs] = ramp
    m[17, 40, xs] = ramp[::-1]
    m[18, NMS_TH - 8:NMS_TH + 8, NMS_TW - 8:NMS_TW + 8] = 0.75
    return m, {"near": near, "far": far, "ramp_x": (int(xs[0]), int(xs[-1]))}


def row_ramp(H, W, y, x0, n):
    """one image, one strictly increasing run of n pixels along row y"""
    m = np.zeros((H, W), np.float32)
    m[y, x0:x0 + n] = (np.arange(n, dtype=np.float32) + 1) / np.float32(n + 1)
    return m


def nms_pass_count_batch(R):
    """B = 3, 24 x 160: isolated peaks (1 pass), a short ramp (4 passes), a long ramp (more than the 8 enqueued passes).  The
    ramp lengths follow from the radius: the chain of successive maxima advances R + 1 pixels per pass."""
    H, W = 24, 160
    m = np.zeros((3, H, W), np.float32)
    m[0, 5::11, 7::13] = 0.5
    m[1] = row_ramp(H, W, 12, 6, 3 * (R + 1) + 1)
    m[2] = row_ramp(H, W, 12, 6, 148)
    return m


def nms_sign_maps():
    """40 x 56, B = 2 each: name -> map.  What the kernels' old `centre > 0` term got wrong: a negative pixel or an exact zero
    can be the first maximum of its window and then sets its neighbours to 0."""
    H, W = 40, 56
    out = {}
    out["uniform(-1,0.05)"] = synth.uniform(5209, (2, H, W), -1.0, 0.05)
    out["all_negative"] = synth.uniform(5202, (2, H, W), -1.0, -0.01)
    z = synth.uniform(5203, (2, H, W), -1.0, -0.01)
    z[:, 14:24, 18:38] = 0.0
    out["negative_with_zero_block"] = z
    b = synth.uniform(5204, (2, H, W), -0.5, 0.1)
    b[:, :4] = b[:, -4:] = 0.0
    b[:, :, :4] = b[:, :, -4:] = 0.0
    out["mixed_with_zero_border"] = b
    p = synth.uniform01(5205, (2, H, W)).copy()
    inf = np.float32(np.inf)
    p[0, 7, 9] = p[0, 7, 12] = p[0, 30, 50] = inf   # two peaks of +inf inside one window at every radius >= 3: the first wins
    p[1, 0, 0] = p[1, 39, 55] = p[1, 20, 31] = p[1, 21, 30] = inf
    out["plus_inf_peaks"] = p
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


UNTRACKED_H, UNTRACKED_W = NMS_TH, NMS_TW * (NMS_FIN_MAXT + 1)  # 32 x 131136: 2049 tiles in one row


def nms_untracked_windows():
    """[(x0, crop [32,w])]: the three non-zero windows of the 2049-tile map, each a field of short ramps (more than 2 passes).
    First tile; across the seam between the last two tiles (2047 | 2048); ending in the map's last column.  The last two cannot
    both be 200 wide: a 200-column window that ends in the 64-column last tile crosses the 2047 | 2048 seam itself, so the third
    window takes the 40 columns that are left after a 16-column gap of zeros."""
    def field(w, seed):
        x = np.arange(w)
        base = ((x % 40) + 1).astype(np.float32) / np.float32(41)          # restarts every 40 columns
        rows = synth.uniform01(seed, (NMS_TH, 1)) * np.float32(1.0 / 64.0)  # distinct rows, slope kept
        f = (base[None, :] + rows).astype(np.float32)
        f[1::3] = 0.0
        return f
    seam = NMS_TW * NMS_FIN_MAXT  # first column of the last tile
    return [(0, field(200, 61)), (seam - 192, field(200, 62)), (UNTRACKED_W - 40, field(40, 63))]


# ------------------------------------------------------------------------------------------ selection inputs (radius 0)
def sparse_positive(seed, B, H, W, nz):
    """exactly nz distinct positive values per image, at random places"""
    N = H * W
    m = np.zeros((B, N), np.float32)
    order = np.argsort(synth.uniform01(seed, (B, N)), axis=1, kind="stable")
    vals = (np.float32(0.05) + np.float32(0.9) * (np.arange(nz, dtype=np.float32) + 1) / np.float32(nz + 1)).astype(np.float32)
    mix = np.argsort(synth.uniform01(seed + 1, (B, nz)), axis=1, kind="stable")
    for b in range(B):
        m[b, order[b, :nz]] = vals[mix[b]]
    return m.reshape(B, H, W)


def select_route(m):
    """per image of a batch whose base is 16-byte aligned (the GPU test asserts that on the device tensor): the load form of
    select_compact_kernel's sweep ('fast' = batched 16-byte loads, 'load4' = 16-byte loads with a scalar tail, 'scalar'), the
    list path ('lds' = candidates kept in LDS, 'generic' = dense map or negative values), and whether some wave's slice is empty"""
    B, Hp, Wp = m.shape
    N = Hp * Wp
    per_wave = (-(-N // SEL_WAVES) + SEL_SLICE - 1) // SEL_SLICE * SEL_SLICE
    out = []
    for b in range(B):
        aligned = (b * N * 4) % 16 == 0
        load = "fast" if (aligned and N % 4 == 0 and N >= 4) else ("load4" if aligned else "scalar")
        path = "generic" if (float(m[b].min()) < 0 or np.count_nonzero(m[b]) > SEL_LCAP) else "lds"
        out.append((load, path, (SEL_WAVES - 1) * per_wave >= N))
    return out


def select_cases():
    """name -> dict(map, top_k, det_thr, pads, ordering, route, facts...).  `route` names the branch of select_compact_kernel the
    case is built for; the tests assert the facts (`nz`, `N % 4`, sign, rank positions) on the map before comparing."""
    c = {}

    def add(name, m, top_k, det_thr=1.0, pads=(0, 0, 0, 0), ordering="yx", route="", loads=("fast",), paths=("lds",), **facts):
        facts.update(loads=list(loads), paths=list(paths))
        c[name] = dict(map=np.ascontiguousarray(m, np.float32), top_k=top_k, det_thr=det_thr, pads=pads, ordering=ordering, route=route, **facts)

    # candidate list exactly full / one over: image 0 stays on the LDS path, image 1 takes the generic one
    m = np.concatenate([sparse_positive(7001, 1, 96, 128, SEL_LCAP), sparse_positive(7003, 1, 96, 128, SEL_LCAP + 1)], 0)
    add("nz_6144_and_6145", m, 500, route="nz == SEL_LCAP keeps the LDS path, nz == SEL_LCAP + 1 is dense -> generic", nz=[SEL_LCAP, SEL_LCAP + 1],
        loads=("fast", "fast"), paths=("lds", "generic"))
    for N in (1, 2, 3, 4, 5, 255, 4095, 4096, 4097):
        u = synth.uniform01(7100 + N, (1, 1, N)) * np.float32(0.9) + np.float32(0.05)
        if N > 8:
            u[0, 0, ::3] = 0.0
        for k in sorted({0, 1, max(1, N // 2), N}):
            add(f"N{N}_k{k}", u, k, route="1 x N map: N < 4 scalar loads, N < 4096 leaves waves with an empty slice, N % 4 picks the load form", N=N,
                loads=("fast" if N % 4 == 0 else "load4",), empty_wave=N not in (4095, 4096))
    for H, W in ((5, 7), (9, 13), (33, 47)):
        u = synth.uniform01(7200 + H, (2, H, W)) ** 2
        u[synth.uniform01(7300 + H, (2, H, W)) < np.float32(0.5)] = 0.0
        add(f"misaligned_{H}x{W}", u, max(3, H * W // 10), route="N % 4 != 0: image 0 vector load4 with a scalar tail, image 1 misaligned -> scalar", n_mod4=(H * W) % 4,
            loads=("load4", "scalar"), paths=("lds", "lds"))
    s = sparse_positive(7400, 1, 24, 40, 40)
    N = 24 * 40
    for k in (0, 1, 39, 40, 41, N - 1, N, N + 5):
        add(f"sparse40_k{k}", s, k, route="lo < zeros when k > nz (threshold 0), rank on the first candidate at k == nz, k >= N -> 0", nz=[40])
    t = sparse_positive(7500, 1, 24, 40, 40)
    vals = np.sort(t[t > 0])
    kth = vals[-10]
    t[0, 0, :4] = kth  # with the original: five copies of the value at descending rank 10
    for k in (8, 10, 12, 14, 15):
        add(f"ties_at_kth_k{k}", t, k, route="sorted[lo] == sorted[hi] through duplicates; survivors are strictly above", kth=float(kth), copies=5)
    d = sparse_positive(7600, 1, 24, 40, 200)
    dv = np.sort(d[d > 0])
    qv = float(np.float32(dv[-50] - (dv[-50] - dv[-51]) * np.float32(0.5)))  # the midpoint quantile at k = 50 (lo, hi = the two values)
    for tag, thr in (("below", float(dv[-120])), ("equal", qv), ("above", float(dv[-20])), ("zero", 0.0)):
        add(f"det_thr_{tag}_quantile", d, 50, det_thr=thr, route="thr = min(quantile, det_thr)", quantile=qv)
    n = synth.uniform(7700, (2, 30, 44), -1.0, 1.0)
    add("negative_thr_below_zero", n, 1000, route="negative values -> generic path; thr < 0: nms keeps negatives, positions only v > 0", thr_negative=True,
        loads=("fast", "fast"), paths=("generic", "generic"))
    p = synth.uniform01(7800, (2, 40, 56)) ** 3
    p[synth.uniform01(7801, (2, 40, 56)) < np.float32(0.8)] = 0.0
    p[:, 2, 5] = p[:, 37, 51] = p[:, 20, 0] = p[:, 4, 30] = 0.99  # inside the pad margin: counted by the quantile, never output
    for o in ("yx", "xy"):
        add(f"lopsided_pads_{o}", p, 60, pads=(1, 7, 5, 3), ordering=o, route="crop after the threshold: margin pixels rank but are not listed",
            margin=[(2, 5), (37, 51), (20, 0), (4, 30)], loads=("fast", "fast"), paths=("lds", "lds"))
        add(f"dense_generic_{o}", synth.uniform01(7900, (1, 90, 100)), 300, pads=(1, 7, 5, 3), ordering=o, route="nz > SEL_LCAP -> generic path with pads",
            paths=("generic",))
    v = synth.uniform01(7950, (1, 32, 64)) ** 2
    v[synth.uniform01(7951, (1, 32, 64)) < np.float32(0.7)] = 0.0
    add("view_32x64", v, 40, route="N % 4 == 0: batched loads from an aligned base; read through a view one float off it: scalar loads")
    add("cap_below_survivors", sparse_positive(7990, 2, 24, 40, 40), 0, det_thr=0.0, route="40 survivors per image for 16 rows", nz=[40, 40],
        loads=("fast", "fast"), paths=("lds", "lds"))
    return c


def check_select_facts(c, nms, pos, thr):
    """the properties a selection case is built for, asserted on its input and on the reference's result (nms cropped, positions
    list, thr) before any kernel output is looked at"""
    m = c["map"]
    B, Hp, Wp = m.shape
    N = Hp * Wp
    if "loads" in c:
        route = select_route(m)
        assert [r[0] for r in route] == c["loads"] and [r[1] for r in route] == c["paths"], (route, c["route"])
        if "empty_wave" in c:
            assert route[0][2] == c["empty_wave"]
    if "nz" in c:
        assert nz_per_image(m) == c["nz"]
    if "N" in c:
        assert N == c["N"] and Hp == 1
    if "n_mod4" in c:
        assert N % 4 == c["n_mod4"] != 0 and B == 2
    if c.get("thr_negative"):
        assert sign_of(m) == "mixed" and (thr < 0).all() and (nms < 0).any() and all((p[:, 2] > 0).all() for p in pos)
    else:
        assert sign_of(m) == "nonneg"
    if "kth" in c:
        assert int((m == np.float32(c["kth"])).sum()) == c["copies"]
        assert all((p[:, 2] > thr[b]).all() for b, p in enumerate(pos))
    if "quantile" in c:
        assert thr[0] == min(np.float32(c["quantile"]), np.float32(c["det_thr"])), (thr, c["quantile"], c["det_thr"])
    if "margin" in c:
        w0, w1, h0, h1 = c["pads"]
        for y, x in c["margin"]:
            assert not (h0 <= y < Hp - h1 and w0 <= x < Wp - w1) and (m[:, y, x] > thr).all(), "a survivor inside the pad margin"
        assert all(len(p) < int((m[b] > thr[b]).sum()) for b, p in enumerate(pos))
