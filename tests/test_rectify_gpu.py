"""GPU tests (-m gpu), component: rectification of raw recordings (datasets/rectify.py, csrc/rectify.hip) against the
float64 numpy restatement of tests/rectify_ref.py.

Bounds, and where each comes from:
  maps            1 float32 ulp: the kernels compute in float64 what the restatement computes in float64, so the two float32
                  results can differ only where a last-place difference of atan / sqrt / the division crosses a float32
                  rounding boundary (a double rounding).  The share of pixels that are not bit-equal is printed.
  rounded EC map  exact: no restated coordinate lies within 1e-9 of a half-integer (asserted; the nearest is 2.0e-6).
  remap, float32  |gpu - f64| <= 16 * 2^-24 * max|I|: the stated operation order has at most 12 roundings of values of
                  magnitude <= 2 max|I| (fx, fy, three differences, three products, three sums).
  remap, uint8    equal, except where the float64 value lies within 16 * 2^-24 * 255 of a half-integer (there rint may fall
                  either way: a difference of 1), and those pixels must stay below 1 % of the frame.
  events          bit for bit, counts included: a gather, two comparisons and a stable compaction have no rounding.

The identity calibration gives identity maps exactly for the radial-tangential builders.  For the fisheye builder it cannot: with
D = 0 the model is still the equidistant projection r -> atan(r), so that case is held to the 1-ulp bound like the others, and
only the principal point (r == 0, s = 1) is exact."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import rectify_ref as ref
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu

N = pkg.native
L = N.lib()
rectify = import_module(pkg.__name__ + ".datasets.rectify")
rep = import_module(pkg.__name__ + ".datasets.representations")
CHUNK = L.einx_events_remap_chunk()
GUARD = 1024  # elements behind every output array, bytes behind the workspace
EPS = 2.0 ** -24


# ---- maps -------------------------------------------------------------------------------------------------------------------
def _within_one_ulp(tag, got, exp64):
    exp = exp64.astype(np.float32)
    with np.errstate(all="ignore"):
        up, down = np.nextafter(exp, np.float32(np.inf)), np.nextafter(exp, np.float32(-np.inf))
    same = (got == exp) | (np.isnan(got) & np.isnan(exp))
    ok = same | (got == up) | (got == down)
    print(f"{tag}: {1.0 - same.mean():.3e} of {got.size} pixels not bit-equal, worst |diff| {np.nanmax(np.abs(got.astype(np.float64) - exp64)):.3e}")
    assert ok.all(), f"{tag}: {int((~ok).sum())} pixels differ by more than 1 float32 ulp"


_ROT = lambda a: np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])  # noqa: E731
FISHEYE_CASES = {
    "mvsec": (ref.MVSEC_K, ref.MVSEC_D, ref.MVSEC_R, ref.MVSEC_P, ref.MVSEC_SIZE),
    "mvsec_3x3_P": (ref.MVSEC_K, ref.MVSEC_D, ref.MVSEC_R, ref.MVSEC_P[:, :3], ref.MVSEC_SIZE),
    "small": (ref.MVSEC_K, ref.MVSEC_D, ref.MVSEC_R, ref.MVSEC_P, ref.SMALL_SIZE),
    "behind_the_camera": ((4.0, 4.0, 6.0, 3.0), ref.MVSEC_D, _ROT(1.4), ref.camera_matrix((4.0, 4.0, 6.0, 3.0)), ref.SMALL_SIZE),
    "identity": (ref.IDENTITY_K, (0.0,) * 4, np.eye(3), np.eye(3), ref.SMALL_SIZE),
}


@pytest.mark.parametrize("name", list(FISHEYE_CASES))
def test_fisheye_map(name):
    K, D, R, P, size = FISHEYE_CASES[name]
    mx, my = rectify.fisheye_rectify_map(K, D, R, P, size, device=DEV)
    ex, ey = ref.fisheye_map(K, D, R, P, size)
    assert mx.shape == (size[1], size[0]) and mx.dtype == torch.float32 and my.shape == mx.shape
    _within_one_ulp(f"fisheye {name} x", _np(mx), ex)
    _within_one_ulp(f"fisheye {name} y", _np(my), ey)
    if name == "behind_the_camera":  # both outcomes of the Wd <= 0 rule occur
        assert (ex == -1.0).any() and (ex != -1.0).any() and np.array_equal(_np(mx) == -1.0, ex == -1.0)
    if name == "identity":
        assert float(mx[0, 0]) == 0.0 and float(my[0, 0]) == 0.0  # the principal point: r == 0, s = 1


RADTAN_CASES = {
    "ec_undistort": (ref.EC_K, ref.EC_D, ref.EC_SIZE, None, None),
    "ec_rectify": (ref.EC_K, ref.EC_D, ref.EC_SIZE, ref.MVSEC_R, ref.MVSEC_P),
    "ec_k3": (ref.EC_K, (-0.368436, 0.150947, -0.000296, -0.000439, -0.02), ref.EC_SIZE, None, None),
    "small": (ref.EC_K, ref.EC_D, ref.SMALL_SIZE, None, None),
}


@pytest.mark.parametrize("name", list(RADTAN_CASES))
def test_radtan_map(name):
    K, D, size, R, P = RADTAN_CASES[name]
    mx, my = rectify.radtan_rectify_map(ref.camera_matrix(K) if name == "small" else K, D, size, R=R, P=P, device=DEV)
    ex, ey = ref.radtan_map(K, D, size, R, P)
    _within_one_ulp(f"radtan {name} x", _np(mx), ex)
    _within_one_ulp(f"radtan {name} y", _np(my), ey)


@pytest.mark.parametrize("size", [ref.EC_SIZE, ref.SMALL_SIZE], ids=["ec", "small"])
@pytest.mark.parametrize("iters", [5, 0, 20])
def test_undistort_points_map_unrounded(size, iters):
    mx, my = rectify.radtan_undistort_points_map(ref.EC_K, ref.EC_D, size, iters=iters, rint=False, device=DEV)
    ex, ey = ref.undistort_points_map(ref.EC_K, ref.EC_D, size, iters=iters, rint=False)
    _within_one_ulp(f"points {size} iters {iters} x", _np(mx), ex)
    _within_one_ulp(f"points {size} iters {iters} y", _np(my), ey)


def test_undistort_points_map_with_a_projection():
    mx, my = rectify.radtan_undistort_points_map(ref.EC_K, ref.EC_D, ref.EC_SIZE, P=ref.MVSEC_P, rint=False, device=DEV)
    ex, ey = ref.undistort_points_map(ref.EC_K, ref.EC_D, ref.EC_SIZE, P=ref.MVSEC_P, rint=False)
    _within_one_ulp("points with P x", _np(mx), ex)
    _within_one_ulp("points with P y", _np(my), ey)


def test_rounded_ec_map_is_exact():
    """rectify_ec.py:70-78 per pixel.  Precondition: the float64 coordinates keep 1e-9 from every half-integer, so that rint of
    the kernel's float64 value and of the restatement's cannot differ; then the gate is equality."""
    ux, uy = ref.undistort_points_map(ref.EC_K, ref.EC_D, ref.EC_SIZE, rint=False)
    gap = min(np.abs(ux - np.floor(ux) - 0.5).min(), np.abs(uy - np.floor(uy) - 0.5).min())
    assert gap > 1e-9, gap
    ex, ey = ref.undistort_points_map(ref.EC_K, ref.EC_D, ref.EC_SIZE)
    mx, my = rectify.radtan_undistort_points_map(ref.EC_K, ref.EC_D, ref.EC_SIZE, device=DEV)
    assert np.array_equal(_np(mx), ex.astype(np.float32)) and np.array_equal(_np(my), ey.astype(np.float32))
    W, H = ref.EC_SIZE
    share = ((ex >= 0) & (ex < W) & (ey >= 0) & (ey < H)).mean()
    print(f"nearest half-integer {gap:.3e}; {share:.3f} of the pixels stay in bounds")
    assert 0.5 < share < 0.95  # both outcomes of the EC filter occur


def test_identity_calibration_gives_identity_maps():
    for size in (ref.SMALL_SIZE, ref.EC_SIZE):
        W, H = size
        u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
        for mx, my in (rectify.radtan_rectify_map(ref.IDENTITY_K, (0,) * 5, size, device=DEV),
                       rectify.radtan_rectify_map(np.eye(3), (0,) * 5, size, R=np.eye(3), P=np.eye(3, 4), device=DEV),
                       rectify.radtan_undistort_points_map(ref.IDENTITY_K, (0,) * 5, size, rint=False, device=DEV),
                       rectify.radtan_undistort_points_map(ref.IDENTITY_K, (0,) * 5, size, device=DEV)):
            assert np.array_equal(_np(mx), u) and np.array_equal(_np(my), v)


# ---- frames -----------------------------------------------------------------------------------------------------------------
def _edge_map(rng, Hs, Ws, H, W):
    """positions all over and around an Hs x Ws source: random ones reaching 2 px outside, the four corners, the last row and
    column exactly, positions outside every border, integers, and entries that are not finite"""
    mx = rng.uniform(-2.0, Ws + 1.0, (H, W)).astype(np.float32)
    my = rng.uniform(-2.0, Hs + 1.0, (H, W)).astype(np.float32)
    # (fractional parts drawn at random: between integer grey values 0.5, 0.25 or 0.3 would plant exact rounding ties)
    f = rng.uniform(0.05, 0.95, 8).round(6)
    special = [(0.0, 0.0), (Ws - 1.0, Hs - 1.0), (Ws - 1.0, f[0]), (f[1], Hs - 1.0), (Ws - f[2], 1.0), (1.0, Hs - f[3]), (-f[4], -f[5]), (-1.0, 2.0),
               (2.0, -1.0), (float(Ws), 1.0), (1.0, float(Hs)), (-7.0, 2.0), (3.0, 1e9), (-1e30, 0.0), (np.nan, 1.0), (1.0, np.nan),
               (np.inf, 1.0), (1.0, -np.inf), (2.0, 3.0), (-1e-10, 1.0 + f[6]), (1.0 + f[7], -1e-10)]
    flat = rng.permutation(H * W)[:len(special)]
    for k, (a, b) in zip(flat, special):
        mx.flat[k], my.flat[k] = a, b
    return mx, my


def _check_remap(tag, src, mx, my, got):
    exp = ref.remap(src, mx, my)
    if src.dtype == np.float32:
        bound = 16 * EPS * float(np.abs(src).max())
        err = float(np.abs(got.astype(np.float64) - exp).max())
        print(f"{tag}: max |gpu - f64| {err:.3e}, bound {bound:.3e}")
        assert got.dtype == np.float32 and err <= bound
    else:
        want = np.clip(np.rint(exp), 0, 255)
        near_tie = np.abs(exp - np.floor(exp) - 0.5) <= 16 * EPS * 255
        diff = np.abs(got.astype(np.float64) - want)
        print(f"{tag}: {int((diff != 0).sum())} of {got.size} pixels differ, {near_tie.mean():.3e} of them lie on a rounding tie")
        assert got.dtype == np.uint8 and (diff[~near_tie] == 0).all() and (diff <= 1).all()
        assert near_tie.mean() <= 0.01


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_remap_small_source_into_a_map_of_another_size(dtype):
    rng = np.random.default_rng(5)
    Hs, Ws, H, W = 7, 13, 5, 9
    mx, my = _edge_map(rng, Hs, Ws, H, W)
    src = rng.integers(0, 256, (3, Hs, Ws)).astype(dtype) if dtype == np.uint8 else rng.normal(0.0, 40.0, (3, Hs, Ws)).astype(np.float32)
    got = rectify.remap(src, _t(mx), _t(my))
    assert got.shape == (3, H, W) and got.device == torch.device(DEV)
    _check_remap(f"7x13 -> 5x9 {dtype.__name__}", src, mx, my, _np(got))
    # one frame without the leading axis; a device tensor is used as it is; a non-contiguous one is copied (documented)
    one = rectify.remap(src[1], _t(mx), _t(my))
    assert one.shape == (H, W) and torch.equal(one, got[1])
    wide = _t(np.concatenate([src, src], axis=2))
    assert not wide[:, :, :Ws].is_contiguous()
    assert torch.equal(rectify.remap(wide[:, :, :Ws], _t(mx), _t(my)), got)


@pytest.fixture(scope="module")
def mvsec_maps():
    mx, my = rectify.fisheye_rectify_map(ref.MVSEC_K, ref.MVSEC_D, ref.MVSEC_R, ref.MVSEC_P, ref.MVSEC_SIZE, device=DEV)
    return mx, my, _np(mx), _np(my)


@pytest.mark.parametrize("F", [1, 3, 29])  # 29: more frames than the launch has frame slices at this size, so threads walk frames
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_remap_full_frames(mvsec_maps, dtype, F):
    mx, my, hx, hy = mvsec_maps
    W, H = ref.MVSEC_SIZE
    rng = np.random.default_rng(7 + F)
    src = rng.integers(0, 256, (F, H, W)).astype(dtype) if dtype == np.uint8 else rng.uniform(0.0, 255.0, (F, H, W)).astype(np.float32)
    _check_remap(f"260x346 F={F} {dtype.__name__}", src, hx, hy, _np(rectify.remap(src, mx, my)))


def test_remap_with_the_identity_map_copies_the_frames():
    W, H = ref.SMALL_SIZE
    mx, my = rectify.radtan_rectify_map(ref.IDENTITY_K, (0,) * 5, ref.SMALL_SIZE, device=DEV)
    src = np.random.default_rng(2).integers(0, 256, (2, H, W)).astype(np.uint8)
    assert np.array_equal(_np(rectify.remap(src, mx, my)), src)
    assert np.array_equal(_np(rectify.remap(src.astype(np.float32), mx, my)), src.astype(np.float32))


# ---- events -----------------------------------------------------------------------------------------------------------------
EH, EW = 37, 53
PATTERNS = ("all", "none", "first", "last", "alternating", "random70")


@pytest.fixture(scope="module")
def event_map():
    """a map whose kept / dropped pixels are known per rule: positions inside the bounds on the even-parity pixels, and on the odd
    ones every way of leaving them (negative, beyond, NaN, infinite; in x or in y).  Some even-parity pixels map EXACTLY to
    W - 1 or H - 1: kept under the EC rule, dropped under MVSEC's.  The last row and column are in both classes."""
    rng = np.random.default_rng(11)
    oy, ox = np.meshgrid(np.arange(EH), np.arange(EW), indexing="ij")
    mx = rng.uniform(0.0, EW - 1.001, (EH, EW)).astype(np.float32)
    my = rng.uniform(0.0, EH - 1.001, (EH, EW)).astype(np.float32)
    mx[0, 0], my[0, 0] = 0.0, 0.0  # the lower bounds are inclusive
    mx[2, 4], my[4, 2] = EW - 1.0, EH - 1.0  # on the MVSEC bound exactly
    mx[6, 6], my[6, 6] = np.nextafter(np.float32(EW - 1), np.float32(0)), np.nextafter(np.float32(EH - 1), np.float32(0))
    odd = (ox + oy) % 2 == 1
    ways = [(-0.25, 3.0), (3.0, -0.25), (float(EW), 3.0), (3.0, float(EH)), (np.nan, 3.0), (3.0, np.nan), (np.inf, 3.0), (3.0, -np.inf),
            (-1.0, -1.0), (EW + 40.0, 1.0), (-0.0 - 1e-30, 2.0)]
    pick = rng.integers(0, len(ways), (EH, EW))
    for k, (a, b) in enumerate(ways):
        sel = odd & (pick == k)
        mx[sel], my[sel] = a, b
    return mx, my, _t(mx), _t(my)


@functools.lru_cache(maxsize=2)
def _draws(n, seed):
    """the random part of a stream of n events, shared by the keep patterns: pool indices, jitter kinds, stamps (with runs of
    equal ones), polarities and the 70 % coin"""
    rng = np.random.default_rng(seed)
    t = 1.5e9 + np.cumsum(np.repeat(rng.uniform(1e-6, 1e-4, (n + 2) // 3), 3)[:n] * (rng.random(n) < 0.6))
    return (rng.integers(0, 1 << 30, n), rng.integers(0, 1 << 30, n), rng.integers(0, 5, n), rng.integers(0, 5, n), t.astype(np.float64),
            rng.integers(0, 2, n).astype(np.float32), rng.random(n) < 0.7)


def _events(n, pattern, mx, my, seed):
    """n time-sorted raw events whose kept / dropped sequence follows `pattern` under BOTH rules (kept ones from the pixels MVSEC's
    rule keeps, dropped ones from those EC's rule drops; the pixels on which the rules differ: test_events_remap_rules_differ).  Raw
    coordinates are the target pixel, the pixel +- 0.25, or (even pixels) the pixel +- 0.5: half-integers, which round half to
    even onto it."""
    with np.errstate(invalid="ignore"):
        good = (mx >= 0) & (mx < np.float32(EW - 1)) & (my >= 0) & (my < np.float32(EH - 1))
        bad = ~((mx >= 0) & (mx < np.float32(EW)) & (my >= 0) & (my < np.float32(EH)))
    gy, gx = np.nonzero(good)
    by, bx = np.nonzero(bad)
    # the last row and the last column are in both pools
    assert (gx == EW - 1).any() and (gy == EH - 1).any() and (bx == EW - 1).any() and (by == EH - 1).any()
    g, b, kx, ky, t, p, coin = _draws(n, seed)
    idx = np.arange(n)
    keep = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": idx == 0, "last": idx == n - 1, "alternating": idx % 2 == 0,
            "random70": coin}[pattern]
    px = np.where(keep, gx[g % len(gx)], bx[b % len(bx)])
    py = np.where(keep, gy[g % len(gy)], by[b % len(by)])
    shift = np.array([0.0, 0.25, -0.25, 0.5, -0.5], np.float32)

    def jitter(c, kind):
        kind = np.where((kind >= 3) & (c % 2 == 1), 0, kind)  # a half-integer next to an odd pixel rounds away from it
        return c.astype(np.float32) + shift[kind]

    return jitter(px, kx), jitter(py, ky), t, p, keep


SENT_F, SENT_I = np.float32(-12345.5), np.int64(-0x0123456789ABCDEF)


def _guarded_out(n):
    """output arrays of n elements, each with GUARD more behind it, all filled with a sentinel; `head` as _native.events_remap lays
    it out (two counts, then out_t's storage)"""
    fs = [torch.full((n + GUARD,), float(SENT_F), dtype=torch.float32, device=DEV) for _ in range(3)]
    head = torch.full((2 + n + GUARD,), int(SENT_I), dtype=torch.int64, device=DEV)
    return fs, head, (fs[0][:n], fs[1][:n], head[2:2 + n].view(torch.float64), fs[2][:n], head[:2 + n])


@pytest.fixture
def ws_guards(monkeypatch):
    made = []

    def guarded(nbytes, device):
        nbytes = int(nbytes)
        buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=device)
        buf[nbytes:] = 0xA5
        made.append((nbytes, buf[nbytes:]))
        return buf[:nbytes]

    monkeypatch.setattr(N, "_workspace", guarded)
    return made


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


def _run_and_check(tag, x, y, t, p, hmx, hmy, dmx, dmy, bounds, ws_guards, dev=None):
    n = len(t)
    dx, dy, dt, dp = dev if dev is not None else (_t(x), _t(y), _t(t), _t(p))
    ex, ey, et, ep, kept, outside = ref.rectify_events(x, y, t, p, hmx, hmy, *bounds)
    results = []
    for _ in range(2):  # the same call twice: the same bits
        fs, head, out = _guarded_out(n)
        before = len(ws_guards)
        N.events_remap(dx, dy, dt, dp, dmx, dmy, *bounds, out=out)
        torch.cuda.synchronize()
        assert len(ws_guards) == before + 1 and ws_guards[-1][0] == L.einx_events_remap_ws_bytes(n)
        assert int((ws_guards[-1][1] != 0xA5).sum()) == 0, f"{tag}: the guard behind the workspace was overwritten"
        h = _np(head)
        assert (int(h[0]), int(h[1])) == (kept, outside), f"{tag}: counts {h[:2]} expected {(kept, outside)}"
        gx, gy, gp = (_np(f) for f in fs)
        gt = h[2:].view(np.float64)
        for name, got, exp in (("x", gx, ex), ("y", gy, ey), ("p", gp, ep), ("t", gt, et)):
            assert np.array_equal(_bits(got[:kept]), _bits(exp)), f"{tag}: {name} differs"
        # nothing behind the kept events is written: neither the rest of the N elements nor the guard
        for got in (gx, gy, gp):
            assert (got[kept:] == SENT_F).all(), f"{tag}: an output array was written behind its {kept} kept events"
        assert (h[2 + kept:] == SENT_I).all(), f"{tag}: out_t was written behind its {kept} kept events"
        assert (np.diff(gt[:kept]) >= 0).all()
        results.append((gx[:kept].copy(), gy[:kept].copy(), gt[:kept].copy(), gp[:kept].copy()))
    for a, b in zip(*results):
        assert np.array_equal(_bits(a), _bits(b))
    return kept


SIZES = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 100003, 3000001]


@pytest.mark.parametrize("n", SIZES)
def test_events_remap_bit_equal(event_map, ws_guards, n):
    """every keep pattern under both bound rules; 3000001 events are 1465 workgroups, more than one scan tile of 1024"""
    hmx, hmy, dmx, dmy = event_map
    seen = set()
    for pattern in PATTERNS:
        x, y, t, p, keep = _events(n, pattern, hmx, hmy, seed=100 + n % 7)
        dev = (_t(x), _t(y), _t(t), _t(p))  # one upload for both rules
        for rule in ("mvsec", "ec"):
            kept = _run_and_check(f"n={n} {rule} {pattern}", x, y, t, p, hmx, hmy, dmx, dmy, rectify._bounds(rule, EH, EW), ws_guards, dev=dev)
            assert kept == int(keep.sum())
            seen.add(kept)
    if n > 2:
        assert {0, 1, n, (n + 1) // 2} <= seen


def test_events_remap_rules_differ_on_the_bound(event_map, ws_guards):
    """pixels that map exactly to W - 1 or H - 1, half-integer raw coordinates (0.5 -> 0, 1.5 -> 2, 2.5 -> 2) and -0.5 -> -0"""
    hmx, hmy, dmx, dmy = event_map
    x = np.array([4.0, 2.0, 6.0, 0.5, 1.5, 2.5, -0.5, EW - 1.0, 3.5, 4.5], np.float32)
    y = np.array([2.0, 4.0, 6.0, 0.5, 2.5, 1.5, -0.5, EH - 1.0, 0.5, 3.5], np.float32)
    t = np.arange(len(x), dtype=np.float64)
    p = np.ones(len(x), np.float32)
    kept = {}
    for rule in ("mvsec", "ec", (10.5, 20.25)):
        bounds = rectify._bounds(rule, EH, EW)
        kept[rule] = _run_and_check(f"bound {rule}", x, y, t, p, hmx, hmy, dmx, dmy, bounds, ws_guards)
    assert kept["ec"] == kept["mvsec"] + 2  # (4, 2) and (2, 4): on MVSEC's bound exactly


def test_events_remap_unaligned_arrays(event_map, ws_guards):
    """arrays that do not start on a 16-byte boundary take the element-wise loads: the same result"""
    hmx, hmy, dmx, dmy = event_map
    n = 3 * CHUNK + 17
    bounds = rectify._bounds("mvsec", EH, EW)
    x, y, t, p, _ = _events(n, "random70", hmx, hmy, seed=9)
    pad = lambda a, k: _t(np.concatenate([np.zeros(k, a.dtype), a]))[k:]  # noqa: E731
    dev = (pad(x, 1), pad(y, 3), pad(t, 1), pad(p, 2))
    assert any(d.data_ptr() % 16 for d in dev)
    _run_and_check("unaligned", x, y, t, p, hmx, hmy, dmx, dmy, bounds, ws_guards, dev=dev)


def test_events_remap_graph_replay(event_map):
    hmx, hmy, dmx, dmy = event_map
    n = 100003
    bounds = rectify._bounds("ec", EH, EW)
    x, y, t, p, _ = _events(n, "random70", hmx, hmy, seed=21)
    ex, ey, et, ep, kept, outside = ref.rectify_events(x, y, t, p, hmx, hmy, *bounds)
    dev = (_t(x), _t(y), _t(t), _t(p))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        eager = N.events_remap(*dev, dmx, dmy, *bounds)  # warm-up on the capture stream
    stream.synchronize()
    fs, head, out = _guarded_out(n)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        N.events_remap(*dev, dmx, dmy, *bounds, out=out)
    for _ in range(2):
        head.fill_(int(SENT_I))
        for f in fs:
            f.fill_(float(SENT_F))
        graph.replay()
        torch.cuda.synchronize()
        h = _np(head)
        assert (int(h[0]), int(h[1])) == (kept, outside)
        for got, exp, first in ((_np(fs[0]), ex, eager[0]), (_np(fs[1]), ey, eager[1]), (_np(fs[2]), ep, eager[3]),
                                (h[2:].view(np.float64), et, eager[2])):
            assert np.array_equal(_bits(got[:kept]), _bits(exp)) and np.array_equal(_bits(got[:kept]), _bits(_np(first)[:kept]))
        assert (_np(fs[0])[kept:] == SENT_F).all() and (h[2 + kept:] == SENT_I).all()


def test_rectify_events_public_entry(event_map):
    """a dict of numpy arrays (uploaded once) and a resident EventSequence give the same RectifiedSequence: kept / dropped, the
    device arrays, and t_host from the one read-back"""
    hmx, hmy, dmx, dmy = event_map
    n = 5 * CHUNK + 5
    bounds = rectify._bounds("mvsec", EH, EW)
    x, y, t, p, _ = _events(n, "random70", hmx, hmy, seed=33)
    ex, ey, et, ep, kept, _ = ref.rectify_events(x, y, t, p, hmx, hmy, *bounds)
    raw = {"x": x.astype(np.float64), "y": y, "t": t, "p": p.astype(np.int8)}
    a = rectify.rectify_events(raw, dmx, dmy, "mvsec")
    b = pkg.EventSequence(raw, device=DEV).rectified(dmx, dmy, "mvsec")
    c = rectify.rectify_events(pkg.EventSequence(raw, device=DEV), dmx, dmy, bounds)
    for seq in (a, b, c):
        assert isinstance(seq, pkg.EventSequence) and len(seq) == kept and (seq.kept, seq.dropped) == (kept, n - kept)
        assert seq.t_host.dtype == np.float64 and np.array_equal(_bits(seq.t_host), _bits(et))
        for name, exp in (("x", ex), ("y", ey), ("t", et), ("p", ep)):
            got = getattr(seq, name)
            assert got.is_contiguous() and got.shape == (kept,) and np.array_equal(_bits(_np(got)), _bits(exp)), name
    empty = rectify.rectify_events({k: v[:0] for k, v in raw.items()}, dmx, dmy, "ec")
    assert len(empty) == 0 and (empty.kept, empty.dropped) == (0, 0) and len(empty.windows([1.0], 1.0)) == 1


def test_default_devices_meet(event_map):
    """the documented chain with every `device` argument left at its default: EventSequence(...) stores an un-indexed "cuda", the
    builders' maps and any `.cuda()` tensor lie on "cuda:0"; that is one device, not two"""
    hmx, hmy, _, _ = event_map
    x, y, t, p, _ = _events(3 * CHUNK + 1, "random70", hmx, hmy, seed=5)
    raw = {"x": x, "y": y, "t": t, "p": p}
    ex, ey, et, ep, kept, _ = ref.rectify_events(x, y, t, p, hmx, hmy, EW - 1.0, EH - 1.0)
    seq = pkg.EventSequence(raw)
    for got in (seq.rectified(torch.from_numpy(hmx).cuda(), torch.from_numpy(hmy).cuda(), "mvsec"),
                rectify.rectify_events(pkg.EventSequence.from_tensors(seq.x, seq.y, seq.t, seq.p), torch.from_numpy(hmx).cuda(),
                                       torch.from_numpy(hmy).cuda(), "mvsec")):
        assert got.kept == kept and np.array_equal(_bits(_np(got.x)), _bits(ex)) and np.array_equal(_bits(got.t_host), _bits(et))
        assert len(got.windows([et[-1]], 1.0)) == 1
    mx, my = rectify.radtan_undistort_points_map(ref.EC_K, ref.EC_D, ref.EC_SIZE)  # default device
    ec = pkg.EventSequence({"x": x + 90, "y": y + 70, "t": t, "p": p}).rectified(mx, my, "ec")  # the middle of the EC sensor
    assert 0 < ec.kept <= len(x) and ec.x.device == mx.device
    fx, fy = rectify.fisheye_rectify_map(ref.MVSEC_K, ref.MVSEC_D, ref.MVSEC_R, ref.MVSEC_P, ref.SMALL_SIZE)
    rx, ry = rectify.radtan_rectify_map(ref.EC_K, ref.EC_D, ref.SMALL_SIZE)
    assert fx.device == rx.device == mx.device and rectify.remap(np.zeros((7, 13), np.uint8), fx, fy).device == mx.device


def test_rectify_events_refuses_coordinates_outside_the_map(event_map):
    """one coordinate equal to W, one negative, one NaN: numpy would raise for the first and WRAP the second; all three are refused"""
    hmx, hmy, dmx, dmy = event_map
    x = np.full(200, 3.0, np.float32)
    y = np.full(200, 3.0, np.float32)
    x[17], x[90], y[150] = float(EW), -1.0, np.nan
    ev = {"x": x, "y": y, "t": np.arange(200.0), "p": np.ones(200, np.float32)}
    with pytest.raises(IndexError, match=r"\b3 of 200 events"):
        rectify.rectify_events(ev, dmx, dmy, "ec")
    *_, kept, outside = ref.rectify_events(x, y, ev["t"], ev["p"], hmx, hmy, float(EW), float(EH))
    assert outside == 3
    x[17], x[90], y[150] = EW - 0.51, -0.5, EH - 1.0  # the nearest coordinates that ARE pixels of the map
    assert len(rectify.rectify_events(ev, dmx, dmy, "ec")) == ref.rectify_events(x, y, ev["t"], ev["p"], hmx, hmy, float(EW), float(EH))[4]


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_raw_recording_to_voxel_grids_on_the_device():
    """raw events -> EventSequence.rectified -> windows by timestamp -> VoxelGrid, all on the device, against the numpy-rectified
    events taken through the existing packed path: the same bits"""
    W, H = ref.EC_SIZE
    rng = np.random.default_rng(41)
    n = 60000
    raw = {"x": rng.integers(0, W, n).astype(np.int16), "y": rng.integers(0, H, n).astype(np.int16),
           "t": 1.5e9 + np.cumsum(rng.uniform(1e-6, 1e-5, n)), "p": rng.integers(0, 2, n).astype(np.int8)}
    mx, my = rectify.radtan_undistort_points_map(ref.EC_K, ref.EC_D, ref.EC_SIZE, device=DEV)
    hx, hy = (m.astype(np.float32) for m in ref.undistort_points_map(ref.EC_K, ref.EC_D, ref.EC_SIZE))
    seq = pkg.EventSequence(raw, device=DEV).rectified(mx, my, "ec")
    ex, ey, et, ep, kept, outside = ref.rectify_events(raw["x"], raw["y"], raw["t"], raw["p"], hx, hy, float(W), float(H))
    assert outside == 0 and 0 < kept < n and (seq.kept, seq.dropped) == (kept, n - kept)
    stamps = raw["t"][[5000, 20000, 20000, 59999]]
    win = seq.windows(stamps, 0.05)
    host = pkg.EventSequence({"x": ex, "y": ey, "t": et, "p": ep}, device="cpu").windows(stamps, 0.05)
    assert np.array_equal(win.begin, host.begin) and np.array_equal(win.end, host.end) and win.total > 1000
    size = (5, H, W)
    got = rep.events_to_voxel_grid_batch(win, size)
    exp = rep.events_to_voxel_grid_batch(host.events_list(), size, device=DEV)
    assert np.array_equal(_bits(_np(got)), _bits(_np(exp))) and float(got.abs().sum()) > 0
