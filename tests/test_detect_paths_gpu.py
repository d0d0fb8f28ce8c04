"""GPU tests (-m gpu), component: detect.  One row per path of csrc/detect.hip's NMS, selection and border kernels, on inputs
constructed to take that path: every row first asserts the property of its input that routes it, then compares the kernels' result
by value with tests/detect_ref.py (NumPy / torch CPU; checked three ways against the C oracle in test_detect_paths_cpu.py).
The sign of a zero is not compared (the kernels keep a suppressed -0.0, the reference writes +0.0); NaN scores are out of scope."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import detect_ref as dr
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu

N = pkg.native
du = import_module(pkg.__name__ + ".core.modules.utils.detector_util")
NEG_INF = float("-inf")

_REF = {}


def _nms_ref(key, build, R):
    """(input, expected map, passes) of one constructed input, computed once per session"""
    if (key, R) not in _REF:
        m = build()
        _REF[key, R] = (m,) + dr.nms_ref(m, R)
    return _REF[key, R]


def _nms_only(m, R, iters):
    return N.detect(_t(m), top_k=0, radius=R, det_thr=NEG_INF, cap=1, nms_iters=iters)


def _check_nms(m, R, exp, budgets=(8,)):
    """radius 4 finishes on the device whatever the wide-pass budget; the other radii converge through the helper's x4 retry"""
    if R == 4:
        for iters in budgets:
            d = _nms_only(m, R, iters)
            assert _np(d.not_converged).tolist() == [0] * m.shape[0], iters
            assert np.array_equal(_np(d.nms), exp), iters
    got = du.fast_nms(_t(m)[:, None], R)
    assert np.array_equal(_np(got)[:, 0], exp)


# ------------------------------------------------------------------ NMS: sizes, seams and stores
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("H,W,route,cond", dr.NMS_SIZES, ids=[f"{h}x{w}" for h, w, _, _ in dr.NMS_SIZES])
def test_nms_sizes_and_stores(H, W, route, cond, R):
    assert cond(H, W), route
    m, exp, passes = _nms_ref(("size", H, W), lambda: dr.nms_size_map(H, W), R)
    assert dr.sign_of(m) == "nonneg"
    _check_nms(m, R, exp, budgets=(1, 2, 8))


@pytest.mark.parametrize("R", [2, 4])
def test_nms_tile_seams(R):
    """pairs, ramps and a plateau across the seams of a 2 x 2 tile map: the value halo is 2R, the is-max halo R, and with a budget
    of one wide pass the radius-4 finisher has to carry changes from a tile to its neighbours through its dirty-tile tracking"""
    m, exp, passes = _nms_ref("seams", lambda: dr.nms_seam_maps(R)[0], R)
    _, facts = dr.nms_seam_maps(R)
    assert m.shape[1:] == (2 * dr.NMS_TH, 2 * dr.NMS_TW) and 1 < dr.ntiles(*m.shape[1:]) <= dr.NMS_FIN_MAXT
    for i, (a, b) in enumerate(facts["near"]):
        assert (a[0] < dr.NMS_TH) != (b[0] < dr.NMS_TH) or (a[1] < dr.NMS_TW) != (b[1] < dr.NMS_TW), "the pair straddles a seam"
        assert np.argwhere(exp[i]).tolist() == [list(min(a, b))]
    for i, (a, b) in enumerate(facts["far"]):
        assert np.argwhere(exp[8 + i]).tolist() == sorted([list(a), list(b)])
    assert passes > 8
    _check_nms(m, R, exp, budgets=(1, 8))


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_nms_per_image_flags_vs_batch_level_stop(R):
    """images that need 1, 4 and more passes than enqueued: the reference counts maxima over the whole batch and keeps every image
    going, the kernels stop each image on its own flag.  Radius 4 finishes image 2 on the device; the other radii report it."""
    m, exp, passes = _nms_ref("passes", lambda: dr.nms_pass_count_batch(R), R)
    per_image = [dr.nms_ref(m[b:b + 1], R)[1] for b in range(3)]
    assert per_image[0] == 1 and per_image[1] == 4 and per_image[2] > 8 + 1 and passes == per_image[2]
    d = _nms_only(m, R, 8)
    flags = _np(d.not_converged).tolist()
    if R == 4:
        assert flags == [0, 0, 0]
        assert np.array_equal(_np(d.nms), exp)
    else:
        assert flags[:2] == [0, 0] and flags[2] != 0
        assert np.array_equal(_np(d.nms)[:2], exp[:2])  # the converged images are final already
    _check_nms(m, R, exp)


# ------------------------------------------------------------------ NMS: signs
SIGN_MAPS = dr.nms_sign_maps()


@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(SIGN_MAPS))
def test_nms_signs(name, R):
    """no sign test in the is-max rule: a negative pixel or an exact zero whose zero-padded window holds nothing larger is a
    maximum and zeroes its neighbours (test_detect_paths_cpu.py::SIGN_SPLITS lists the rows that fail with `centre > 0` back)"""
    m, exp, passes = _nms_ref(("sign", name), lambda: SIGN_MAPS[name], R)
    want = {"uniform(-1,0.05)": "mixed", "all_negative": "neg", "negative_with_zero_block": "nonpos", "mixed_with_zero_border": "mixed",
            "plus_inf_peaks": "nonneg"}[name]
    assert dr.sign_of(m) == want and m.shape == (2, 40, 56)
    if name == "plus_inf_peaks":
        assert np.isinf(m).sum() == 7 and np.isinf(exp).sum() >= 4
    _check_nms(m, R, exp)


@pytest.mark.parametrize("R", [2, 4])
def test_points_map_on_a_signed_map(R):
    """prob_map_to_points_map end to end on a mixed-sign map: border removal in place, NMS, quantile threshold"""
    raw = dr.synth.uniform(5301, (2, 40, 56), -0.5, 0.1)
    assert dr.sign_of(raw) == "mixed"
    bordered = dr.border_ref(raw, 4)
    after, _ = dr.nms_ref(bordered, R)
    exp, pos, _, thr = dr.select_torch(after, 30, 0.08)  # radius 2: the threshold wins, radius 4: the quantile
    assert all(len(p) >= 30 for p in pos) and ((thr < np.float32(0.08)).all() if R == 4 else (thr == np.float32(0.08)).all())
    score = _t(raw)[:, None]
    got = du.prob_map_to_points_map(score, prob_thresh=0.08, nms_dist=R, border_dist=4, top_k=30)
    assert np.array_equal(_np(got), exp)
    assert np.array_equal(_np(score)[:, 0], bordered)
    listed = du.prob_map_to_positions_with_prob(got)
    for b in range(2):
        assert np.array_equal(_np(listed[b]), pos[b])


# ------------------------------------------------------------------ NMS: untracked finisher
def test_nms_finisher_without_tile_tracking():
    """more tiles than the finisher tracks (2049 > NMS_FIN_MAXT): every pass revisits every tile.  Three windows of short ramps
    (first tile, across the seam of the last two tiles, up to the last column) need more passes than the two enqueued; the
    expected map is put together from the windows' crops (independent: test_detect_paths_cpu.py), all else stays zero."""
    H, W = dr.UNTRACKED_H, dr.UNTRACKED_W
    assert dr.ntiles(H, W) == dr.NMS_FIN_MAXT + 1 > dr.NMS_FIN_MAXT
    m = np.zeros((1, H, W), np.float32)
    exp = np.zeros((1, H, W), np.float32)
    for x0, win in dr.nms_untracked_windows():
        out, passes = dr.nms_ref(win[None], 4)
        assert passes > 2 and dr.sign_of(win) == "nonneg"
        m[0, :, x0:x0 + win.shape[1]] = win
        exp[0, :, x0:x0 + win.shape[1]] = out[0]
    d = _nms_only(m, 4, 2)
    assert _np(d.not_converged).tolist() == [0]
    got = _np(d.nms)
    assert np.count_nonzero(got) == np.count_nonzero(exp)
    assert np.array_equal(got, exp)


# ------------------------------------------------------------------ selection (radius 0: the kernel reads the map under test)
SELECT = dr.select_cases()


def _check_select(c, score):
    m = c["map"]
    B = m.shape[0]
    nms, pos, idx, thr = dr.select_torch(m, c["top_k"], c["det_thr"], c["pads"], c["ordering"])
    dr.check_select_facts(c, nms, pos, thr)
    cap = max(max(len(p) for p in pos), 1)
    d = N.detect(score, top_k=c["top_k"], radius=0, det_thr=c["det_thr"], pads=c["pads"], ordering=c["ordering"], cap=cap)
    cnt = _np(d.counts)
    assert cnt.tolist() == [len(p) for p in pos], c["route"]
    assert np.array_equal(_np(d.thr), thr), (_np(d.thr), thr)
    for b in range(B):
        assert np.array_equal(_np(d.positions[b, :cnt[b]]), pos[b])
        assert np.array_equal(_np(d.indices[b, :cnt[b]]), idx[b])
    assert np.array_equal(_np(d.nms), nms)


@pytest.mark.parametrize("name", list(SELECT))
def test_select_paths(name):
    c = SELECT[name]
    m = c["map"]
    score = _t(m)
    n = m.shape[1] * m.shape[2]
    assert score.data_ptr() % 16 == 0
    if "n_mod4" in c:
        assert (score.data_ptr() + 4 * n) % 16 != 0, "image 1 must start off a 16-byte boundary"
    _check_select(c, score)


def test_select_view_with_odd_storage_offset():
    """N % 4 == 0 but the map starts 4 bytes off a 16-byte boundary: scalar loads"""
    c = {k: v for k, v in SELECT["view_32x64"].items() if k not in ("loads", "paths")}  # those describe the aligned read
    u = c["map"]
    flat = torch.zeros(u.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = _t(u).reshape(-1)
    view = flat[1:].view(1, 32, 64)
    assert view.storage_offset() == 1 and view.is_contiguous() and view.data_ptr() % 16 == 4 and u.size % 4 == 0
    _check_select(c, view)


GUARD, PATTERN = 4096, 0xA5  # the guard zone of test_workspace_gpu.py


def test_detect_c_abi_with_fewer_rows_than_survivors():
    """einx.h: `counts` may exceed cap, only cap rows are written.  Outputs prefilled; the rows behind the last image's cap, and the
    guard bytes behind the workspace, must be untouched."""
    B, H, W, nz, cap, spare = 2, 24, 40, 40, 16, 8
    c = SELECT["cap_below_survivors"]
    m = c["map"]
    assert m.shape == (B, H, W) and c["top_k"] == 0 and c["det_thr"] == 0.0
    _, pos, idx, thr = dr.select_torch(m, 0, 0.0)
    assert [len(p) for p in pos] == [nz, nz] and cap < nz
    score = _t(m)
    p = N.DetectParams(B, H, W, H, W, 0, 0, 0, 0, 0.0, 0, cap, 1)
    L = N.lib()
    nbytes = int(L.einx_detect_ws_bytes(ctypes.byref(p)))
    ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    ws[nbytes:] = PATTERN
    positions = torch.full((B * cap + spare, 3), float("nan"), dtype=torch.float32, device=DEV)
    indices = torch.full((B * cap + spare,), -1, dtype=torch.int32, device=DEV)
    counts = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    out_thr = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    flags = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    N.check(L.einx_detect(N._ptr(score), ctypes.byref(p), N._ptr(ws), None, N._ptr(positions), N._ptr(indices), N._ptr(counts), N._ptr(out_thr),
                          N._ptr(flags), N._stream(score)), "einx_detect")
    torch.cuda.synchronize()
    assert _np(counts).tolist() == [nz, nz]
    assert _np(flags).tolist() == [0, 0] and np.array_equal(_np(out_thr), thr)
    for b in range(B):
        assert np.array_equal(_np(positions[b * cap:(b + 1) * cap]), pos[b][:cap])
        assert np.array_equal(_np(indices[b * cap:(b + 1) * cap]), idx[b][:cap])
    assert bool(torch.isnan(positions[B * cap:]).all()) and bool((indices[B * cap:] == -1).all())
    assert int((ws[nbytes:] != PATTERN).sum()) == 0


# ------------------------------------------------------------------ border
@pytest.mark.parametrize("H,W,border", [(10, 14, 0), (10, 14, 3), (10, 14, 5), (10, 14, 7), (11, 14, 5), (10, 14, 100), (1, 1, 0), (1, 1, 1)])
def test_remove_border_edges(H, W, border):
    """border 0 changes nothing; border >= min(H, W) / 2 clears the whole map (11 x 14 at 5 keeps one row); 1 x 1"""
    m = dr.synth.uniform(8100 + H, (2, 1, H, W), -1.0, 1.0)
    exp = dr.border_ref(m, border)
    if border == 0:
        assert np.array_equal(exp, m)
    elif 2 * border >= min(H, W):
        assert not exp.any()
    else:
        assert exp.any() and not np.array_equal(exp, m)
    t = _t(m)
    assert N.remove_border(t, border) is t
    assert np.array_equal(_np(t), exp)
