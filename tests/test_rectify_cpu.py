"""Rectification (datasets/rectify.py, csrc/rectify.hip), the part that needs no GPU: the C ABI's new symbols and
its workspace query, every refusal of the Python layer (all raised before a device call), and the sanity of the float64
restatement the GPU tests compare with."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import rectify_ref as ref
from helpers import load_pkg

pkg = load_pkg()
L = pkg.native.lib()
rectify = import_module(pkg.__name__ + ".datasets.rectify")
datasets = import_module(pkg.__name__ + ".datasets")
EINX_ERR_ARG = -1

SYMBOLS = ("einx_rectify_map_fisheye", "einx_rectify_map_radtan", "einx_undistort_points_map_radtan", "einx_remap_bilinear",
           "einx_events_remap_ws_bytes", "einx_events_remap", "einx_events_remap_chunk")


def test_symbols_resolve_and_the_abi_version_stays():
    sig = import_module(pkg.__name__ + "._lib").SIGNATURES
    for name in SYMBOLS:
        assert name in sig and hasattr(L, name), name
    assert L.einx_abi_version() == 6
    for name in ("fisheye_rectify_map", "radtan_rectify_map", "radtan_undistort_points_map", "remap", "rectify_events"):
        assert getattr(datasets, name) is getattr(rectify, name)
    assert callable(pkg.EventSequence.rectified)


def test_events_remap_workspace_is_linear_in_the_workgroups():
    """positive, non-decreasing in N, and below 1 MiB + N / 64 bytes: no per-event flag (not even one bit each) fits in that"""
    q = L.einx_events_remap_ws_bytes
    chunk = L.einx_events_remap_chunk()
    assert chunk >= 512 and chunk % 64 == 0
    sizes = [0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 10**3, 100003, 10**6, 3000001, 10**8, 2**31 - 1, 2**31, 3 * 10**9]
    got = [int(q(n)) for n in sizes]
    assert all(g > 0 for g in got)
    assert got == sorted(got)
    for n in (10**3, 10**6, 3 * 10**9):
        assert int(q(n)) < (1 << 20) + n // 64, n
    assert int(q(-1)) == 0


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    """null pointers, non-positive sizes and a short workspace: EINX_ERR_ARG with a message, from host code that runs before a launch"""
    buf = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    k = (ctypes.c_double * 4)(1, 1, 0, 0)
    d = (ctypes.c_double * 5)()
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused first
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    assert L.einx_rectify_map_fisheye(None, P(d), P(buf), P(buf), 4, 4, one, one, None) == EINX_ERR_ARG
    assert b"null" in L.einx_last_error()
    assert L.einx_rectify_map_fisheye(P(k), P(d), P(buf), P(buf), 0, 4, one, one, None) == EINX_ERR_ARG
    assert L.einx_rectify_map_radtan(P(k), P(d), P(buf), P(buf), 4, -1, one, one, None) == EINX_ERR_ARG
    assert L.einx_rectify_map_radtan(P(k), P(d), P(buf), P(buf), 4, 4, None, one, None) == EINX_ERR_ARG
    zero = (ctypes.c_double * 9)()
    assert L.einx_rectify_map_radtan(P(k), P(d), P(buf), P(zero), 4, 4, one, one, None) == EINX_ERR_ARG
    assert b"singular" in L.einx_last_error()
    assert L.einx_undistort_points_map_radtan(P(k), P(d), None, 4, 4, 5, 1, one, one, None) == EINX_ERR_ARG
    assert L.einx_undistort_points_map_radtan(P(k), P(d), P(buf), 4, 4, -1, 1, one, one, None) == EINX_ERR_ARG
    assert L.einx_remap_bilinear(None, 0, 1, 4, 4, one, one, 4, 4, one, None) == EINX_ERR_ARG
    assert L.einx_remap_bilinear(one, 2, 1, 4, 4, one, one, 4, 4, one, None) == EINX_ERR_ARG
    assert L.einx_remap_bilinear(one, 0, 0, 4, 4, one, one, 4, 4, one, None) == EINX_ERR_ARG
    assert L.einx_remap_bilinear(one, 1, 1, 4, 4, one, one, 4, 0, one, None) == EINX_ERR_ARG
    ev = [one] * 4
    outs = [one] * 5
    need = int(L.einx_events_remap_ws_bytes(1000))
    assert L.einx_events_remap(*ev, -1, one, one, 4, 4, 3.0, 3.0, *outs, one, need, None) == EINX_ERR_ARG
    assert L.einx_events_remap(None, one, one, one, 1000, one, one, 4, 4, 3.0, 3.0, *outs, one, need, None) == EINX_ERR_ARG
    assert L.einx_events_remap(*ev, 1000, None, one, 4, 4, 3.0, 3.0, *outs, one, need, None) == EINX_ERR_ARG
    assert L.einx_events_remap(*ev, 1000, one, one, 0, 4, 3.0, 3.0, *outs, one, need, None) == EINX_ERR_ARG
    assert L.einx_events_remap(*ev, 1000, one, one, 4, 4, 3.0, 3.0, *outs, None, need, None) == EINX_ERR_ARG
    assert L.einx_events_remap(*ev, 1000, one, one, 4, 4, 3.0, 3.0, *outs, one, need - 1, None) == EINX_ERR_ARG
    assert b"workspace" in L.einx_last_error()


def _maps(h=5, w=9, device="cpu"):
    return torch.zeros((h, w), device=device), torch.zeros((h, w), device=device)


def test_map_builders_refuse_bad_calibrations():
    I3 = np.eye(3)
    with pytest.raises(ValueError, match="K must be"):
        rectify.fisheye_rectify_map(np.eye(4), ref.MVSEC_D, I3, I3, (8, 8))
    with pytest.raises(ValueError, match="K must be"):
        rectify.radtan_rectify_map((1.0, 1.0, 0.0), ref.EC_D, (8, 8))
    with pytest.raises(ValueError, match="D must hold 4"):
        rectify.fisheye_rectify_map(ref.MVSEC_K, ref.EC_D, I3, I3, (8, 8))
    with pytest.raises(ValueError, match="D must hold 5"):
        rectify.radtan_rectify_map(ref.EC_K, ref.MVSEC_D, (8, 8))
    with pytest.raises(ValueError, match="D must hold 5"):
        rectify.radtan_undistort_points_map(ref.EC_K, ref.MVSEC_D, (8, 8))
    with pytest.raises(ValueError, match="R must be 3x3"):
        rectify.fisheye_rectify_map(ref.MVSEC_K, ref.MVSEC_D, np.eye(4)[:3], I3, (8, 8))
    with pytest.raises(ValueError, match="P must be 3x3 or 3x4"):
        rectify.fisheye_rectify_map(ref.MVSEC_K, ref.MVSEC_D, I3, np.eye(4), (8, 8))
    with pytest.raises(ValueError, match="P must be 3x3 or 3x4"):
        rectify.radtan_undistort_points_map(ref.EC_K, ref.EC_D, (8, 8), P=np.zeros(9))
    for size in ((8,), (0, 8), (8, -1), 8):
        with pytest.raises(ValueError, match="size must be"):
            rectify.radtan_rectify_map(ref.EC_K, ref.EC_D, size)
    with pytest.raises(ValueError, match="iters"):
        rectify.radtan_undistort_points_map(ref.EC_K, ref.EC_D, (8, 8), iters=-1)


def test_remap_refuses_bad_frames_and_maps():
    mx, my = _maps()
    img = np.zeros((2, 7, 13), np.uint8)
    with pytest.raises(ValueError, match="one shape"):
        rectify.remap(img, mx, torch.zeros(5, 8))
    with pytest.raises(ValueError, match="one shape"):
        rectify.remap(img, mx[0], my[0])
    with pytest.raises(ValueError, match="float32"):
        rectify.remap(img, mx.double(), my.double())
    with pytest.raises(ValueError, match="must be tensors"):
        rectify.remap(img, mx.numpy(), my.numpy())
    with pytest.raises(ValueError, match="map_x lies on"):
        rectify.remap(img, mx, torch.zeros((5, 9), device="meta"))
    with pytest.raises(ValueError, match="uint8 or float32"):
        rectify.remap(img.astype(np.float64), mx, my)
    with pytest.raises(ValueError, match="uint8 or float32"):
        rectify.remap(torch.zeros((2, 7, 13), dtype=torch.float16), mx, my)
    with pytest.raises(ValueError, match=r"\[F, Hs, Ws\]"):
        rectify.remap(np.zeros((2, 2, 7, 13), np.uint8), mx, my)
    with pytest.raises(ValueError, match=r"\[F, Hs, Ws\]"):
        rectify.remap(torch.zeros(13), mx, my)
    with pytest.raises(ValueError, match="the frames lie on"):
        rectify.remap(torch.zeros((2, 7, 13), device="meta"), mx, my)
    with pytest.raises(ValueError, match="numpy array or a tensor"):
        rectify.remap([[0.0]], mx, my)
    with pytest.raises(ValueError, match="empty"):
        rectify.remap(np.zeros((2, 0, 13), np.uint8), mx, my)


def test_rectify_events_refuses_bad_arguments():
    mx, my = _maps()
    ev = {"x": np.zeros(3), "y": np.zeros(3), "t": np.arange(3.0), "p": np.zeros(3)}
    seq = pkg.EventSequence(ev, device="cpu")
    for rule in ("MVSEC", "dsec", 3, (1.0,), (1.0, 2.0, 3.0), None, ("a", "b")):
        with pytest.raises(ValueError, match="rule must be"):
            rectify.rectify_events(seq, mx, my, rule)
    with pytest.raises(ValueError, match="one shape"):
        rectify.rectify_events(seq, mx, my[:4], "ec")
    with pytest.raises(ValueError, match="one shape"):
        seq.rectified(mx[None], my[None], "ec")
    with pytest.raises(ValueError, match="float32"):
        seq.rectified(mx.to(torch.float16), my.to(torch.float16), "ec")
    with pytest.raises(ValueError, match="map_x lies on"):
        seq.rectified(torch.zeros((5, 9), device="meta"), my, "mvsec")
    with pytest.raises(ValueError, match="the event sequence lies on"):
        seq.rectified(torch.zeros((5, 9), device="meta"), torch.zeros((5, 9), device="meta"), "mvsec")
    with pytest.raises(ValueError, match="EventSequence or a dict"):
        rectify.rectify_events([ev], mx, my, "ec")
    with pytest.raises(ValueError, match="differ in length"):  # the existing upload path's own refusal
        rectify.rectify_events({**ev, "p": np.zeros(2)}, mx, my, "ec")
    assert rectify._bounds("mvsec", 260, 346) == (345.0, 259.0) and rectify._bounds("ec", 180, 240) == (240.0, 180.0)
    assert rectify._bounds((10.5, 3), 5, 9) == (10.5, 3.0)


def test_restatement_undistortion_inverts_the_distortion():
    """distorting the undistorted points returns the pixel within 1e-6 px after 20 iterations, on the inner half of the EC
    sensor (where the fixed-point iteration contracts fast)"""
    W, H = ref.EC_SIZE
    v, u = np.meshgrid(np.arange(H // 4, 3 * H // 4, dtype=np.float64), np.arange(W // 4, 3 * W // 4, dtype=np.float64), indexing="ij")
    xu, yu = ref.undistort_points(ref.EC_K, ref.EC_D, u, v, iters=20)
    ub, vb = ref.distort_points(ref.EC_K, ref.EC_D, xu, yu)
    err = max(np.abs(ub - u).max(), np.abs(vb - v).max())
    print(f"round trip on the inner half of the EC sensor: {err:.3e} px")
    assert err <= 1e-6


def test_restatement_identity_and_precondition_of_the_rounded_map():
    """the identity calibration of the radtan model gives identity maps exactly; no coordinate of the EC points map lies within
    1e-9 of a half-integer (so rint cannot flip on a last-place difference), and the EC bounds filter both keeps and drops"""
    for size in (ref.SMALL_SIZE, ref.EC_SIZE):
        W, H = size
        u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        for mx, my in (ref.radtan_map(ref.IDENTITY_K, (0,) * 5, size), ref.undistort_points_map(ref.IDENTITY_K, (0,) * 5, size, rint=False)):
            assert np.array_equal(mx, u) and np.array_equal(my, v)
    mx, my = ref.undistort_points_map(ref.EC_K, ref.EC_D, ref.EC_SIZE, rint=False)
    gap = min(np.abs(mx - np.floor(mx) - 0.5).min(), np.abs(my - np.floor(my) - 0.5).min())
    W, H = ref.EC_SIZE
    rx, ry = np.rint(mx), np.rint(my)
    share = ((rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)).mean()
    print(f"nearest half-integer: {gap:.3e}; in bounds: {share:.3f}")
    assert gap > 1e-9
    assert 0.5 < share < 0.95
