"""Pose tracks and the depth / image pairing (datasets/poses.py, datasets/recording.py, csrc/posetrack.hip), the part
that needs no GPU: the float64 restatement the GPU tests compare with (tests/poses_f64.py) against what the reference's own
PoseInterpolator recorded (tests/golden/poses.npz, made by tests/golden/gen_poses.py with scipy), the pairing against numpy's
outer-difference argmin, the C ABI's new symbols, and every refusal of the Python layer that is raised before a device call.

The bound on a pose.  Reference and restatement are two float64 evaluations of the same function (1.1e-15 apart at the pose's scale
when the fixture was made), so after a cast to float32 they can differ only where a value lies on a float32 rounding boundary: by
one float32 spacing of the entry, at most 2^-23 |entry|.  Rotation entries are below 1 and a pose's translation entries below its
largest, so the bound per pose is 2^-23 max(1, max |translation|)."""
import ctypes
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import poses_f64 as P
from helpers import GOLDEN, load_pkg

pkg = load_pkg()
L = pkg.native.lib()
poses = import_module(pkg.__name__ + ".datasets.poses")
recording = import_module(pkg.__name__ + ".datasets.recording")
datasets = import_module(pkg.__name__ + ".datasets")
EINX_ERR_ARG = -1
Z = np.load(os.path.join(GOLDEN, "poses.npz"))
META = json.loads(bytes(Z["meta"]).decode())
SYMBOLS = ("einx_pose_interp", "einx_pose_relative", "einx_nearest_stamp")


def f32_bound(T):
    """per pose [Q]: 2^-23 max(1, max |translation|)"""
    return 2.0 ** -23 * np.maximum(1.0, np.abs(np.asarray(T, np.float64)[:, :3, 3]).max(1))


@pytest.mark.parametrize("name", [n for n, _, _ in P.TRACK_CASES])
def test_restatement_agrees_with_the_recorded_reference_poses(name):
    stamps, t, R, quat_R, queries = P.track_case(name)
    ref = Z[f"{name}.poses"]
    assert ref.dtype == np.float64 and ref.shape == (len(queries), 4, 4)
    mine, bad = P.interpolate(stamps, t, P.knots(R, quat_R), queries, inverse=True)
    assert bad == 0
    d32 = np.abs(mine.astype(np.float32).astype(np.float64) - ref.astype(np.float32).astype(np.float64)).max((1, 2))
    bound = f32_bound(ref)
    unequal = float((mine.astype(np.float32) != ref.astype(np.float32)).mean())
    d64 = float((np.abs(mine - ref).max((1, 2)) / (bound * 2.0 ** 23)).max())
    print(f"{name}: {len(queries)} queries, float32 casts differ in {100 * unequal:.4f} % of the entries, worst {float((d32 / bound).max()):.3f} of "
          f"the bound; scaled float64 difference {d64:.3g}")
    assert (d32 <= bound).all()
    # the product of a pose and its un-inverted form is the identity: `inverse` is the closed-form inverse of the other
    fwd, _ = P.interpolate(stamps, t, P.knots(R, quat_R), queries, inverse=False)
    assert np.abs(mine @ fwd - np.eye(4)).max() < 1e-13 * max(1.0, float(np.abs(t).max())) ** 2


def test_restatement_edges():
    """a query on a knot gives that knot's pose (first, interior, last); outside and NaN queries give NaN rows and are counted"""
    stamps, t, R, quat_R, _ = P.track_case("exact")
    qk = P.knots(R, quat_R)
    T, bad = P.interpolate(stamps, t, qk, stamps[[0, 5, 23]], inverse=False)
    assert bad == 0
    assert np.abs(T[:, :3, 3] - t[[0, 5, 23]]).max() < 1e-14 * np.abs(t).max()
    assert np.abs(T[:, :3, :3] - P.matrix_from_quat(qk[[0, 5, 23]])).max() < 2e-15
    q = np.array([stamps[0] - 1e-3, stamps[3], np.nan, stamps[-1] + 1e-3])
    T, bad = P.interpolate(stamps, t, qk, q)
    assert bad == 3 and np.isnan(T[[0, 2, 3]]).all() and np.isfinite(T[1]).all()
    T01, T10, bad = P.relative(stamps, t, qk, q, q[::-1].copy())
    assert bad == 6 and np.isnan(T01).all() and np.isnan(T10).all()
    T01, T10, bad = P.relative(stamps, t, qk, stamps[[2, 9]], stamps[[9, 2]])
    assert bad == 0 and np.abs(T01 @ T10 - np.eye(4)).max() < 1e-13 and np.abs(T01[0] - T10[1]).max() == 0.0


@pytest.mark.parametrize("name", list(P.PAIRING_CASES))
def test_pairing_restatement_is_bit_equal_to_the_recorded_argmin(name):
    stamps, queries = P.PAIRING_CASES[name]
    rec = Z[f"pairing.{name}"]
    assert rec.dtype == np.int64 and name in META["pairing"]
    assert np.array_equal(P.nearest_index(stamps, queries), rec)
    assert np.array_equal(P.nearest_index_dense(stamps, queries), rec)  # numpy here gives what numpy gave there


def test_pairing_cases_plant_what_they_claim():
    assert Z["pairing.tie"].tolist() == [0, 0, 1, 3, 4]
    s, q = P.PAIRING_CASES["mixed"]
    # different stamps below the query that round to one distance: the answer is neither the last stamp below the query ...
    j = int(np.searchsorted(s, q[0])) - 1
    assert abs(s[j] - q[0]) == abs(s[j - 1] - q[0]) and s[j] != s[j - 1] and Z["pairing.mixed"][0] == j - 1
    # ... nor left to the side the unrounded distances would choose
    assert abs(s[3] - q[4]) == abs(s[0] - q[4]) and Z["pairing.mixed"][4] < 3
    assert Z["pairing.nan"][0] == 0 and Z["pairing.dup_run"][0] == 1


def test_pairing_restatement_against_numpy_on_seeded_stamps():
    rng = np.random.default_rng(11)
    for F in (1, 2, 3, 40, 1000):
        s = np.sort(np.round(rng.uniform(0.0, 60.0, F), 0 if F > 3 else 2))  # F = 40 and 1000 are full of duplicates
        q = np.concatenate([rng.uniform(-5.0, 65.0, 200), s, (s[1:] + s[:-1]) / 2, [np.nan]])
        assert np.array_equal(P.nearest_index(s, q), P.nearest_index_dense(s, q)), F


def test_symbols_resolve_and_the_abi_version_stays():
    sig = import_module(pkg.__name__ + "._lib").SIGNATURES
    for name in SYMBOLS:
        assert name in sig and hasattr(L, name), name
    assert L.einx_abi_version() == 6
    assert datasets.PoseTrack is poses.PoseTrack and datasets.nearest_index is poses.nearest_index
    assert callable(recording.Recording.pair_batches)
    for name in ("pose_interp", "pose_relative", "nearest_stamp"):
        assert callable(getattr(pkg.native, name))


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused first
    assert L.einx_pose_interp(None, one, one, 2, one, 1, 1, 0, one, one, None) == EINX_ERR_ARG
    assert b"null" in L.einx_last_error()
    assert L.einx_pose_interp(one, one, one, 1, one, 1, 1, 0, one, one, None) == EINX_ERR_ARG
    assert b"two knots" in L.einx_last_error()
    assert L.einx_pose_interp(one, one, one, 2, one, -1, 1, 0, one, one, None) == EINX_ERR_ARG
    assert L.einx_pose_interp(one, one, one, 2, one, 1, 1, 2, one, one, None) == EINX_ERR_ARG
    assert b"out_type" in L.einx_last_error()
    assert L.einx_pose_interp(one, one, one, 2, one, 1, 1, 0, None, one, None) == EINX_ERR_ARG
    assert L.einx_pose_interp(one, one, one, 2, one, 1, 1, 0, one, None, None) == EINX_ERR_ARG
    assert L.einx_pose_relative(one, one, None, 2, one, one, 1, one, one, one, None) == EINX_ERR_ARG
    assert L.einx_pose_relative(one, one, one, 0, one, one, 1, one, one, one, None) == EINX_ERR_ARG
    assert L.einx_pose_relative(one, one, one, 2, one, None, 1, one, one, one, None) == EINX_ERR_ARG
    assert L.einx_pose_relative(one, one, one, 2, one, one, -2, one, one, one, None) == EINX_ERR_ARG
    assert L.einx_nearest_stamp(one, 0, one, 1, one, None) == EINX_ERR_ARG
    assert b"F must be positive" in L.einx_last_error()
    assert L.einx_nearest_stamp(None, 3, one, 1, one, None) == EINX_ERR_ARG
    assert L.einx_nearest_stamp(one, 3, one, -1, one, None) == EINX_ERR_ARG
    assert L.einx_nearest_stamp(one, 3, None, 1, one, None) == EINX_ERR_ARG


def _knots(n=4):
    ts = 1.5e9 + 0.01 * np.arange(n)
    return ts, np.zeros((n, 3)), np.stack([np.eye(3)] * n)


def test_pose_track_constructor_refusals():
    ts, t, R = _knots()
    quat = np.tile([0.0, 0.0, 0.0, 1.0], (4, 1))
    cases = {
        "one knot": (ts[:1], t[:1], R[:1], False, "at least 2"),
        "no knot": (ts[:0], t[:0], R[:0], False, "at least 2"),
        "equal stamps": (ts[[0, 1, 1, 3]], t, R, False, "strictly increasing"),
        "decreasing stamps": (ts[::-1].copy(), t, R, False, "strictly increasing"),
        "NaN stamp": (np.where(np.arange(4) == 2, np.nan, ts), t, R, False, "NaN"),
        "NaN translation": (ts, np.where(np.arange(12).reshape(4, 3) == 5, np.nan, t), R, False, "NaN"),
        "NaN rotation": (ts, t, np.where(np.arange(36).reshape(4, 3, 3) == 7, np.nan, R), False, "NaN"),
        "zero quaternion": (ts, t, np.where(np.arange(4)[:, None] == 1, 0.0, quat), True, "zero-norm"),
        "t of another length": (ts, t[:3], R, False, r"t must be \[N,3\]"),
        "t of another width": (ts, np.zeros((4, 2)), R, False, r"t must be \[N,3\]"),
        "matrices where quaternions are announced": (ts, t, R, True, r"\[N,4\] quaternions"),
        "quaternions where matrices are announced": (ts, t, quat, False, r"\[N,3,3\] matrices"),
        "R of another length": (ts, t, R[:3], False, r"\[N,3,3\] matrices"),
        "stamps that are not 1-D": (ts[:, None], t, R, False, r"timestamps must be \[N\]"),
    }
    for tag, (a, b, c, q, msg) in cases.items():
        with pytest.raises(ValueError, match=msg):
            poses.PoseTrack(a, b, c, quat_R=q, device="cpu")
        assert tag
    poses.PoseTrack(ts, t, R, device="cpu")
    poses.PoseTrack(ts, t, 3.0 * quat, quat_R=True, device="cpu")


def test_pose_track_knots_are_the_restatements():
    """the host construction (nearest rotation, quaternion, normalisation) gives the restatement's knots, bit for bit, and unit
    quaternions"""
    for name, _, _ in P.TRACK_CASES:
        stamps, t, R, quat_R, _ = P.track_case(name)
        track = poses.PoseTrack(stamps, t, R, quat_R=quat_R, device="cpu")
        assert track.quats.dtype == torch.float64 and track.stamps.dtype == torch.float64 and track.trans.dtype == torch.float64
        assert np.array_equal(track.quats.numpy(), P.knots(R, quat_R)), name
        assert np.abs(np.sqrt((track.quats.numpy() ** 2).sum(1)) - 1.0).max() < 4e-16
        assert len(track) == len(stamps) and track.range == (stamps[0], stamps[-1])
    # a reflection's nearest ROTATION, not its nearest orthogonal matrix
    ts, t, R = _knots(2)
    R[1] = np.diag([1.0, 1.0, -1.0]) + 1e-3
    q = poses.PoseTrack(ts, t, R, device="cpu").quats.numpy()
    assert np.linalg.det(P.matrix_from_quat(q)[1]) > 0.999


def test_host_queries_outside_the_track_raise_interp1ds_error_before_any_launch():
    """the track lies on the CPU here, where a launch would raise RuntimeError: the ValueError comes first"""
    ts, t, R = _knots()
    track = poses.PoseTrack(ts, t, R, device="cpu")
    lo, hi = ts[0], ts[-1]
    below = rf"A value \({lo - 1.0}\) in x_new is below the interpolation range's minimum value \({lo}\)\."
    above = rf"A value \({hi + 0.5}\) in x_new is above the interpolation range's maximum value \({hi}\)\."
    for q in (lo - 1.0, [ts[1], lo - 1.0], np.array([lo - 1.0]), torch.tensor([ts[2], lo - 1.0], dtype=torch.float64)):
        with pytest.raises(ValueError, match=below):
            track.interpolate(q)
    with pytest.raises(ValueError, match=above):
        track.interpolate([ts[1], hi + 0.5])
    with pytest.raises(ValueError, match="nan"):
        track.interpolate([ts[1], float("nan")])
    with pytest.raises(ValueError, match=below):
        track.relative([ts[1]], [lo - 1.0])
    with pytest.raises(ValueError, match=above):
        track.relative([hi + 0.5], [ts[1]])
    with pytest.raises(RuntimeError, match="HIP device"):  # in range: the launch is reached, and there is no CPU path
        track.interpolate([ts[1]])
    assert track.out_of_range is None


def test_nearest_index_refusals():
    with pytest.raises(ValueError, match="no stamps"):
        poses.nearest_index([], [1.0], device="cpu")
    with pytest.raises(ValueError, match="sorted"):
        poses.nearest_index([0.0, 2.0, 1.0], [1.0], device="cpu")
    with pytest.raises(ValueError, match="NaN"):
        poses.nearest_index([0.0, float("nan")], [1.0], device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        poses.nearest_index([0.0, 1.0, 1.0], [1.0], device="cpu")


def test_recording_refusals_before_any_upload():
    ts, t, R = _knots(6)
    track = poses.PoseTrack(ts, t, R, device="cpu")
    ev = {"x": np.zeros(3, np.float32), "y": np.zeros(3, np.float32), "t": ts[:3].copy(), "p": np.ones(3, np.float32)}
    img, dep = np.zeros((5, 4, 6), np.uint8), np.zeros((3, 4, 6), np.float32)
    its, dts, K = ts[:5], ts[1:4], np.eye(3)
    make = lambda **kw: recording.Recording(**{**dict(events=ev, images=img, image_ts=its, depth=dep, depth_ts=dts, poses=track, K=K, device="cpu"), **kw})  # noqa: E731
    for kw, msg in ((dict(events=[1, 2]), "EventSequence or a dict"), (dict(poses=(ts, t, R)), "PoseTrack"),
                    (dict(images=img.astype(np.float32)), "images must be torch.uint8"), (dict(depth=dep.astype(np.float64)), "depth must be torch.float32"),
                    (dict(images=img[0]), r"images must be \[F,H,W\]"), (dict(depth=dep[:, :3]), "depth frames"),
                    (dict(image_ts=its[:4]), "4 image_ts for 5 frames"), (dict(depth_ts=dts[:2]), "2 depth_ts for 3 frames"),
                    (dict(depth_ts=np.array([ts[1], ts[2], ts[-1] + 1.0])), "outside the pose track"),
                    (dict(depth_ts=np.array([ts[1], np.nan, ts[2]])), "NaN"), (dict(K=np.eye(4)), "K must be 3x3"),
                    (dict(images=img[:0], image_ts=its[:0]), "no images")):
        with pytest.raises(ValueError, match=msg):
            make(**kw)
    with pytest.raises(ValueError, match="sorted"):  # the last check before the pairing's launch
        make(image_ts=its[::-1].copy())
