"""GPU tests (-m gpu), component: pose tracks and the depth / image pairing (csrc/posetrack.hip, datasets/poses.py)
against the float64 restatement tests/poses_f64.py, which tests/test_poses_cpu.py holds to the reference's recorded poses.

Bounds, per pose, at its scale s = max(1, max |translation|):
  float32 output: 2^-23 s.  Kernel and restatement are float64 evaluations of the same expressions in the same order, so their
      float32 casts differ only where a value lies on a float32 rounding boundary, by one spacing (test_poses_cpu.py).
  float64 output: 64 x 2^-52 s.  About fifty operations of relative error 2^-52 each lie between the knots and an entry, and the
      device's sin / atan2 differ from the host's by a few units in the last place.
The worst difference seen is printed next to each."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import poses_f64 as P
from helpers import GOLDEN
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu

N = pkg.native
L = N.lib()
poses = import_module(pkg.__name__ + ".datasets.poses")
Z = np.load(os.path.join(GOLDEN, "poses.npz"))
GUARD = 64
F64_FACTOR = 64.0 * 2.0 ** -52
F32_FACTOR = 2.0 ** -23


def _scale(T):
    return np.maximum(1.0, np.abs(np.asarray(T, np.float64)[:, :3, 3]).max(1)) if len(T) else np.ones(0)


def _check(tag, got, want, dtype):
    """got (device result, as numpy) against the restatement `want` [Q,4,4] float64 under the bound of `dtype`"""
    assert got.shape == want.shape and got.dtype == (np.float32 if dtype == torch.float32 else np.float64), tag
    if dtype == torch.float32:
        want, factor = want.astype(np.float32), F32_FACTOR
    else:
        factor = F64_FACTOR
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    fin = ~np.isnan(want).any((1, 2))
    d = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)).max((1, 2)) if fin.any() else np.zeros(0)
    bound = factor * _scale(want[fin])
    worst = float((d / bound).max()) if d.size else 0.0
    print(f"{tag}: {int(fin.sum())} poses, worst difference {float(d.max()) if d.size else 0.0:.3g} = {worst:.3f} of the bound")
    assert (d <= bound).all(), tag
    return worst


class Case:
    """a track on the device with its host knots"""

    def __init__(self, stamps, t, R, quat_R=False):
        self.stamps, self.t, self.quats = stamps, t, P.knots(R, quat_R)
        self.track = poses.PoseTrack(stamps, t, R, quat_R=quat_R, device=DEV)
        assert np.array_equal(_np(self.track.quats), self.quats)  # the same knots on both sides, bit for bit

    def want(self, q, inverse=True):
        return P.interpolate(self.stamps, self.t, self.quats, q, inverse=inverse)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, _, _ in P.TRACK_CASES:
        stamps, t, R, quat_R, queries = P.track_case(name)
        out[name] = (Case(stamps, t, R, quat_R), queries)
    return out


def _interp_guarded(track, q, inverse, dtype):
    """einx_pose_interp through the C ABI into a buffer with GUARD sentinel elements behind the Q x 16 outputs: (poses, counter)"""
    Q = int(q.numel())
    buf = torch.full((Q * 16 + GUARD,), -7.0, dtype=dtype, device=DEV)
    bad = torch.full((2,), 99, dtype=torch.int32, device=DEV)
    N.check(L.einx_pose_interp(N._ptr(track.stamps), N._ptr(track.trans), N._ptr(track.quats), len(track), N._ptr(q), Q, int(inverse),
                               0 if dtype == torch.float32 else 1, N._ptr(buf), N._ptr(bad), N._stream(buf)), "einx_pose_interp")
    torch.cuda.synchronize()
    assert bool((buf[Q * 16:] == -7.0).all()), "guard elements behind the output were written"
    assert int(bad[1]) == 99, "the counter is one int32"
    return _np(buf[:Q * 16]).reshape(Q, 4, 4), int(bad[0])


def _mixed_queries(case, Q, seed):
    """Q queries, unsorted and with repeats: the first, an interior and the last knot, both lerp-branch stretches (identical
    neighbours 7-8, neighbours 1e-9 rad apart 15-16), then draws (with replacement) from a pool of uniform ones"""
    s = case.stamps
    rng = np.random.default_rng(seed)
    special = [s[0], s[5], s[-1], 0.25 * s[7] + 0.75 * s[8], 0.5 * (s[15] + s[16]), s[8], s[16]]
    pool = rng.uniform(s[0], s[-1], 40)
    q = np.concatenate([special, rng.choice(pool, max(Q - len(special), 0))])[:Q]
    return q[rng.permutation(len(q))]


@pytest.mark.parametrize("Q", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("inverse", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pose_interp_against_the_restatement(cases, dtype, inverse, Q):
    case, _ = cases["exact"]
    q = _mixed_queries(case, Q, seed=Q + 1000 * inverse)
    got, bad = _interp_guarded(case.track, _t(q), inverse, dtype)
    want, _ = case.want(q, inverse)
    assert bad == 0
    _check(f"interp {dtype} inverse={inverse} Q={Q}", got, want, dtype)
    if Q:
        assert np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (Q, 1)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", [n for n, _, _ in P.TRACK_CASES])
def test_pose_interp_on_the_fixture_tracks(cases, name, dtype):
    """every recorded query of every fixture track (matrix knots exact and perturbed, N = 2, quaternion knots) through
    PoseTrack.interpolate with a device tensor"""
    case, queries = cases[name]
    got = case.track.interpolate(_t(queries), dtype=dtype)
    _check(f"fixture {name} {dtype}", _np(got), case.want(queries)[0], dtype)
    assert int(case.track.out_of_range) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pose_interp_long_track(dtype):
    """N = 1025: eleven search steps instead of five (and one; N = 2 is among the fixture tracks)"""
    stamps, t, R = P.make_track(seed=9, N=1025)
    case = Case(stamps, t, R)
    rng = np.random.default_rng(10)
    q = np.concatenate([rng.uniform(stamps[0], stamps[-1], 250), stamps[[0, 1, 511, 512, 513, 1023, 1024]]])
    got, bad = _interp_guarded(case.track, _t(q), True, dtype)
    assert bad == 0 and len(q) == 257
    _check(f"N=1025 {dtype}", got, case.want(q)[0], dtype)


def test_queries_outside_the_track_give_nan_rows_and_are_counted(cases):
    case, queries = cases["exact"]
    q = queries[:40].copy()
    clean = _np(case.track.interpolate(_t(q)))
    q[3], q[17], q[29] = case.stamps[0] - 1e-3, case.stamps[-1] + 1e-3, np.nan
    got = _np(case.track.interpolate(_t(q)))
    counter = case.track.out_of_range
    assert counter.dtype == torch.int32 and counter.device.type == "cuda" and int(counter) == 3
    rows = np.isnan(got).all((1, 2))
    assert np.nonzero(rows)[0].tolist() == [3, 17, 29] and not np.isnan(got[~rows]).any()
    assert np.array_equal(got[~rows], clean[~rows])  # the rest, bit for bit
    got64, bad = _interp_guarded(case.track, _t(q), False, torch.float64)
    assert bad == 3 and np.isnan(got64[[3, 17, 29]]).all() and not np.isnan(np.delete(got64, [3, 17, 29], 0)).any()
    # the next call starts from zero again
    case.track.interpolate(_t(queries[:5]))
    assert int(case.track.out_of_range) == 0


def test_stamps_at_epoch_scale_give_the_poses_of_stamps_at_zero():
    """one track with stamps from 0 and the same track 1.5e9 s later, queries shifted likewise: stamps and queries are multiples of
    2^-10 s and 2^-16 s, so both sets are exact in float64 and every difference q - t_i is the same number.  A float32 stamp path
    cannot tell the shifted knots apart."""
    rng = np.random.default_rng(21)
    _, t, R = P.make_track(seed=20)
    stamps0 = np.cumsum(rng.integers(5, 21, 24)).astype(np.float64) * 2.0 ** -10
    k = rng.integers(int(stamps0[0] * 2 ** 16), int(stamps0[-1] * 2 ** 16) + 1, 130)
    q0 = np.concatenate([k.astype(np.float64) * 2.0 ** -16, stamps0])
    shift = 1.5e9
    assert np.array_equal((stamps0 + shift) - shift, stamps0) and np.array_equal((q0 + shift) - shift, q0)
    assert len(np.unique((stamps0 + shift).astype(np.float32))) == 1  # what float32 makes of the shifted stamps
    a, b = Case(stamps0, t, R), Case(stamps0 + shift, t, R)
    for dtype in (torch.float32, torch.float64):
        ga, gb = _np(a.track.interpolate(_t(q0), dtype=dtype)), _np(b.track.interpolate(_t(q0 + shift), dtype=dtype))
        _check(f"shifted against its restatement {dtype}", gb, b.want(q0 + shift)[0], dtype)
        d = np.abs(ga.astype(np.float64) - gb.astype(np.float64)).max((1, 2))
        bound = (F32_FACTOR if dtype == torch.float32 else F64_FACTOR) * _scale(ga)
        print(f"stamps at 0 against stamps at 1.5e9, {dtype}: worst difference {float(d.max()):.3g}")
        assert (d <= bound).all()
    assert int(b.track.out_of_range) == 0


def test_host_queries_and_single_numbers(cases):
    case, queries = cases["quat"]
    q = queries[:9]
    dev = _np(case.track.interpolate(_t(q), dtype=torch.float64))
    assert np.array_equal(_np(case.track.interpolate(q, dtype=torch.float64)), dev)
    assert np.array_equal(_np(case.track.interpolate(list(q), dtype=torch.float64)), dev)
    one = case.track.interpolate(float(q[4]), dtype=torch.float64)
    assert one.shape == (4, 4) and np.array_equal(_np(one), dev[4])
    with pytest.raises(ValueError, match="above the interpolation range"):
        case.track.interpolate(case.stamps[-1] + 1.0)
    with pytest.raises(TypeError):
        case.track.interpolate(q, dtype=torch.float16)


@pytest.mark.parametrize("npairs", [1, 33])
def test_pose_relative(cases, npairs):
    case, queries = cases["p1e-4"]
    rng = np.random.default_rng(npairs)
    q0, q1 = rng.choice(queries, npairs), rng.choice(queries, npairs)
    T01, T10 = case.track.relative(_t(q0), _t(q1))
    assert int(case.track.out_of_range) == 0 and T01.dtype == torch.float32 and T01.shape == (npairs, 4, 4)
    w01, w10, _ = P.relative(case.stamps, case.t, case.quats, q0, q1)
    _check(f"T_0to1 P={npairs}", _np(T01), w01, torch.float32)
    _check(f"T_1to0 P={npairs}", _np(T10), w10, torch.float32)
    # each is the other's inverse: seven float32 roundings of size 2^-24 s meet in an entry of the product
    prod = _np(T01).astype(np.float64) @ _np(T10).astype(np.float64)
    s = np.maximum(_scale(_np(T01)), _scale(_np(T10)))
    d = np.abs(prod - np.eye(4)).max((1, 2))
    print(f"T_0to1 T_1to0 - I: worst {float((d / (8 * F32_FACTOR * s)).max()):.3f} of the bound")
    assert (d <= 8 * F32_FACTOR * s).all()
    # a pose relative to itself
    I01, I10 = case.track.relative(_t(q0), _t(q0))
    for got in (I01, I10):
        assert (np.abs(_np(got).astype(np.float64) - np.eye(4)).max((1, 2)) <= F32_FACTOR).all()
    # host queries take the same path after the range check
    H01, _ = case.track.relative(q0, q1)
    assert torch.equal(H01, T01)


def test_pose_relative_outside_the_track(cases):
    case, queries = cases["exact"]
    q0, q1 = queries[:6].copy(), queries[6:12].copy()
    clean01, clean10 = case.track.relative(_t(q0), _t(q1))
    q0[1], q1[1], q1[4] = np.nan, case.stamps[0] - 1.0, case.stamps[-1] + 1.0
    T01, T10 = case.track.relative(_t(q0), _t(q1))
    assert int(case.track.out_of_range) == 3  # queries, not pairs
    for got, clean in ((T01, clean01), (T10, clean10)):
        rows = torch.isnan(got).all(2).all(1)
        assert rows.tolist() == [False, True, False, False, True, False] and torch.equal(got[~rows], clean[~rows])


@pytest.mark.parametrize("name", list(P.PAIRING_CASES))
def test_nearest_stamp_fixture_cases(name):
    stamps, queries = P.PAIRING_CASES[name]
    got = poses.nearest_index(stamps, queries, device=DEV)
    assert got.dtype == torch.int64 and np.array_equal(_np(got), Z[f"pairing.{name}"])
    assert torch.equal(poses.nearest_index(_t(np.asarray(stamps)), _t(np.asarray(queries))), got)  # device tensors as they are


@pytest.mark.parametrize("F", [1, 2, 1000])
def test_nearest_stamp_against_numpy(F):
    rng = np.random.default_rng(F)
    s = 1.5e9 + np.sort(np.round(rng.uniform(0.0, 30.0, F), 1 if F > 2 else 3))  # F = 1000 over 301 values: runs of equal stamps
    q = np.concatenate([1.5e9 + rng.uniform(-2.0, 32.0, 150), rng.choice(s, 60), 1.5e9 + np.round(rng.uniform(0.0, 30.0, 46), 1) + 0.05, [np.nan]])
    assert len(q) == 257 and (F < 1000 or len(np.unique(s)) < F)
    got = _np(poses.nearest_index(s, q, device=DEV))
    assert np.array_equal(got, P.nearest_index_dense(s, q))
    assert poses.nearest_index(s, [], device=DEV).shape == (0,)
