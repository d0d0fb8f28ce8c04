"""TimeSurface / EventStack / EventDistanceMap (csrc/event_reps.hip), the part that needs no GPU:
the numpy restatement (tests/event_reps_ref.py) against the reference's own outputs (tests/golden/event_reps.npz), the chamfer
distance against the true Euclidean distance under derived bounds, and the host side of the feature (size queries, the
`representation_type` table)."""
import json
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

import event_reps_ref as R
from event_reps_cases import DISTANCE_MAP_CASES, DISTANCE_MAP_NAMES, MAX_SET, case_events, case_id, plan_name
from helpers import Golden, load_pkg, row_checksums

pkg = load_pkg()
REPS = Golden("event_reps")
NAMES = list(REPS.cases)
OPS = ("time_surface", "event_stack", "distance_map")


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference_fixture(name):
    """the per-event predicate and "highest index wins" reproduce the reference's two searchsorted slices and numpy's
    assignment bit for bit on every fixture case, the p = -1 channel wrap and events exactly on a bin boundary included"""
    ev = R.fixture_events(REPS, name)
    size = tuple(int(v) for v in REPS[f"{name}.size"])
    for key, fn in (("time_surface", R.time_surface), ("event_stack", R.event_stack)):
        got = fn(ev, size)
        if f"{name}.{key}" in REPS:
            assert np.array_equal(got.view(np.uint32), REPS[f"{name}.{key}"].view(np.uint32)), (name, key)
        else:
            rs, rx = row_checksums(got)
            assert np.array_equal(got.reshape(-1)[::7], REPS[f"{name}.{key}.stride7"]), (name, key)
            assert np.array_equal(rs, REPS[f"{name}.{key}.rowsum"]) and np.array_equal(rx, REPS[f"{name}.{key}.rowxor"]), (name, key)


def test_fixture_has_boundary_events_and_channel_wrap():
    """what the fixture is meant to pin is really in it: events that sit in two bins, and the last channel of an odd `bins`
    written through the wrap only"""
    for bins in (4, 5, 6):
        ev = R.fixture_events(REPS, f"b{bins}_boundary")
        for nb in (bins, bins // 2):
            members = R.bin_members(ev, nb, 20, 30)[0]
            assert sum(len(np.intersect1d(members[i], members[i + 1])) for i in range(nb - 1)) >= 6 * (nb - 1), (bins, nb)
    assert np.abs(REPS["b5_20x30_pm1_continuous.time_surface"][4]).sum() > 0
    assert np.abs(REPS["b5_20x30_p01_continuous.time_surface"][4]).sum() == 0


def test_chamfer_sweep_equals_closed_form():
    """the two raster sweeps with the integer weights give exactly the closed form (the restatement uses the sweeps for slices
    too large for the brute force; the kernel sweeps as well)"""
    rng = np.random.default_rng(5)
    for _ in range(60):
        H, W = int(rng.integers(5, 39)), int(rng.integers(6, 23))
        mask = np.zeros((H, W), bool)
        k = int(rng.integers(1, 11))
        mask[rng.integers(0, H, k), rng.integers(0, W, k)] = True
        assert np.array_equal(R.chamfer(mask), R.chamfer_sweep(mask)), (H, W, k)
    assert np.array_equal(R.chamfer_sweep(np.zeros((7, 9), bool)), np.full((7, 9), 8192.0, np.float32))


def test_chamfer_distance_against_euclidean():
    """D / E of every non-set pixel lies in [HV / 65536, sqrt(HV^2 + (DIAG - HV)^2) / 65536] = [0.955, 1.040993]: along an axis the
    chamfer distance is 0.955 per pixel (the lower end; a diagonal step costs 1.3693 / sqrt 2 = 0.968 per unit), and over all
    directions (a, b), a >= b, the ratio (HV (a - b) + DIAG b) / sqrt(a^2 + b^2) peaks where (a, b) is parallel to
    (HV, DIAG - HV).  Bounds derived, not measured; 1e-6 relative slack for the float32 output."""
    from scipy.ndimage import distance_transform_edt
    lo, hi = R.HV / 65536.0, np.sqrt(R.HV ** 2 + (R.DIAG - R.HV) ** 2) / 65536.0
    assert abs(hi - 1.040993) < 1e-6
    rng = np.random.default_rng(11)
    for _ in range(25):
        H, W = int(rng.integers(5, 61)), int(rng.integers(6, 81))
        mask = np.zeros((H, W), bool)
        k = int(rng.integers(1, 11))
        mask[rng.integers(0, H, k), rng.integers(0, W, k)] = True
        d = R.chamfer(mask).astype(np.float64)
        e = distance_transform_edt(~mask)
        assert np.all(d[mask] == 0)
        ratio = d[~mask] / e[~mask]
        assert ratio.min() >= lo * (1 - 1e-6) and ratio.max() <= hi * (1 + 1e-6), (ratio.min(), ratio.max())
    # a bin without a pixel: the saturation value, also through the event path (a sample without events)
    assert np.array_equal(R.chamfer(np.zeros((4, 5), bool)), np.full((4, 5), 8192.0, np.float32))
    empty = {k: np.zeros(0, np.float64) for k in "xytp"}
    assert np.array_equal(R.distance_map(empty, (3, 4, 5)), np.full((3, 4, 5), 8192.0, np.float32))
    assert not R.time_surface(empty, (4, 4, 5)).any() and not R.event_stack(empty, (3, 4, 5)).any()


# ---- host side of the feature ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_ws_bytes_queries(op):
    """the three size queries exist, are bound, refuse bad shapes with 0 and size the flagship batch"""
    sig = import_module(pkg.__name__ + "._lib").SIGNATURES
    assert f"einx_{op}_ws_bytes" in sig and f"einx_{op}" in sig
    q = getattr(pkg.native.lib(), f"einx_{op}_ws_bytes")
    assert q(0, 16, 260, 346, 1000) == 0
    assert q(32, 0, 260, 346, 1000) == 0
    assert q(32, 16, 260, 346, -1) == 0
    assert q(32, 16, 0, 346, 1000) == 0 and q(32, 16, 260, 0, 1000) == 0
    n = q(32, 16, 260, 346, 32 * 60000)
    assert n > 0 and n % 256 == 0
    # one 32-bit word per cell (time surface, event stack) or one bit per pixel in rows of whole words (distance map)
    words = 32 * 16 * 260 * (346 if op != "distance_map" else 11)
    assert 4 * words <= n < 4 * words + 1024
    assert q(32, 16, 260, 346, 0) == n  # the events take no workspace


def test_distance_map_plan_covers_every_width():
    """einx_distance_map_plan (the selection einx_distance_map launches from, without the launch): every width the op takes, at
    the smallest and the largest height, plans to a name that has rows in tests/event_reps_cases.py; all six arms occur there; what
    the op refuses plans to NULL, and the size query gives 0 for the same shapes"""
    L = pkg.native.lib()
    assert "einx_distance_map_plan" in import_module(pkg.__name__ + "._lib").SIGNATURES
    assert DISTANCE_MAP_NAMES == [f"distance_map_kernel<{ppl}>" for ppl in (2, 4, 6, 8, 12, 16)]
    for H in (1, 4096):
        for W in range(1, 1025):
            name = plan_name(L, H, W)
            assert name in DISTANCE_MAP_NAMES, (H, W, name)
            assert L.einx_distance_map_ws_bytes(1, 1, H, W, 0) > 0, (H, W)
    for H, W in ((1, 1025), (4096, 1025), (4097, 1), (4097, 1024), (0, 5), (5, 0), (-1, 5), (5, -1), (0, 0)):
        assert plan_name(L, H, W) is None, (H, W)
        assert L.einx_distance_map_ws_bytes(1, 1, H, W, 0) == 0, (H, W)


@pytest.mark.parametrize("case", DISTANCE_MAP_CASES, ids=case_id)
def test_distance_map_case_plans_to_its_name(case):
    H, W, name = case
    assert plan_name(pkg.native.lib(), H, W) == name


def _forward_sweep_only(mask):
    """event_reps_ref.chamfer_sweep without its second half: the distances a kernel would give whose backward sweep did nothing"""
    H, W = mask.shape
    d = np.where(mask, 0, R.INF).astype(np.int64)
    ramp = R.HV * np.arange(W, dtype=np.int64)
    prev = np.full(W, R.INF, np.int64)
    for y in range(H):
        p = np.concatenate(([R.INF], prev, [R.INF]))
        c = np.minimum(d[y], np.minimum(np.minimum(p[:-2], p[2:]) + R.DIAG, prev + R.HV))
        prev = d[y] = ramp + np.minimum.accumulate(c - ramp)
    return np.minimum(d, R.INF).astype(np.float32) * np.float32(1.0 / 65536.0)


@pytest.mark.parametrize("case", DISTANCE_MAP_CASES, ids=case_id)
def test_distance_map_case_events_draw_their_patterns(case):
    """the events of a table row: their occupancy under the contract (first and last event dropped, yet defining the time
    normalisation) is exactly the intended pattern per bin; no slice has more than 16 set pixels, so the closed form is cheap; the
    closed form equals the two sweeps; and the forward sweep alone does not, so the row needs the backward sweep.  (The 1x1 map
    is the one exception to the last point: its only pixel has no neighbour, so the forward sweep alone is exact there.)"""
    H, W, _ = case
    events_list, size, masks = case_events(H, W)
    assert len(events_list) == 2 and size == (9, H, W)
    forward_differs = False
    for b, (ev, mask) in enumerate(zip(events_list, masks)):
        empty = 8 - b  # sample 1 holds the patterns rotated by one bin
        assert ev["x"][0] < 0 and ev["x"][-1] < 0 and ev["t"][0] == 1.5e9 and ev["t"][-1] == 1.5e9 + 0.05
        assert np.array_equal(R.occupancy(ev, size), mask)
        assert mask.reshape(9, -1).sum(1).max() <= MAX_SET
        assert [i for i in range(9) if not mask[i].any()] == [empty]
        for m in mask:
            closed = R.chamfer(m)
            assert np.array_equal(closed, R.chamfer_sweep(m))
            forward_differs |= not np.array_equal(closed, _forward_sweep_only(m))
        assert np.array_equal(R.chamfer(mask[empty]), np.full((H, W), 8192.0, np.float32))
    assert forward_differs == ((H, W) != (1, 1))


def test_representation_table():
    rep = import_module(pkg.__name__ + ".datasets.representations")
    assert set(rep.REPRESENTATIONS) == {"VoxelGrid", "TimeSurface", "EventStack", "EventDistanceMap"}
    for name, fn in rep.REPRESENTATIONS.items():
        assert rep.build_representation(name) is fn and callable(fn)
    assert rep.REPRESENTATIONS["VoxelGrid"] is rep.events_to_voxel_grid_batch
    with pytest.raises(ValueError, match=r"^Unsupported representation type 'Bogus'\.$"):
        rep.build_representation("Bogus")
    for fn in ("events_to_time_surface", "events_to_event_stack", "events_to_distance_map"):
        assert callable(getattr(rep, fn)) and callable(getattr(rep, fn + "_batch"))
    with pytest.raises(ValueError, match="Unsupported representation type"):
        pkg.SameTimeEvaluator(None, 5, representation_type="Bogus")


def test_no_kernel_uses_scratch():
    """every kernel of csrc/event_reps.hip, as compiled for gfx950: no scratch (private memory), no spill, no LDS"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tools", "kernel_resources.py"), os.path.join(root, pkg.__name__, "csrc", "event_reps.hip"), "--json"]
    kernels = json.loads(subprocess.run(cmd, capture_output=True, text=True, check=True).stdout)
    names = " ".join(k["name"] for k in kernels)
    for want in ("rep_events_kernel<0>", "rep_events_kernel<1>", "rep_events_kernel<2>", "time_surface_gather_kernel", "event_stack_convert_kernel",
                 *DISTANCE_MAP_NAMES):
        assert want in names, (want, names)
    for k in kernels:
        assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["LDS Size [bytes/block]"]) == 0, k
