"""GPU tests (-m gpu), component: event representations other than the voxel grid.
TimeSurface / EventStack / EventDistanceMap (csrc/event_reps.hip) against the reference's fixtures
(tests/golden/event_reps.npz) and the numpy restatement (tests/event_reps_ref.py), bit for bit: everything is integer work or
one correctly rounded float64 division and cast, so there is no tolerance anywhere in this file."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import event_reps_ref as R
from event_reps_cases import DISTANCE_MAP_CASES, case_events, case_id, plan_name
from helpers import Golden, row_checksums, synth, synth_raw_events
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu

rep = import_module(pkg.__name__ + ".datasets.representations")
REPS = Golden("event_reps")
OPS = {"TimeSurface": (rep.events_to_time_surface, R.time_surface), "EventStack": (rep.events_to_event_stack, R.event_stack),
       "EventDistanceMap": (rep.events_to_distance_map, R.distance_map)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _expected(name, ev, size):
    if name == "EventDistanceMap" and size[1] * size[2] > 5000:  # the brute force is quadratic; test_event_reps_cpu.py ties the two forms
        return R.distance_map(ev, size, form=R.chamfer_sweep)
    return OPS[name][1](ev, size)


@pytest.mark.parametrize("case", list(REPS.cases))
def test_ops_equal_fixtures_and_restatement(case):
    ev = R.fixture_events(REPS, case)
    size = tuple(int(v) for v in REPS[f"{case}.size"])
    keep = {k: v.copy() for k, v in ev.items()}
    for name, (fn, _) in OPS.items():
        got = _np(fn(ev, size))
        assert got.shape == size and got.dtype == np.float32
        assert np.array_equal(_bits(got), _bits(_expected(name, ev, size))), (case, name)
        key = {"TimeSurface": "time_surface", "EventStack": "event_stack"}.get(name)
        if key and f"{case}.{key}" in REPS:
            assert np.array_equal(_bits(got), _bits(REPS[f"{case}.{key}"])), (case, name)  # the reference's own bits
        elif key:
            rs, rx = row_checksums(got)
            assert np.array_equal(got.reshape(-1)[::7], REPS[f"{case}.{key}.stride7"]), (case, name)
            assert np.array_equal(rs, REPS[f"{case}.{key}.rowsum"]) and np.array_equal(rx, REPS[f"{case}.{key}.rowxor"]), (case, name)
        assert np.array_equal(_bits(got), _bits(_np(fn(ev, size)))), "two runs differ"
    assert all(np.array_equal(ev[k], keep[k]) for k in ev)  # the caller's dict is left alone


def _collision_events(c):
    """the recipe of test_nextrows_gpu.py::test_voxel_grid_collisions_and_out_of_range_events"""
    n, H, W = c["n"], c["H"], c["W"]
    x = synth.uniform(c["seed"], (n,), -3.0, min(W + 2.0, c["box"]))
    y = synth.uniform(c["seed"] + 1, (n,), -3.0, min(H + 2.0, c["box"]))
    hot = synth.uniform01(c["seed"] + 2, (n,)) < np.float32(0.33)
    x = np.where(hot, np.float32(W // 3) + np.float32(0.25), x).astype(np.float32)
    y = np.where(hot, np.float32(H // 2) + np.float32(0.5), y).astype(np.float32)
    t = 1.5e9 + np.cumsum(synth.uniform01(c["seed"] + 3, (n,)).astype(np.float64) * 1e-4 + 1e-6)
    if c.get("unsorted"):  # unsorted timestamps between the first and the last event
        t[1:-1] = t[1:-1][np.argsort(synth.uniform01(77, (n - 2,)))]
    p = np.where(hot | (synth.uniform01(c["seed"] + 4, (n,)) < np.float32(0.5)), np.float32(1), np.float32(-1)).astype(np.float32)
    return {"x": x, "y": y, "t": t, "p": p}


COLLISIONS = [dict(seed=3, n=20000, H=260, W=346, bins=5, box=4), dict(seed=4, n=50000, H=260, W=346, bins=5, box=400),
              dict(seed=5, n=9000, H=97, W=131, bins=3, box=30, unsorted=True), dict(seed=15, n=9000, H=97, W=131, bins=6, box=300, unsorted=True),
              dict(seed=6, n=70000, H=480, W=640, bins=5, box=700), dict(seed=8, n=20000, H=300, W=640, bins=16, box=700)]


@pytest.mark.parametrize("c", COLLISIONS, ids=lambda c: f"{c['H']}x{c['W']}b{c['bins']}s{c['seed']}")
def test_collisions_out_of_range_and_unsorted_events(c):
    """thousands of events on a handful of pixels, a hot pixel taking a third of them, coordinates in [-3, W+2] x [-3, H+2]
    (dropped, where numpy would wrap or raise), unsorted stamps (the per-event predicate is the contract): bit-equal to the
    restatement."""
    ev = _collision_events(c)
    size = (c["bins"], c["H"], c["W"])
    assert (ev["x"] < 0).any() and (ev["y"] < 0).any()
    for name, (fn, _) in OPS.items():
        got = _np(fn(ev, size))
        assert np.array_equal(_bits(got), _bits(_expected(name, ev, size))), (c, name)
    assert np.abs(_np(rep.events_to_event_stack(ev, size))).max() > 100  # the hot pixel really collects thousands of events


def _small_batch():
    base = dict(seed=21, n=4000, H=40, W=48, bins=6, frac=True, pneg=True)
    a, b = synth_raw_events(base), synth_raw_events(dict(base, seed=22, n=1500))
    empty = {k: v[:0] for k, v in a.items()}
    return [a, empty, b], (6, 40, 48)


def test_batch_with_empty_sample_stage_path_and_capture():
    """a batched call with one empty sample == the per-sample calls; the EventStage / on_stage_stream path of
    events_representation_batch gives the same bits; so does a replayed torch.cuda.graph capture of each op"""
    evs, size = _small_batch()
    L, N = pkg.native.lib(), pkg.native
    for name in OPS:
        batch_fn = rep.REPRESENTATIONS[name]
        single = [_np(batch_fn([e], size, DEV))[0] for e in evs]
        for b, e in enumerate(evs):
            assert np.array_equal(_bits(single[b]), _bits(_expected(name, e, size))), (name, b)
        got = _np(batch_fn(evs, size, DEV))
        assert np.array_equal(_bits(got), _bits(np.stack(single))), name
        assert np.array_equal(_bits(got), _bits(_np(batch_fn(evs, size, DEV)))), "two runs differ"
        assert (single[1] == (8192.0 if name == "EventDistanceMap" else 0.0)).all()  # the sample without events
        stage = rep.EventStage(DEV)
        for on_stage in (False, True):
            g, m = rep.events_representation_batch(evs, size, device=DEV, stage=stage, on_stage_stream=on_stage, representation_type=name)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(_np(g)), _bits(got)), (name, on_stage)
            assert np.array_equal(_np(m), _np(rep.events_mask_batch(evs, (size[2], size[1]), DEV)))
        # capture: the raw call on a side stream, replayed twice into a poisoned output
        op = {"TimeSurface": "time_surface", "EventStack": "event_stack", "EventDistanceMap": "distance_map"}[name]
        x, y, t, p, offs = rep._pack(evs, DEV)
        out = torch.full((len(evs),) + size, float("nan"), device=DEV)
        ws = torch.empty(getattr(L, f"einx_{op}_ws_bytes")(len(evs), *size, int(offs[-1])), dtype=torch.uint8, device=DEV)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            rc = getattr(L, f"einx_{op}")(N._ptr(x), N._ptr(y), N._ptr(t), N._ptr(p), offs.ctypes.data_as(ctypes.c_void_p), len(evs), *size,
                                          N._ptr(out), N._ptr(ws), ws.numel(), N._stream(out))
        assert rc == 0
        for _ in range(2):
            out.fill_(float("nan"))
            ws.fill_(0xAB)
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(_bits(_np(out)), _bits(got)), name


@pytest.mark.parametrize("case", DISTANCE_MAP_CASES, ids=case_id)
def test_every_distance_map_arm(case):
    """tests/event_reps_cases.py: every instantiation of distance_map_kernel at the first, the last and the exact-fit widths of its
    arm, H = 1 / 2 / 7, sparse patterns (corners, far columns, an empty bin) whose distances cross all 64 lanes and climb from the
    last row: bit-equal to the closed form for both samples, from the instantiation the row names, twice the same bits"""
    H, W, name = case
    events_list, size, _ = case_events(H, W)
    got = _np(rep.events_to_distance_map_batch(events_list, size, DEV))
    assert got.shape == (2,) + size and got.dtype == np.float32
    for b, ev in enumerate(events_list):
        assert np.array_equal(_bits(got[b]), _bits(R.distance_map(ev, size, form=R.chamfer))), (case, b)
    assert plan_name(pkg.native.lib(), H, W) == name
    assert np.array_equal(_bits(got), _bits(_np(rep.events_to_distance_map_batch(events_list, size, DEV)))), "two runs differ"


BIG_B, BIG_SIZE = 193, (4, 5, 9)


def _big_batch():
    """B = 193 samples: four launches of 64 (the offsets travel as kernel arguments, 64 samples at a time).  Samples 63 and 191
    (the last of a launch) are empty; all of 64..127 are, so the second launch has no event at all; sample 150 has 700 events, so
    only the third launch has more than one block of events; sample 192 makes a last launch of one sample; every other sample
    has (37 b) % 23 events."""
    bins, H, W = BIG_SIZE
    n = [0 if b in (63, 191) or 64 <= b < 128 else 700 if b == 150 else (37 * b) % 23 for b in range(BIG_B)]
    assert n[192] > 0 and n[62] > 0 and n[128] > 0 and max(n[:128] + n[151:]) < 256
    return [synth_raw_events(dict(seed=1000 + 5 * b, n=k, H=H, W=W, bins=bins, frac=True, pneg=True)) for b, k in enumerate(n)]


def test_batches_beyond_one_chunk():
    """all three ops at B = 193: every sample equals its own restatement bit for bit (the distance map: the closed form), the
    empty samples are all 0.0 (distance map: 8192.0); a capture of the raw call, replayed into an output poisoned with NaN, gives the
    same bits, the launch without events included"""
    evs = _big_batch()
    L, N = pkg.native.lib(), pkg.native
    x, y, t, p, offs = rep._pack(evs, DEV)
    for name, (_, ref) in OPS.items():
        op = {"TimeSurface": "time_surface", "EventStack": "event_stack", "EventDistanceMap": "distance_map"}[name]
        expect = np.stack([ref(e, BIG_SIZE) for e in evs])
        fill = 8192.0 if name == "EventDistanceMap" else 0.0
        for b, e in enumerate(evs):
            if len(e["t"]) == 0:
                assert (expect[b] == fill).all()
        out = torch.full((BIG_B,) + BIG_SIZE, float("nan"), device=DEV)
        ws = torch.empty(getattr(L, f"einx_{op}_ws_bytes")(BIG_B, *BIG_SIZE, int(offs[-1])), dtype=torch.uint8, device=DEV)
        call = lambda: getattr(L, f"einx_{op}")(N._ptr(x), N._ptr(y), N._ptr(t), N._ptr(p), offs.ctypes.data_as(ctypes.c_void_p), BIG_B,  # noqa: E731
                                                *BIG_SIZE, N._ptr(out), N._ptr(ws), ws.numel(), N._stream(out))
        assert call() == 0
        torch.cuda.synchronize()
        got = _np(out)
        bad = [b for b in range(BIG_B) if not np.array_equal(_bits(got[b]), _bits(expect[b]))]
        assert not bad, (name, bad)
        assert np.array_equal(_bits(got), _bits(_np(rep.REPRESENTATIONS[name](evs, BIG_SIZE, DEV)))), name  # the package's own path
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = call()
        assert rc == 0
        out.fill_(float("nan"))
        ws.fill_(0xAB)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(_np(out)), _bits(expect)), name


def test_bad_arguments_are_refused():
    L, N = pkg.native.lib(), pkg.native
    evs, size = _small_batch()
    x, y, t, p, offs = rep._pack(evs, DEV)
    out = torch.zeros((len(evs),) + size, device=DEV)
    for op in ("time_surface", "event_stack", "distance_map"):
        need = getattr(L, f"einx_{op}_ws_bytes")(len(evs), *size, int(offs[-1]))
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        call = lambda o, nbytes: getattr(L, f"einx_{op}")(N._ptr(x), N._ptr(y), N._ptr(t), N._ptr(p), o.ctypes.data_as(ctypes.c_void_p),  # noqa: E731
                                                          len(evs), *size, N._ptr(out), N._ptr(ws), nbytes, N._stream(out))
        assert call(offs, need - 1) == -1      # EINX_ERR_ARG: short workspace
        bad = offs.copy()
        bad[0] = 1
        assert call(bad, need) == -1           # offsets_host[0] != 0
        assert call(offs, need) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        rep.events_to_time_surface(evs[0], (1, 40, 48))  # bins // 2 == 0 bins


def _model(bins):
    cfg = pkg.default_config("SP_MNN", event_channels=bins)
    for sec in (cfg.event_extractor.vgg, cfg.image_extractor.superpointv1):
        sec.detection_top_k = 128
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=31)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    return model


@pytest.mark.parametrize("evaluator", ["SameTimeEvaluator", "DifferentTimeEvaluator"])
def test_evaluators_take_representation_type(evaluator):
    """for every representation_type: last_inputs[0] is the op's output, the metric rows of `step` equal those of `run` and those
    of a plain EIM forward on that representation; the default is the voxel grid, the same bits as without the argument"""
    metrics = import_module(pkg.__name__ + ".core.metrics._native_metrics")
    H, W, B, bins = 100, 124, 2, 6
    model = _model(bins)
    evs = [synth_raw_events(dict(seed=300 + b, n=6000, H=H, W=W, bins=bins, frac=False, pneg=False)) for b in range(B)]
    img = synth.synth_image(77, B, H, W)
    cls = getattr(pkg, evaluator)
    seen = {}
    for name, batch_fn in rep.REPRESENTATIONS.items():
        ev_step = cls(model, bins=bins, resolution=(W, H), representation_type=name)
        rows, _ = ev_step.step(evs, _t(img))
        rows = _np(rows)
        expect = batch_fn(evs, (bins, H, W), device=DEV)
        assert np.array_equal(_bits(_np(ev_step.last_inputs[0])), _bits(_np(expect))), name
        ev_run = cls(model, bins=bins, resolution=(W, H), representation_type=name)
        (rows_run, _), = list(ev_run.run([(evs, _t(img))]))
        assert np.array_equal(_bits(_np(ev_run.last_inputs[0])), _bits(_np(expect))), name
        assert np.array_equal(rows, _np(rows_run), equal_nan=True), name
        ef, imf, _m = model(expect, _t(img), ev_step.last_inputs[1])
        fwd = metrics.batch_metrics(ef._batched, imf._batched, model._last_match, None, ev_step.mma_thr, ev_step.vdd_thr)
        assert np.array_equal(rows, _np(fwd), equal_nan=True), name
        seen[name] = _np(expect)
    default = cls(model, bins=bins, resolution=(W, H))
    assert default.representation_type == "VoxelGrid"
    default.step(evs, _t(img))
    assert np.array_equal(_bits(_np(default.last_inputs[0])), _bits(seen["VoxelGrid"]))
    assert np.array_equal(_bits(seen["VoxelGrid"]), _bits(_np(rep.events_to_voxel_grid_batch(evs, (bins, H, W), True, DEV))))
    assert len({a.tobytes() for a in seen.values()}) == 4  # four different inputs really reached the network
