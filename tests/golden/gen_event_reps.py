#!/usr/bin/env python3
"""Fixture of the time surface and the event stack, generated from the reference (build container only):
    python tests/golden/gen_event_reps.py   ->  tests/golden/event_reps.npz
Runs /root/reference/datasets/representations.py::events_to_time_surface and ::events_to_event_stack (cv2 stubbed: neither
touches it) on inputs that are in range and sorted, where the reference neither raises nor depends on where a binary search
lands: p in {0, 1} and in {-1, +1} (the latter wraps channel -1 of the time surface), even and odd bins, stamps drawn
continuously and on a coarse grid (many events share a stamp), all stamps equal, a single event, and stamps whose
normalised time lies EXACTLY on an interior bin boundary (found by searching the doubles next to boundary * denominator; such an
event belongs to two bins).  The small cases are stored in full; the 346x260 / 60k events / 16 bins case stores its inputs
as integers (tests/event_reps_ref.py::fixture_events rebuilds the float arrays) and its outputs as helpers.row_checksums plus
every 7th element.  The distance map has no fixture: cv2 is not available here, and DESIGN.md 8d defines that op by its written
algorithm.  The inputs are stored with the outputs; nothing of the reference's source is."""
import importlib.util, json, os, sys, types
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from event_reps_ref import fixture_events  # noqa: E402
from helpers import row_checksums  # noqa: E402

for name in ("cv2", "h5py", "hdf5plugin", "numba", "tqdm"):
    if name not in sys.modules:
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)  # imported at module level by the reference, unused by these functions
spec = importlib.util.spec_from_file_location("ref_representations", "/root/reference/datasets/representations.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)
rng = np.random.default_rng(20261017)
out = {}


def boundary_stamps(nb, span):
    """stamps in (0, span) whose tn = t / (span + 1e-8) equals i * dt or (i - 1) * dt + dt exactly, for every interior boundary"""
    den, dt, found = span + 1e-8, 1.0 / nb, []
    for i in range(1, nb):
        for target in {i * dt, (i - 1) * dt + dt}:
            c = target * den
            for _ in range(8):
                c = np.nextafter(c, -np.inf)
            for _ in range(17):
                if c / den == target:
                    found.append(c)
                c = np.nextafter(c, np.inf)
    return np.array(sorted(set(found)))


def coords(n, H, W):
    # quarter-pixel positions: fractional like rectified coordinates, and few enough distinct values to compress well
    return (rng.integers(0, 4 * W, n) / 4).astype(np.float32), (rng.integers(0, 4 * H, n) / 4).astype(np.float32)


def small_case(name, size, n, pol, stamps):
    bins, H, W = size
    x, y = coords(n, H, W)
    if stamps == "continuous":
        t = 1.5e9 + np.sort(rng.uniform(0, 0.05, n))
    elif stamps == "grid":  # 40 distinct stamps: long runs of equal times, some of them on or next to a boundary
        t = 1.5e9 + np.sort(rng.integers(0, 40, n)) * 1.25e-3
    elif stamps == "equal":
        t = np.full(n, 1.5e9)
    elif stamps == "boundary":
        nbs = sorted({bins, bins // 2})
        edge = np.concatenate([boundary_stamps(nb, 1.0) for nb in nbs])
        assert len(edge) >= sum(nb - 1 for nb in nbs), "no stamp found on some boundary"
        t = np.sort(np.concatenate([[0.0], np.repeat(edge, 6), rng.uniform(0, 1, n - 2 - 6 * len(edge)), [1.0]]))
    p = rng.choice(np.array(pol, np.float32), n)
    out[f"{name}.size"] = np.array(size)
    for k, v in (("x", x), ("y", y), ("t", t), ("p", p)):
        out[f"{name}.{k}"] = v


SMALL = []
for bins in (4, 5, 6):
    for (H, W) in ((13, 17), (20, 30)):
        for pol, pn in (((0, 1), "p01"), ((-1, 1), "pm1")):
            for stamps in ("continuous", "grid"):
                SMALL.append((f"b{bins}_{H}x{W}_{pn}_{stamps}", (bins, H, W), 3000, pol, stamps))
    SMALL.append((f"b{bins}_equal", (bins, 13, 17), 500, (-1, 1), "equal"))
    SMALL.append((f"b{bins}_one_event", (bins, 13, 17), 1, (0, 1), "equal"))
    SMALL.append((f"b{bins}_boundary", (bins, 20, 30), 3000, (-1, 1), "boundary"))
for c in SMALL:
    small_case(*c)

# the flagship geometry: integer pixel coordinates, microsecond increments, stored as integers
n = 60000
out["large.size"] = np.array([16, 260, 346])
out["large.xi"] = rng.integers(0, 346, n).astype(np.uint16)
out["large.yi"] = rng.integers(0, 260, n).astype(np.uint16)
out["large.pi"] = rng.integers(0, 2, n).astype(np.uint8)
out["large.dt_us"] = rng.integers(0, 4, n).astype(np.uint8)

names = [c[0] for c in SMALL] + ["large"]
meta = {"cases": [{"name": n, "size": [int(v) for v in out[f"{n}.size"]]} for n in names]}  # what helpers.Golden reads
out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
for name in names:
    ev = fixture_events(out, name)
    size = tuple(int(v) for v in out[f"{name}.size"])
    ts = ref.events_to_time_surface({k: v.copy() for k, v in ev.items()}, size).numpy()
    es = ref.events_to_event_stack({k: v.copy() for k, v in ev.items()}, size).numpy()
    for key, a in (("time_surface", ts), ("event_stack", es)):
        if name == "large":
            out[f"{name}.{key}.rowsum"], out[f"{name}.{key}.rowxor"] = row_checksums(a)
            out[f"{name}.{key}.stride7"] = a.reshape(-1)[::7]
        else:
            out[f"{name}.{key}"] = a
    print(name, float(np.abs(ts).sum()), float(np.abs(es).sum()))
np.savez_compressed(os.path.join(HERE, "event_reps.npz"), **out)
print(os.path.getsize(os.path.join(HERE, "event_reps.npz")), "bytes")
