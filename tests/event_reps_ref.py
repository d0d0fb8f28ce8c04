"""Plain numpy restatement of the three contracts of csrc/event_reps.hip: time surface, event stack and
event distance map of ONE sample.  Nothing here is fast; it is what the kernels are compared with bit for bit.

Common rules: tn = (t - t[0]) / ((t[-1] - t[0]) + 1e-8) in float64; event k is in bin i iff tn >= t0 and tn <= t1 with
t0 = i * dt, t1 = t0 + dt, dt = 1.0 / nb (both sides inclusive); xi = int(x), yi = int(y) truncated toward zero, and an event
outside the image is dropped.  A sample without events gives zeros (distance map: 8192.0)."""
import numpy as np

HV, DIAG = 62587, 89738   # 0.955 and 1.3693 in 16.16 fixed point
INF = 0x7FFFFFFF >> 2      # "no set pixel": float32(INF) / 65536 == 8192.0


def bin_members(events, nb, H, W):
    """per bin the indices (ascending) of the in-range events the predicate puts there, with xi, yi, (int)p and tn"""
    t = np.asarray(events["t"], np.float64)
    n = len(t)
    xi = np.asarray(events["x"], np.float32).astype(np.int32)
    yi = np.asarray(events["y"], np.float32).astype(np.int32)
    pi = np.asarray(events["p"], np.float32).astype(np.int32)
    if n == 0:
        return [np.zeros(0, np.int64)] * nb, xi, yi, pi, t
    with np.errstate(all="ignore"):
        tn = (t - t[0]) / ((t[-1] - t[0]) + 1e-8)
    inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    dt = 1.0 / nb
    bins = []
    for i in range(nb):
        t0 = i * dt
        t1 = t0 + dt
        bins.append(np.nonzero(inside & (tn >= t0) & (tn <= t1))[0])
    return bins, xi, yi, pi, tn


def time_surface(events, input_size):
    bins, H, W = (int(v) for v in input_size)
    out = np.zeros((bins, H, W), np.float32)
    win = np.full((bins, H, W), -1, np.int64)  # index of the event whose stamp a cell holds
    members, xi, yi, pi, tn = bin_members(events, bins // 2, H, W)
    for i, idx in enumerate(members):
        for k in idx:
            c = 2 * i + int(pi[k])
            if -bins <= c < 0:
                c += bins  # numpy wraps a negative index once
            if not 0 <= c < bins:
                continue
            if k > win[c, yi[k], xi[k]]:  # the highest-indexed event wins
                win[c, yi[k], xi[k]] = k
                out[c, yi[k], xi[k]] = np.float32(tn[k])
    return out


def event_stack(events, input_size):
    bins, H, W = (int(v) for v in input_size)
    acc = np.zeros((bins, H, W), np.int64)
    members, xi, yi, pi, _ = bin_members(events, bins, H, W)
    for i, idx in enumerate(members):
        for k in idx:
            acc[i, yi[k], xi[k]] += 2 * int(pi[k]) - 1
    return acc.astype(np.float32)


def chamfer(mask):
    """[H,W] bool -> float32 3x3 chamfer distance to the set pixels: the closed form, brute force over the set pixels, int64"""
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    d = np.full((H, W), INF, np.int64)
    gy, gx = np.mgrid[0:H, 0:W]
    for y, x in zip(ys, xs):
        dx, dy = np.abs(gx - x), np.abs(gy - y)
        lo, hi = np.minimum(dx, dy), np.maximum(dx, dy)
        d = np.minimum(d, HV * (hi - lo) + DIAG * lo)
    return d.astype(np.float32) * np.float32(1.0 / 65536.0)


def chamfer_sweep(mask):
    """the same distances by the classic two raster sweeps with the integer weights (forward: up-left, up, up-right, left;
    backward: the mirror), one row at a time; test_event_reps_cpu.py ties it to `chamfer`.  For slices too large for the brute
    force."""
    H, W = mask.shape
    d = np.where(mask, 0, INF).astype(np.int64)
    ramp = HV * np.arange(W, dtype=np.int64)
    pad = lambda r: np.concatenate(([INF], r, [INF]))  # noqa: E731

    def row(own, prev, flip):
        p = pad(prev)
        c = np.minimum(own, np.minimum(np.minimum(p[:-2], p[2:]) + DIAG, prev + HV))
        if flip:
            c = c[::-1]
        c = ramp + np.minimum.accumulate(c - ramp)  # d[x] = min(c[x], d[x-1] + HV)
        return c[::-1] if flip else c

    prev = np.full(W, INF, np.int64)
    for y in range(H):
        prev = d[y] = row(d[y], prev, False)
    prev = np.full(W, INF, np.int64)
    for y in range(H - 1, -1, -1):
        prev = d[y] = row(d[y], prev, True)
    return np.minimum(d, INF).astype(np.float32) * np.float32(1.0 / 65536.0)


def occupancy(events, input_size):
    """[bins,H,W] bool: the pixels hit by any event of a bin"""
    bins, H, W = (int(v) for v in input_size)
    occ = np.zeros((bins, H, W), bool)
    members, xi, yi, _, _ = bin_members(events, bins, H, W)
    for i, idx in enumerate(members):
        occ[i, yi[idx], xi[idx]] = True
    return occ


def distance_map(events, input_size, form=chamfer):
    return np.stack([form(m) for m in occupancy(events, input_size)])


def fixture_events(z, name):
    """the event dict of case `name` of tests/golden/event_reps.npz (gen_event_reps.py).  The large case stores integers:
    pixel coordinates, polarity and microsecond increments; its stamps are 1.5e9 + cumsum(increments) * 1e-6."""
    if f"{name}.x" in z:
        return {k: np.asarray(z[f"{name}.{k}"]) for k in ("x", "y", "t", "p")}
    t = 1.5e9 + np.cumsum(np.asarray(z[f"{name}.dt_us"]).astype(np.float64)) * 1e-6
    return {"x": np.asarray(z[f"{name}.xi"]).astype(np.float32), "y": np.asarray(z[f"{name}.yi"]).astype(np.float32), "t": t,
            "p": np.asarray(z[f"{name}.pi"]).astype(np.float32)}
