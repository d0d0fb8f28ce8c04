"""The distance map's coverage table: every instantiation einx_distance_map can select (distance_map_kernel<PPL>, PPL pixels per
lane, chosen from ceil(W / 64)), at the edges of each arm, with the name einx_distance_map_plan reports.  Not collected by pytest
(no test_ prefix); used by test_event_reps_cpu.py (every row plans to its name, no name the dispatcher produces is missing here, the
events really draw the intended patterns) and by test_event_reps_gpu.py::test_every_distance_map_arm (bit-equal to the closed form).

RULE: a new arm in csrc/event_reps.hip needs its widths here.  The CPU sweep over W = 1..1024 fails on a name without a row.

Widths: per arm the last width of the arm before (W = 64 PPL_prev, an exact fit: lane 63 holds real pixels, the backward sweep has
no padding), the first of the arm (64 PPL_prev + 1: the most padding) and the one before the exact fit; W <= 32 is one 32-bit word
per row (the kernel's second word index clamps onto the first), W = 33 the first two-word row; W = 1 has no horizontal neighbour.
Heights: H = 1 (no previous row in either sweep), 2, and 7 (the backward sweep's carry up from the last row over several rows).

Patterns, one per bin, each of at most 16 set pixels so that the closed form (event_reps_ref.chamfer, brute force over the set
pixels) is the reference, and sparse, so that distances travel across all 64 lanes and up from the last row:
  0-3  one pixel in each corner: (0, 0), (0, W-1), (H-1, 0), (H-1, W-1)
  4    (H//2, 0) and (H//2, W-1) together
  5    column W-1 in every row
  6    every ceil(W / 16)-th pixel of row 0
  7    at most 16 seeded random pixels
  8    no event: 8192.0 everywhere
Sample 0 holds pattern i in bin i, sample 1 pattern (i + 1) % 9: a slice index error shows."""
import functools

import numpy as np

WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024)
HEIGHTS = (1, 2, 7)
BINS = 9
MAX_SET = 16  # set pixels per slice: what keeps the brute-force closed form cheap


def _arm(W):
    for ppl in (2, 4, 6, 8, 12, 16):
        if W <= 64 * ppl:
            return f"distance_map_kernel<{ppl}>"
    raise ValueError(W)


# (H, W, expected kernel name)
DISTANCE_MAP_CASES = [(H, W, _arm(W)) for W in WIDTHS for H in HEIGHTS]
DISTANCE_MAP_NAMES = sorted({c[2] for c in DISTANCE_MAP_CASES}, key=lambda s: int(s[s.index("<") + 1:-1]))


def case_id(c):
    return f"{c[0]}x{c[1]}"


def plan_name(lib, H, W):
    """einx_distance_map_plan as a str (None for a shape einx_distance_map refuses)"""
    r = lib.einx_distance_map_plan(int(H), int(W))
    return None if r is None else r.decode()


def patterns(H, W):
    """[BINS,H,W] bool: the nine patterns of the module docstring"""
    m = np.zeros((BINS, H, W), bool)
    m[0, 0, 0] = m[1, 0, W - 1] = m[2, H - 1, 0] = m[3, H - 1, W - 1] = True
    m[4, H // 2, 0] = m[4, H // 2, W - 1] = True
    m[5, :, W - 1] = True
    m[6, 0, ::-(-W // 16)] = True
    rng = np.random.default_rng([H, W])
    m[7, rng.integers(0, H, MAX_SET), rng.integers(0, W, MAX_SET)] = True
    return m


@functools.lru_cache(maxsize=None)
def case_events(H, W):
    """(events_list, input_size, masks): B = 2 event dicts whose occupancy is masks [2,BINS,H,W].  Each pattern's events lie at
    the centre of their bin, at x + 0.25, y + 0.5; the first and the last event of a sample lie outside the image (dropped) and
    carry the two stamps the time normalisation is taken from.  Shared between tests: do not modify."""
    pat = patterns(H, W)
    masks = np.stack([pat, np.roll(pat, -1, axis=0)])
    events_list = []
    for mask in masks:
        x, y, t = [-5.0], [0.5], [1.5e9]
        for i in range(BINS):
            ys, xs = np.nonzero(mask[i])
            x += list(xs + 0.25)
            y += list(ys + 0.5)
            t += [1.5e9 + (i + 0.5) / BINS * 0.05] * len(xs)
        x.append(-5.0)
        y.append(0.5)
        t.append(1.5e9 + 0.05)
        ev = {"x": np.asarray(x, np.float32), "y": np.asarray(y, np.float32), "t": np.asarray(t, np.float64), "p": np.ones(len(x), np.float32)}
        for v in ev.values():
            v.setflags(write=False)
        events_list.append(ev)
    masks.setflags(write=False)
    return events_list, (BINS, H, W), masks
