"""CPU tests, component: detect.  The constructed inputs of tests/test_detect_paths_gpu.py against three statements of the rules that
share no code: tests/detect_ref.py in NumPy comparisons, the same loop in torch's unfold / argmax / fold and torch.quantile, and
oracle/einx_oracle.c.  The GPU rows compare the kernels with detect_ref alone; this file is what makes detect_ref trustworthy."""
import numpy as np
import pytest

import detect_ref as dr
from helpers import load_pkg

pkg = load_pkg()


def _three_way(oracle, m, R):
    a, pa = dr.nms_ref(m, R)
    b, pb = dr.nms_torch(m, R)
    c = np.array(m, np.float32)
    pc = oracle.fast_nms(c, R)
    assert np.array_equal(a, b) and np.array_equal(a, c), (int((a != b).sum()), int((a != c).sum()))
    assert pa == pb == pc, (pa, pb, pc)
    return a, pa


@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("H,W", [(h, w) for h, w, _, _ in dr.NMS_SIZES])
def test_nms_sizes_three_way(oracle, H, W, R):
    m = dr.nms_size_map(H, W)
    out, passes = _three_way(oracle, m, R)
    assert dr.sign_of(m) == "nonneg"
    if min(H, W) > 2 * R:
        assert passes >= 2 and 0 < np.count_nonzero(out) < np.count_nonzero(m)


@pytest.mark.parametrize("R", [2, 4])
def test_nms_seams_three_way(oracle, R):
    m, facts = dr.nms_seam_maps(R)
    out, passes = _three_way(oracle, m, R)
    for i, (a, b) in enumerate(facts["near"]):
        assert a[1] < dr.NMS_TW <= b[1] or b[1] < dr.NMS_TW <= a[1] or a[0] < dr.NMS_TH <= b[0] or b[0] < dr.NMS_TH <= a[0], "the pair must straddle a seam"
        assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) == R
        first = min(a, b)  # raster order = tuple order of (y, x)
        assert np.argwhere(out[i]).tolist() == [list(first)], "first raster wins"
    for i, (a, b) in enumerate(facts["far"]):
        assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) == R + 1
        assert np.argwhere(out[8 + i]).tolist() == sorted([list(a), list(b)]), "R + 1 apart: both survive"
    x0, x1 = facts["ramp_x"]
    assert x0 < dr.NMS_TW - 2 * R and x1 >= dr.NMS_TW + 2 * R, "the ramps reach past the value halo on both sides of the seam"
    for i in (16, 17, 18):
        assert dr.nms_ref(m[i:i + 1], R)[1] > 2, "suppression information has to cross the seam on successive passes"
    assert out[16, 10, x1] > 0 and out[17, 40, x0] > 0  # the top of each ramp survives
    assert out[18, dr.NMS_TH - 8, dr.NMS_TW - 8] == np.float32(0.75)  # first raster pixel of the plateau


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_nms_pass_count_batch_three_way(oracle, R):
    m = dr.nms_pass_count_batch(R)
    per_image = [dr.nms_ref(m[b:b + 1], R)[1] for b in range(3)]
    assert per_image[0] == 1 and per_image[1] == 4 and per_image[2] > 9, per_image
    out, passes = _three_way(oracle, m, R)
    assert passes == max(per_image)  # the batch-level count keeps every image going until the slowest one is done
    for b in range(3):  # ... which changes nothing on the others: per-image stopping gives the same maps
        assert np.array_equal(out[b], dr.nms_ref(m[b:b + 1], R)[0][0])


# which of the sign inputs distinguish the reference's rule from "only a positive pixel can be a maximum" at which radius
SIGN_SPLITS = {"uniform(-1,0.05)": (1, 2, 3, 4), "all_negative": (1, 2, 3, 4), "negative_with_zero_block": (1, 2, 3, 4),
               "mixed_with_zero_border": (1, 2), "plus_inf_peaks": ()}


@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(SIGN_SPLITS))
def test_nms_signs_three_way(oracle, name, R):
    m = dr.nms_sign_maps()[name]
    assert dr.sign_of(m) == {"uniform(-1,0.05)": "mixed", "all_negative": "neg", "negative_with_zero_block": "nonpos",
                             "mixed_with_zero_border": "mixed", "plus_inf_peaks": "nonneg"}[name]
    out, _ = _three_way(oracle, m, R)
    # the kernels stop each image when a pass changes nothing, the reference stops the batch when the count of maxima repeats: on
    # signed maps a maximum can lose its rank (its zeroed neighbours are above it), so the two are compared here and not assumed equal
    assert np.array_equal(dr.nms_per_image_fixpoint(m, R), out)
    old = dr.nms_per_image_fixpoint(m, R, positive_only=True)
    assert (not np.array_equal(old, out)) == (R in SIGN_SPLITS[name]), int((old != out).sum())


def test_nms_untracked_windows_are_independent_crops(oracle):
    """the 2049-tile map is never unfolded: its expected result is put together from the windows' crops.  Check on a narrow map
    that this is right: two windows 16 zero columns apart give the same result together as alone."""
    wins = dr.nms_untracked_windows()
    assert dr.ntiles(dr.UNTRACKED_H, dr.UNTRACKED_W) == dr.NMS_FIN_MAXT + 1
    seam = dr.NMS_TW * dr.NMS_FIN_MAXT
    (xa, a), (xb, b), (xc, c) = wins
    assert xa == 0 and xb < seam < xb + b.shape[1] and xc + c.shape[1] == dr.UNTRACKED_W and xc - (xb + b.shape[1]) >= 8
    for _, w in wins:
        assert dr.sign_of(w) == "nonneg"
        out, passes = _three_way(oracle, w[None], 4)
        assert passes > 2
    both = np.zeros((1, dr.NMS_TH, b.shape[1] + 16 + c.shape[1]), np.float32)
    both[0, :, :b.shape[1]] = b
    both[0, :, b.shape[1] + 16:] = c
    out, _ = _three_way(oracle, both, 4)
    assert np.array_equal(out[0, :, :b.shape[1]], dr.nms_ref(b[None], 4)[0][0])
    assert np.array_equal(out[0, :, b.shape[1] + 16:], dr.nms_ref(c[None], 4)[0][0])
    assert not out[0, :, b.shape[1]:b.shape[1] + 16].any()


SELECT = dr.select_cases()


@pytest.mark.parametrize("name", list(SELECT))
def test_select_torch_vs_oracle(oracle, name):
    c = SELECT[name]
    m = c["map"]
    B, Hp, Wp = m.shape
    w0, w1, h0, h1 = c["pads"]
    nms, pos, idx, thr = dr.select_torch(m, c["top_k"], c["det_thr"], c["pads"], c["ordering"])
    o_nms, o_pos, o_idx, o_thr, _ = oracle.detect_post(m[:, None].copy(), c["top_k"], 0, 0, c["det_thr"], c["pads"], c["ordering"])
    assert np.array_equal(thr, o_thr), (thr, o_thr)
    assert np.array_equal(nms, o_nms[:, h0:Hp - h1, w0:Wp - w1])
    for b in range(B):
        assert np.array_equal(pos[b], o_pos[b]) and np.array_equal(idx[b], o_idx[b])
    dr.check_select_facts(c, nms, pos, thr)


def test_select_sparse40_rank_positions():
    """where the two ranks fall for each top_k of the sparse map: the branch of the threshold code each case reaches"""
    N, nz = 24 * 40, 40
    zeros = N - nz
    seen = set()
    for k in (1, 39, 40, 41, N - 1):
        lo, hi = pkg.native.topk_ranks(N, k)
        seen.add("lo < zeros" if lo < zeros else ("lo on the first candidate" if lo == zeros else "lo among the candidates"))
        if lo < zeros <= hi:
            seen.add("hi on the first candidate")
    assert seen == {"lo < zeros", "lo on the first candidate", "lo among the candidates", "hi on the first candidate"}, seen


RANK_N = [264 * 352, 260 * 346, 480 * 640, 184 * 240, 720 * 1280, 1, 2, 3, 5, 17, 4097, 1000003]


def test_topk_ranks_are_the_ranks_torch_quantile_reads():
    rng = np.random.default_rng(20240)
    pairs = 0
    for N in RANK_N:
        ks = {1, 2, 3, 10, 37, 100, 500, 1024, N // 2, N - 2, N - 1} | {int(k) for k in rng.integers(1, max(N, 2), 16)}
        for k in sorted(k for k in ks if 0 < k < N):
            assert pkg.native.topk_ranks(N, k) == dr.quantile_ranks(N, k), (N, k)
            pairs += 1
    assert pairs > 180
