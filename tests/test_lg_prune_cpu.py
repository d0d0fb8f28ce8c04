"""LightGlue point pruning, the parts that need no GPU: the float32 keep rule, the gate, the order (stop, then prune),
the empty-side rule and the scatter-back on the float64 restatement (tests/lg_prune_ref.py), the package's switches, refusals and
evaluator key, and the C ABI's argument checks and size queries."""
import ctypes
import types
from importlib import import_module

import numpy as np
import pytest
import torch

import lg_prune_ref as P
from helpers import lgf64_pair, lgf64_shipped_state_dict, load_pkg

pkg = load_pkg()
H = import_module(pkg.__name__ + ".harness")
LIB = import_module(pkg.__name__ + "._lib")
L = pkg.native.lib()
WIDTH = 0.99
MSHIFTS = {1: -5.78, 5: -5.52}  # the GPU test's configuration (tests/test_lg_prune_gpu.py)


def _state_dict(mshifts=MSHIFTS, tshifts=None):
    sd = lgf64_shipped_state_dict(7)
    for i, s in mshifts.items():
        sd[f"log_assignment.{i}.matchability.bias"] = sd[f"log_assignment.{i}.matchability.bias"] + np.float32(s)
    for i, s in (tshifts or {}).items():
        sd[f"token_confidence.{i}.token.0.bias"] = sd[f"token_confidence.{i}.token.0.bias"] + np.float32(s)
    return sd


def _pair(seed, n, m):
    d0, d1, k0, k1 = lgf64_pair(seed, n, m)
    return k0, d0, k1, d1


def test_float32_keep_rule_at_the_boundary():
    # thr_w = float32(1.0 - double(width_confidence)), not 1.0f - float32(width_confidence): 0.99 tells them apart
    thr = P.width_threshold(0.99)
    assert thr.dtype == np.float32 and thr == np.float32(1.0 - 0.99) and thr != np.float32(1.0) - np.float32(0.99)
    up, down = np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0))
    assert P.keep_mask(np.array([down, thr, up]), thr).tolist() == [False, False, True]  # strictly greater, in float32
    # a double a hair above the float32 threshold rounds onto it and is NOT kept; halfway to the next float32 it rounds up (to even)
    assert P.keep_mask(np.array([float(thr) + 1e-12]), thr).tolist() == [False]
    assert P.keep_mask(np.array([float(up) - 1e-12]), thr).tolist() == [True]
    # the token term (early stopping only): low-confidence points are never pruned, c <= thr_t in float32
    thr_t = np.float32(0.9)
    c = np.array([np.nextafter(thr_t, np.float32(1)), thr_t, np.nextafter(thr_t, np.float32(0))])
    assert P.keep_mask(np.array([down] * 3), thr, c, thr_t).tolist() == [False, True, True]
    assert P.keep_mask(np.array([up] * 3), thr, c, thr_t).tolist() == [True, True, True]
    # the package's helper states the same rule on tensors (what the reference's get_pruning_mask computes, :723-730)
    lg = pkg.LightGlue({"width_confidence": 0.99})
    s = torch.tensor([float(down), float(thr), float(up)])
    assert lg.get_pruning_mask(None, s, 0).tolist() == [False, False, True]
    ct = torch.tensor([float(c[0]), float(c[1]), float(c[2])])
    assert lg.get_pruning_mask(ct, torch.full((3,), float(down)), 0).tolist() == [False, True, True]  # thr[0] = float32(0.9)


def test_gate_and_prune_of_a_side_that_never_passes():
    """count > min_kpts (upstream's desc.shape[-2] > pruning_th): with min_kpts = 31 the 31 rows of side 0 are never touched and
    their prune stays 1 (the increment is inside the `if`); side 1 starts above the gate and is pruned until it is not"""
    sd = _state_dict()
    pair = _pair(11, 31, 33)
    r = P.run(sd, *pair, WIDTH, min_kpts=31)
    assert r["safe"] and r["live"][0] == 31 and (r["prune0"] == 1).all() and np.array_equal(r["kept0"], np.arange(31))
    assert [s["layer"] for s in r["steps"]] == [0, 1] and all(s["pruned"] == [False, True] for s in r["steps"])
    assert r["live"][1] == len(r["steps"][1]["kept"][1]) < 31  # after layer 1 it no longer passes: untouched from then on
    assert sorted(set(r["prune1"].tolist())) == [2.0, 3.0]  # dropped at the second step / kept by both; none reaches n_layers
    free = P.run(sd, *pair, WIDTH, min_kpts=0)
    assert free["live"] == (15, 16) and sorted(set(free["prune0"].tolist())) == [2.0, 6.0, 9.0]  # dropped after layer 1, after layer 5, never
    assert int((free["prune0"] == 9).sum()) == 15
    gated = P.run(sd, *pair, WIDTH, min_kpts=1024)
    assert gated["steps"] == [] and (gated["prune0"] == 1).all() and (gated["prune1"] == 1).all()
    plain = P.lg_f64.forward(sd, *pair)
    assert np.array_equal(gated["matches0"], plain["matches0"]) and np.array_equal(gated["log_assignment"], plain["log_assignment"])
    lg = pkg.LightGlue({})
    assert lg.pruning_keypoint_thresholds == {"cpu": -1, "mps": -1, "cuda": 1024, "flash": 1536}
    assert lg.pruning_min_kpts(torch.device("cpu")) == -1 and lg.pruning_min_kpts(torch.device("cuda", 0)) == 1024
    lg.pruning_keypoint_thresholds["cuda"] = 0  # a plain dict the user edits
    assert lg.pruning_min_kpts("cuda") == 0


def test_nothing_pruned_without_the_moved_biases_and_the_near_figure():
    """the synthetic model's matchability sigmoids stay above 0.01 on the test pair, so width_confidence 0.99 keeps every row and
    prune reaches n_layers; the float32 and float64 runs of the restatement differ by less than NEAR / 4 in those sigmoids"""
    sd0 = _state_dict({})
    pair = _pair(11, 31, 33)
    r = P.run(sd0, *pair, WIDTH)
    assert r["safe"] and r["live"] == (31, 33) and (r["prune0"] == 9).all() and (r["prune1"] == 9).all() and len(r["steps"]) == 8
    sd = _state_dict()
    a, b = P.run(sd, *pair, WIDTH), P.run(sd, *pair, WIDTH, dtype=torch.float32)
    worst = 0.0
    for x, y in zip(a["steps"], b["steps"]):
        assert all(np.array_equal(p, q) for p, q in zip(x["kept"], y["kept"]))
        worst = max([worst] + [float(np.abs(p - q.astype(np.float64)).max()) for p, q in zip(x["sig"], y["sig"])])
    print("float32 vs float64 matchability sigmoid:", worst)
    assert 4 * worst <= P.NEAR == 1e-5


def test_stop_comes_before_the_step():
    """early stopping and pruning together: the (64, 64) pair stops after layer 5 (r = 0.96 > 0.95) and is NOT pruned there, although
    that layer's moved matchability bias drops more than half of the rows of the pair that runs on; the ratio's denominator is
    the original n + m"""
    sd = _state_dict({1: -5.78, 5: -5.6}, {5: 5.0})
    r = P.run(sd, *_pair(11, 64, 64), WIDTH, 0, 0.95)
    assert r["safe"] and r["stop"] == 6 and r["head"] == 5 and [s["layer"] for s in r["steps"]] == [0, 1, 2, 3, 4]
    assert r["live"] == (63, 62) and r["r"][5] == float(P.ES.ratio(r["below"][5], 128))
    assert int((r["prune0"] == 6).sum()) == 63 and int((r["prune0"] == 2).sum()) == 1
    on = P.run(sd, *_pair(11, 31, 33), WIDTH, 0, 0.95)
    assert on["safe"] and on["stop"] == 9 and on["live"] == (17, 17)
    sizes = {s["layer"]: (len(s["kept"][0]), len(s["kept"][1])) for s in on["steps"]}
    assert sizes[4] == (30, 32) and sizes[5] == (17, 17)
    # the token term: without early stopping the same weights keep fewer rows after layer 1
    plain = P.run(sd, *_pair(11, 31, 33), WIDTH, 0, -1)
    assert plain["stop"] is None and len(plain["steps"][1]["kept"][0]) == 24 < 30


def test_a_side_pruned_to_zero_rows_finishes_the_pair():
    sd = _state_dict()
    k0, d0, k1, d1 = _pair(11, 1, 1)
    r = P.run(sd, k0, d0, k1, d1, WIDTH)
    assert r["safe"] and r["live"] == (0, 0) and r["head"] is None and r["log_assignment"] is None and r["stop"] is None
    assert r["matches0"].tolist() == [-1] and r["matches1"].tolist() == [-1] and r["scores0"].tolist() == [0.0]
    assert r["prune0"].tolist() == [6.0] and [s["layer"] for s in r["steps"]] == [0, 1, 2, 3, 4, 5]
    es = P.run(_state_dict({1: -5.78, 5: -5.6}, {5: 2.0}), k0, d0, k1, d1, WIDTH, 0, 0.95)
    assert es["safe"] and es["live"] == (1, 0) and es["stop"] == 6 and es["head"] is None and es["matches0"].tolist() == [-1]
    empty = P.run(sd, k0[:0], d0[:0], k1, d1, WIDTH, 0, 0.95)
    assert empty["stop"] == 0 and empty["live"] == (0, 1) and empty["steps"] == [] and empty["prune1"].tolist() == [1.0]


def test_scatter_back_by_hand():
    # survivors of side 0: original points 1, 4, 5; of side 1: 0, 2, 7.  Survivor 0 matches survivor 2, survivor 2 matches survivor 0
    ind0, ind1 = np.array([1, 4, 5]), np.array([0, 2, 7])
    m0, s0 = np.array([2, -1, 0]), np.array([0.5, 0.25, 0.75])
    out_m, out_s = P.scatter_back(m0, s0, ind0, ind1, 6)
    assert out_m.tolist() == [-1, 7, -1, -1, -1, 0] and out_s.tolist() == [0.0, 0.5, 0.0, 0.0, 0.25, 0.75]
    m1, s1 = np.array([2, -1, 0]), np.array([0.75, 0.0, 0.5])
    out_m, out_s = P.scatter_back(m1, s1, ind1, ind0, 8)
    assert out_m.tolist() == [5, -1, -1, -1, -1, -1, -1, 1] and out_s.tolist() == [0.75, 0, 0, 0, 0, 0, 0, 0.5]
    out_m, out_s = P.scatter_back(np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64), ind1, 3)
    assert out_m.tolist() == [-1, -1, -1] and out_s.tolist() == [0, 0, 0]


def test_package_switches_and_refusals():
    lg = pkg.LightGlue({"width_confidence": 0.95}).eval()
    assert lg.point_pruning is False and not lg.point_pruning_active()  # the reference ignores the key: opt-in
    lg.point_pruning = True
    assert lg.point_pruning_active() and not lg.early_stop_active()
    lg.conf["width_confidence"] = -1  # read at every call
    assert not lg.point_pruning_active()
    lg.conf["width_confidence"] = 0.95
    lg.train()
    assert not lg.point_pruning_active()
    lg.eval()
    # the 8h refusal still fires with the switch off, and no longer with it on
    lg.point_pruning, lg.early_stop, lg.conf["depth_confidence"] = False, True, 0.9
    with pytest.raises(NotImplementedError, match="8h"):
        lg.early_stop_active()
    assert not lg.point_pruning_active()
    lg.point_pruning = True
    assert lg.early_stop_active() and lg.point_pruning_active()


def test_loss_refuses_pruned_pred():
    lg = pkg.LightGlue({}).eval()
    pred = {"kept0": torch.zeros(1, 4, dtype=torch.int64), "ref_descriptors0": torch.zeros(1, 1, 4, 256), "ref_descriptors1": torch.zeros(1, 1, 4, 256)}
    with pytest.raises(ValueError, match="kept0"):
        lg.loss(pred, {"gt_matches0": torch.zeros(1, 4), "gt_matches1": torch.zeros(1, 4)})


def test_evaluator_reports_kept_ratio_only_when_live_is_present():
    ev = H.SameTimeEvaluator(None, 5)
    ev._metric_mean.add(torch.zeros(3, len(ev.names), dtype=torch.float64))
    bf = lambda c: types.SimpleNamespace(counts=torch.tensor(c, dtype=torch.int32))  # noqa: E731
    ev._account_kept(types.SimpleNamespace(live=None), bf([4, 4, 0]), bf([4, 6, 0]))
    assert "matcher_kept_ratio" not in ev.result()
    mr = types.SimpleNamespace(live=torch.tensor([2, 4, 0, 2, 1, 0], dtype=torch.int32), kept0=torch.zeros(3, 4), kept1=torch.zeros(3, 6))
    ev._account_kept(mr, bf([4, 4, 0]), bf([4, 6, 0]))  # (2 + 2) / 8, (4 + 1) / 10; the pair with n + m == 0 is left out
    assert ev.result()["matcher_kept_ratio"] == pytest.approx((0.5 + 0.5) / 2)
    rows = H.kept_ratio_rows(mr.live, bf([4, 9, 0]).counts, bf([4, 6, 0]).counts, 4, 6)  # counts are clamped to the capacities
    assert rows.shape == (3, 1) and rows[:2, 0].tolist() == [0.5, 0.5] and bool(torch.isnan(rows[2, 0]))


def test_different_time_evaluator_refuses_matcher_loss_with_pruning():
    lg = pkg.LightGlue({"width_confidence": 0.9}).eval()
    model = types.SimpleNamespace(matcher=types.SimpleNamespace(matcher=lg))
    ev = H.DifferentTimeEvaluator(model, 5, matcher_loss=True)
    batch = H._Batch([], None)
    ev._validate(batch)  # pruning off: nothing to refuse
    lg.point_pruning = True
    with pytest.raises(ValueError, match="point pruning"):
        ev._validate(batch)


def test_c_abi_argument_checks_and_size_queries():
    assert L.einx_abi_version() == 6  # additive symbols only
    assert "einx_lightglue_adaptive" in LIB.SIGNATURES and "einx_lightglue_adaptive_ws_bytes" in LIB.SIGNATURES
    q, es, base = L.einx_lightglue_adaptive_ws_bytes, L.einx_lightglue_early_stop_ws_bytes, L.einx_lg_ws_bytes_heads
    for bad in ((0, 64, 64, 256, 4, 256, 9), (2, 0, 64, 256, 4, 256, 9), (2, 64, 0, 256, 4, 256, 9), (2, 64, 64, 250, 4, 256, 9),
                (2, 64, 64, 256, 4, 256, 0), (2, 64, 64, 256, 4, 256, 33)):
        assert q(*bad) == 0, bad
    for shape in ((1, 5, 33, 256, 4, 256, 9), (5, 130, 130, 256, 4, 256, 9), (64, 2048, 2048, 256, 4, 256, 9), (3, 40, 48, 128, 2, 128, 3)):
        B, c0, c1 = shape[:3]
        extra = q(*shape) - es(*shape)
        assert q(*shape) % 256 == 0 and es(*shape) > base(*shape[:6]) > 0
        assert 4 * (B * c0 + B * c1 + 3 * B) <= extra <= 4 * (B * c0 + B * c1 + 3 * B) + 5 * 256, (shape, extra)  # dst0, dst1, prev, stop + rounding
    # the early-stop entry keeps its size: 8h's figure
    assert es(5, 130, 130, 256, 4, 256, 9) - base(5, 130, 130, 256, 4, 256) <= 1536
    # argument checks come before any launch: no device is needed
    w = LIB.LgWeights()
    w.n_layers = 2
    heads = (LIB.LgHead * 2)()
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    hs = ctypes.sizeof(LIB.LgHead)

    def rc(heads_=heads, head_size=hs, depth=-1.0, width=0.5, la=None, live=p, wp=ctypes.byref(w)):
        return L.einx_lightglue_adaptive(wp, heads_, head_size, depth, width, 0, *([None] * 3), 64, *([None] * 3), 64, 2, 1.0, 1.0, 1.0, 1.0, p,
                                         *([None] * 4), la, None, None, None, p, p, p, p, live, None)

    for kw, word in ((dict(live=None), b"null pointer"), (dict(wp=None), b"null pointer"), (dict(head_size=hs + 8), b"head_size"),
                     (dict(width=0.0), b"width_confidence"), (dict(width=-1.0), b"width_confidence"), (dict(width=1.5), b"width_confidence"),
                     (dict(la=p), b"log_assignment"), (dict(), b"log_assignment head")):
        assert rc(**kw) == -1 and word in L.einx_last_error(), (kw, L.einx_last_error())
    w.n_layers = 33
    assert rc() == -1 and b"1..32 layers" in L.einx_last_error()
    w.n_layers = 2
    for h in heads:
        h.proj_w = h.proj_b = h.match_w = h.match_b = p
    assert rc(depth=0.5) == -1 and b"token_confidence" in L.einx_last_error()
    assert rc() == -1 and b"null pointer" in L.einx_last_error()  # heads complete: the shared body's own checks (kpts0 is null)


# (B, cap0, cap1, d, heads, input_dim, n_layers) -> einx_lg_ws_bytes_heads, einx_lightglue_early_stop_ws_bytes,
# einx_lightglue_adaptive_ws_bytes, recorded from the library BEFORE the three carve functions became one (callers allocate by these
# figures, and the regions' offsets follow from the same walk): the shapes of the test above, unequal capacities both ways round,
# a single keypoint, 2 heads with an input projection, 1 and 32 layers, a head width that is no power of two, one 256-wide head.
WS_BYTES = {
    (1, 5, 33, 256, 4, 256, 9): (335872, 337408, 338688),
    (5, 130, 130, 256, 4, 256, 9): (11396608, 11398144, 11404544),
    (64, 2048, 2048, 256, 4, 256, 9): (2389706240, 2389708032, 2390757632),
    (3, 40, 48, 128, 2, 128, 3): (1229568, 1230848, 1232896),
    (2, 130, 70, 256, 4, 256, 9): (3506176, 3507712, 3510528),
    (2, 70, 130, 256, 4, 256, 9): (3506176, 3507712, 3510528),
    (1, 1, 1, 256, 4, 256, 9): (21760, 23296, 24576),
    (3, 130, 130, 128, 2, 64, 3): (3644672, 3645952, 3650304),
    (2, 64, 64, 256, 4, 256, 1): (2239744, 2241024, 2242816),
    (2, 64, 64, 256, 4, 256, 32): (2239744, 2241792, 2243584),
    (2, 64, 48, 256, 4, 256, 1): (1960192, 1961472, 1963264),
    (2, 64, 48, 256, 4, 256, 32): (1960192, 1962240, 1964032),
    (2, 64, 64, 96, 3, 96, 4): (863488, 864768, 866560),
    (1, 7, 7, 1024, 4, 1024, 2): (491776, 493056, 494336),
}
# every argument that makes all three queries return 0 ...
WS_ZERO = ((0, 64, 64, 256, 4, 256, 9), (-1, 64, 64, 256, 4, 256, 9), (2, 0, 64, 256, 4, 256, 9), (2, 64, 0, 256, 4, 256, 9),
           (2, 64, 64, 0, 4, 256, 9), (2, 64, 64, 256, 0, 256, 9), (2, 64, 64, 250, 4, 256, 9), (2, 64, 64, 256, 3, 256, 9),
           (2, 64, 64, 2048, 4, 256, 9), (2, 64, 64, 24, 4, 24, 9))
# ... and the layer counts that only the early-stop and adaptive queries refuse (the plain query takes no layer count)
WS_ZERO_LAYERS = ((2, 64, 64, 256, 4, 256, 0), (2, 64, 64, 256, 4, 256, -1), (2, 64, 64, 256, 4, 256, 33))


def test_workspace_sizes_are_the_recorded_ones():
    def q(shape):
        return (L.einx_lg_ws_bytes_heads(*shape[:6]), L.einx_lightglue_early_stop_ws_bytes(*shape), L.einx_lightglue_adaptive_ws_bytes(*shape))

    for shape, want in WS_BYTES.items():
        assert q(shape) == want, shape
    for shape in WS_ZERO:
        assert q(shape) == (0, 0, 0), shape
    for shape in WS_ZERO_LAYERS:
        assert q(shape) == (2239744, 0, 0), shape
    assert q((2, 64, 64, 256, 4, 8, 9)) == q((2, 64, 64, 256, 4, 256, 9))  # input_dim is part of the ABI and of no region
