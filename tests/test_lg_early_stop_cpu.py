"""LightGlue early stopping, the parts that need no GPU: the thresholds, the float32 decision, the float64
restatement (tests/lg_early_stop_ref.py) on the shipped model, and the package's switches, refusals and evaluator key."""
import types
from importlib import import_module

import numpy as np
import pytest
import torch

import lg_early_stop_ref as R
from helpers import lgf64_pair, lgf64_shipped_state_dict, load_pkg

pkg = load_pkg()
H = import_module(pkg.__name__ + ".harness")
COUNTS = [(31, 33), (64, 64), (129, 300), (130, 130)]


def test_thresholds():
    thr = R.thresholds(9)
    assert len(thr) == 8 and all(t.dtype == np.float32 for t in thr)
    assert thr[0] == np.float32(0.9)
    assert all(a > b for a, b in zip(thr, thr[1:])) and all(0.8 < t <= 0.9 for t in thr)
    lg = pkg.LightGlue({})
    assert len(lg.confidence_thresholds) == 9 and lg.confidence_thresholds[0] == pytest.approx(0.9, abs=1e-15)
    assert [np.float32(t) for t in lg.confidence_thresholds[:8]] == thr
    assert lg.confidence_threshold(3) == lg.confidence_thresholds[3]
    lg.conf["n_layers"] = -1  # the formula leaves [0, 1] only for a negative layer count: 0.8 + 0.1 e^(4 i)
    assert lg.confidence_threshold(2) == 1.0 and lg.confidence_threshold(0) == pytest.approx(0.9)


def test_float32_decision():
    # n + m = 64, depth_confidence = 0.75: r = 1 - below / 64 is exact in float32; 16 -> 0.75 (not above), 15 -> 0.765625
    assert not R.decide(16, 64, 0.75) and R.decide(15, 64, 0.75)
    assert R.ratio(16, 64) == np.float32(0.75) and R.ratio(15, 64).dtype == np.float32
    # depth_confidence is rounded to float32 before the comparison: r = 1 - 2/5 = float32(0.6) does not exceed the double 0.6,
    # whose float32 it equals (float32(0.6) > 0.6 as doubles)
    assert R.ratio(2, 5) == np.float32(0.6) and float(R.ratio(2, 5)) > 0.6 and not R.decide(2, 5, 0.6)
    assert R.decide(0, 2, 0.99) and not R.decide(1, 2, 0.5)
    # safety: the same decision over [below - near, below + near]
    assert R.safe(15, 0, 64, 0.75) and not R.safe(15, 1, 64, 0.75) and R.safe(10, 5, 64, 0.75) and R.safe(40, 3, 64, 0.75)


@pytest.fixture(scope="module")
def restated():
    sd = lgf64_shipped_state_dict(7)
    out = {}
    for n, m in COUNTS:
        d0, d1, k0, k1 = lgf64_pair(11, n, m)
        out[(n, m)] = (sd, (k0, d0, k1, d1))
    return out


@pytest.mark.parametrize("depth,expect", [(0.15, 2), (0.25, 8), (0.5, 9)])
def test_restatement_stop_on_the_shipped_model(restated, depth, expect):
    """r is 0.17-0.21 after layer 1, 0.30-0.39 after layer 7 and below 0.12 elsewhere: a depth_confidence between the bands stops
    every pair at 2, at 8, or never; float32 and float64 runs count the same"""
    for (n, m), (sd, pair) in restated.items():
        r64 = R.run(sd, *pair, depth)
        assert all(r64["safe"]), ((n, m), r64)
        assert r64["stop"] == expect, ((n, m), r64["stop"], r64["r"])
        if (n, m) == (31, 33):
            r32 = R.run(sd, *pair, depth, dtype=torch.float32)
            assert r32["stop"] == expect and r32["below"] == r64["below"]
        assert r64["log_assignment"].shape == (n + 1, m + 1) and r64["x0"].shape == (n, 256)


def test_restatement_uses_the_stopping_head(restated):
    import lg_f64
    sd, pair = restated[(31, 33)]
    r = R.run(sd, *pair, 0.15)
    t = R.truncated_state_dict(sd, r["stop"])
    assert "log_assignment.1.final_proj.weight" in t and "log_assignment.2.final_proj.weight" not in t
    assert "token_confidence.0.token.0.weight" in t and "token_confidence.1.token.0.weight" not in t
    full = lg_f64.forward(t, *pair)
    assert len(full["layers"]) == 2 and np.array_equal(full["log_assignment"], r["log_assignment"])
    assert np.array_equal(full["matches0"], r["matches0"])
    assert R.run(sd, pair[0][:0], pair[1][:0], pair[2], pair[3], 0.15)["stop"] == 0


def test_package_defaults_and_refusals():
    lg = pkg.LightGlue({"depth_confidence": 0.95}).eval()
    assert lg.early_stop is False and not lg.early_stop_active()  # the reference ignores the key: opt-in
    lg.early_stop = True
    assert lg.early_stop_active()
    lg.conf["depth_confidence"] = -1  # read at every call
    assert not lg.early_stop_active()
    lg.conf["depth_confidence"] = 0.95
    lg.train()
    assert not lg.early_stop_active()
    lg.eval()
    lg.conf["width_confidence"] = 0.99
    with pytest.raises(NotImplementedError, match="8h"):
        lg.early_stop_active()
    lg.early_stop = False
    assert not lg.early_stop_active()


def test_loss_refuses_early_stopped_pred():
    lg = pkg.LightGlue({}).eval()
    pred = {"stop": torch.tensor([3]), "ref_descriptors0": torch.zeros(1, 1, 4, 256), "ref_descriptors1": torch.zeros(1, 1, 4, 256)}
    with pytest.raises(ValueError, match="stop"):
        lg.loss(pred, {"gt_matches0": torch.zeros(1, 4), "gt_matches1": torch.zeros(1, 4)})


def test_evaluator_reports_stop_layer_only_when_present():
    ev = H.SameTimeEvaluator(None, 5)
    rows = torch.zeros(3, len(ev.names), dtype=torch.float64)
    ev._metric_mean.add(rows)
    ev._account_stop(types.SimpleNamespace(stop=None))
    assert "matcher_stop_layer" not in ev.result()
    ev._account_stop(types.SimpleNamespace(stop=torch.tensor([2, 9, 0], dtype=torch.int32)))
    ev._account_stop(types.SimpleNamespace(stop=torch.tensor([4], dtype=torch.int32)))
    assert ev.result()["matcher_stop_layer"] == pytest.approx(15 / 4)


def test_different_time_evaluator_refuses_matcher_loss_with_early_stop():
    lg = pkg.LightGlue({"depth_confidence": 0.9}).eval()
    model = types.SimpleNamespace(matcher=types.SimpleNamespace(matcher=lg))
    ev = H.DifferentTimeEvaluator(model, 5, matcher_loss=True)
    batch = H._Batch([], None)
    ev._validate(batch)  # early stopping off: nothing to refuse
    lg.early_stop = True
    with pytest.raises(ValueError, match="early stopping"):
        ev._validate(batch)
