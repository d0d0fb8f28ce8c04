"""LightGlue.loss in eval mode, the parts that need no GPU: the float64 restatement (tests/lg_loss_ref.py) against
the reference's recorded values (tests/golden/lg_loss.npz), the mirrored refusals, the dense torch NLLLoss against the
restatement, and the evaluator's new keys on fake rows.

Bound (no new constant): every nll* value is a mean of log_assignment entries, so it is held to the bound this project puts on
those entries against float64 on identical inputs, helpers.la_bound_f64([the float32 peer's error], max |la|); row_norm is a mean
of sums of exp(la) and is held to that bound times max(1, row_norm); the counts are compared exactly."""
import types
from importlib import import_module

import numpy as np
import pytest
import torch

import lg_loss_ref as R
from helpers import Golden, close_and_record, la_bound_f64, load_pkg, state_dict_for

pkg = load_pkg()
LGM = import_module(pkg.__name__ + ".core.modules.matchers.lightglue")
H = import_module(pkg.__name__ + ".harness")
GT = import_module(pkg.__name__ + ".core.geometry.gt_generation")
G = Golden("lg_loss")
FAIL = G.meta["failures"]
COUNT_KEYS = ("num_matchable", "num_unmatchable")


def case_bound(c):
    return la_bound_f64([c["peer_la_err"]], c["la_absmax"])


def check_values(tag, got, exp, bound):
    """got / exp: [.., 8] in LOSS_KEYS order; exp the float64 restatement (or the reference)"""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    for i, k in enumerate(R.LOSS_KEYS):
        if k in COUNT_KEYS:
            assert np.array_equal(got[..., i], exp[..., i]), (tag, k, got[..., i], exp[..., i])
        elif k == "row_norm":
            close_and_record(f"{tag}.row_norm", got[..., i], exp[..., i], atol=bound * max(1.0, float(np.nanmax(np.abs(exp[..., i])))))
        else:
            close_and_record(f"{tag}.{k}", got[..., i], exp[..., i], atol=bound)


def restated(c):
    """the float64 restatement of a fixture case on the reference's stored descriptors: ([B,8] values, [B,8] sums)"""
    sd = state_dict_for(c)
    head = R.head_dict(sd, f"log_assignment.{c['n_layers'] - 1}.")
    vals, rows = [], []
    for b, kind in enumerate(c["kinds"]):
        gt0, gt1, pos0 = R.labels(kind, c["n"], c["m"])
        v, r8, _ = R.loss(G[f"{c['name']}.ref0"][b], G[f"{c['name']}.ref1"][b], head, gt0, gt1, R.scatter(pos0, c["m"]))
        vals.append([v[k] for k in R.LOSS_KEYS]), rows.append(r8)
    return np.array(vals), np.array(rows)


@pytest.mark.parametrize("name", list(G.cases))
def test_restatement_agrees_with_the_reference(name):
    c = G.cases[name]
    vals, rows = restated(c)
    assert np.array_equal(vals, G[f"{name}.f64_values"], equal_nan=True) or np.allclose(vals, G[f"{name}.f64_values"], rtol=1e-12, atol=1e-12)
    assert np.allclose(rows, G[f"{name}.f64_sums"], rtol=1e-12, atol=1e-12)
    check_values(f"lg_loss.f64_vs_reference.{name}", G[f"{name}.ref_values"], vals, case_bound(c))
    assert c["f64_vs_ref"] < case_bound(c)


def test_label_recipes_cover_what_they_claim():
    gt0, gt1, pos0 = R.labels("edges", 130, 130)
    W = R.scatter(pos0, 130)
    assert W[126, 127] and W[127, 128] and W[128, 127] and W[129, 128] and W.sum(1).max() == 1
    both = (pos0 >= 0) & (gt0 == -1)
    assert both.any() and (gt0 == -2).any() and (gt1 == -1).any() and (gt1 == -2).any() and (gt1 >= 0).any()
    g0, g1, p = R.labels("nopos", 70, 200)
    assert (p == -1).all() and set(g0) == {-1, -2} and set(g1) == {-1, -2}
    g0, g1, p = R.labels("ignore", 9, 5)
    assert (p == -1).all() and (g0 == -2).all() and (g1 == -2).all()
    M = R.dense_multi(40, 50)
    assert M.sum(1).max() > 1 and set(np.unique(M)) == {0, 1}
    # the sums of an all-ignored pair: nothing but row_sum and n
    la = np.log(np.full((10, 6), 0.1))
    s = R.sums(la, g0, g1, R.scatter(p, 5))
    assert (s[:6] == 0).all() and s[7] == 9 and np.isclose(s[6], 9 * 6 * 0.1)
    assert np.isnan(list(R.values(np.zeros(8)).values())).all()


# ---- the refusals ----------------------------------------------------------------------------------------------------------
def _small_model():
    return LGM.LightGlue({"input_dim": 64, "descriptor_dim": 64, "num_heads": 2, "n_layers": 2}).eval()


def _fake(B, n, m, layers=1, d=64):
    pred = {"ref_descriptors0": torch.zeros(B, layers, n, d), "ref_descriptors1": torch.zeros(B, layers, m, d)}
    data = {"gt_matches0": torch.full((B, n), -1), "gt_matches1": torch.full((B, m), -1), "gt_assignment": torch.zeros(B, n, m, dtype=torch.bool)}
    return pred, data


@pytest.mark.parametrize("tag", ["n_gt_m", "n_lt_m"])
def test_unequal_counts_raise_the_reference_error(tag):
    f = FAIL[tag]
    assert f["raises"] == "RuntimeError"
    err = LGM.nll_size_error(f["B"], f["n"], f["m"])
    assert type(err).__name__ == f["raises"] and str(err) == f["message"]
    with pytest.raises(RuntimeError) as e:
        _small_model().loss(*_fake(f["B"], f["n"], f["m"]))
    assert str(e.value) == f["message"]
    # the dense NLLLoss fails by itself, in the same assignment as the reference's
    pred, data = _fake(f["B"], f["n"], f["m"])
    with pytest.raises(RuntimeError) as e:
        LGM.NLLLoss({})({"log_assignment": torch.zeros(f["B"], f["n"] + 1, f["m"] + 1)}, data)
    assert str(e.value) == f["message"]


def test_equal_counts_and_n_is_m_plus_one():
    assert LGM.nll_size_error(2, 7, 7) is None and LGM.nll_size_error(2, 1, 1) is None
    e = LGM.nll_size_error(3, 8, 7)  # the slice :8 of 8 columns
    assert "(8)" in str(e) and "(7)" in str(e) and "[3, 8]" in str(e) and "[3, 7]" in str(e)
    with pytest.raises(RuntimeError) as t:
        LGM.NLLLoss({})({"log_assignment": torch.zeros(3, 9, 8)}, _fake(3, 8, 7)[1])
    assert str(t.value) == str(e)


def test_one_column_is_refused_where_the_reference_broadcasts():
    f = FAIL["m_is_1"]
    assert f["raises"] is None and f["m"] == 1 < f["n"]  # the reference returns values there
    with pytest.raises(NotImplementedError, match="broadcast"):
        _small_model().loss(*_fake(f["B"], f["n"], f["m"]))


def test_two_layers_in_eval_mode_raise_the_reference_key_error():
    f = FAIL["eval_two_layers"]
    assert f["raises"] == "KeyError"
    with pytest.raises(KeyError) as e:
        _small_model().loss(*_fake(2, 12, 12, layers=2))
    assert e.value.args[0] == f["arg"] and str(e.value) == f["message"]


def test_training_mode_is_refused_and_names_the_design_section():
    assert FAIL["training"]["raises"] is None and "confidence" in FAIL["training"]["keys"]
    with pytest.raises(NotImplementedError, match="DESIGN.md 8"):
        _small_model().train().loss(*_fake(2, 12, 12, layers=2))


def test_loss_conf_is_merged_over_the_reference_defaults():
    lg = LGM.LightGlue({"input_dim": 64, "descriptor_dim": 64, "num_heads": 2, "n_layers": 1, "loss": {"nll_balancing": 0.25}})
    assert lg.conf.loss.nll_balancing == 0.25 and lg.conf.loss.gamma == 1.0 and lg.conf.loss.fn == "nll"
    assert isinstance(lg.loss_fn, LGM.NLLLoss) and lg.loss_fn.conf.nll_balancing == 0.25 and lg.loss_fn.conf.gamma_f == 0.0
    assert LGM.NLLLoss({}).conf == {"nll_balancing": 0.5, "gamma_f": 0.0}
    assert not [k for k in lg.state_dict() if k.startswith("loss_fn")]


# ---- the dense torch NLLLoss against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.cases))
@pytest.mark.parametrize("balancing", [0.5, 0.3])
def test_dense_nll_loss_agrees_with_the_restatement(name, balancing):
    c = G.cases[name]
    sd = state_dict_for(c)
    head = R.head_dict(sd, f"log_assignment.{c['n_layers'] - 1}.")
    las, data, exp = [], {"gt_matches0": [], "gt_matches1": [], "gt_assignment": []}, []
    for b, kind in enumerate(c["kinds"]):
        gt0, gt1, pos0 = R.labels(kind, c["n"], c["m"])
        W = R.dense_multi(c["n"], c["m"]) if b == 0 else R.scatter(pos0, c["m"])  # any 0/1 matrix
        v, _, la = R.loss(G[f"{name}.ref0"][b], G[f"{name}.ref1"][b], head, gt0, gt1, W, balancing)
        las.append(la), exp.append(v)
        for k, a in zip(data, (gt0, gt1, W.astype(bool))):
            data[k].append(a)
    data = {k: torch.from_numpy(np.stack(v)) for k, v in data.items()}
    nll, weights, d = LGM.NLLLoss({"nll_balancing": balancing})({"log_assignment": torch.from_numpy(np.stack(las))}, data)
    assert list(d) == ["assignment_nll", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable"] and d["assignment_nll"] is nll
    assert weights.shape == (len(las), c["n"] + 1, c["m"] + 1)
    for k in d:  # float64 in, float64 out: the two differ by summation order only
        np.testing.assert_allclose(d[k].numpy(), [e[k] for e in exp], rtol=1e-12, atol=1e-12, err_msg=k)
    # given weights are used as they are
    nll2, w2, _ = LGM.NLLLoss({"nll_balancing": balancing})({"log_assignment": torch.from_numpy(np.stack(las))}, None, weights=weights)
    assert w2 is weights and torch.equal(nll2, nll)


# ---- lazy gt_assignment helpers ---------------------------------------------------------------------------------------------
def test_lazy_assignment_keeps_pos0_and_prefixed_keeps_it_lazy():
    pos0 = torch.tensor([[2, -1, 0]], dtype=torch.int32)
    d = GT.FeatsDict()
    d.update({"assignment": GT._LazyAssignment(pos0, 4), "matches0": torch.tensor([[2, -1, 0]])})
    g = GT.prefixed(d)
    assert list(g) == ["gt_assignment", "gt_matches0"] and g.lazy_keys() == ["gt_assignment"] and d.lazy_keys() == ["assignment"]
    assert GT.lazy_pos0(g, "gt_assignment") is pos0 and GT.lazy_pos0(d) is pos0 and g.lazy_keys() == ["gt_assignment"]
    a = g["gt_assignment"]
    assert a.dtype == torch.bool and a.tolist() == [[[False, False, True, False], [False] * 4, [True, False, False, False]]]
    assert GT.lazy_pos0(g, "gt_assignment") is None and GT.lazy_pos0({"gt_assignment": a}, "gt_assignment") is None
    assert GT.lazy_pos0({f"gt_{k}": v for k, v in d.items()}, "gt_assignment") is None  # val_matcher.py:82 resolves it


# ---- the evaluator ----------------------------------------------------------------------------------------------------------
def test_matcher_loss_rows_and_result_keys_on_fake_rows():
    rows = torch.tensor([[-6.0, 3.0, -2.0, 4.0, -1.0, 2.0, 5.0, 10.0],   # a pair with everything
                         [0.0, 0.0, -3.0, 1.0, 0.0, 0.0, 4.0, 8.0],      # no positive, no -1 column
                         [0.0] * 8], dtype=torch.float64)                   # no keypoints on a side: n = 0
    got = H.matcher_loss_rows(rows, 0.25)
    assert got.dtype == torch.float64 and got.shape == (3, 4)
    exp = [[R.values(r.numpy(), 0.25)[k] for k in ("total", "nll_pos", "nll_neg", "row_norm")] for r in rows]
    assert np.array_equal(got.numpy(), np.array(exp), equal_nan=True)
    assert got[0].tolist() == [0.25 * 2.0 + 0.75 * 0.5, 2.0, 0.5, 0.5] and got[1].tolist() == [0.75 * 1.5, 0.0, 1.5, 0.5]
    assert torch.isnan(got[2]).all()

    lg = types.SimpleNamespace(matcher=types.SimpleNamespace(matcher=_small_model()))
    ev = pkg.DifferentTimeEvaluator(lg, 5, matcher_loss=True)
    metric = torch.from_numpy(np.arange(2 * len(ev.names), dtype=np.float64).reshape(2, -1) / 8.0)
    ev._metric_mean.add(metric)
    before = ev.result()
    assert list(before) == list(ev.names)  # nothing labelled yet: no new key
    ev._nll_mean.add(got[:2])
    ev._nll_mean.add(got[2:])
    res = ev.result()
    assert list(res) == list(ev.names) + list(H.MATCHER_LOSS_NAMES)
    assert H.MATCHER_LOSS_NAMES == ("matcher_loss", "matcher_nll_pos", "matcher_nll_neg", "matcher_row_norm")
    for i, k in enumerate(H.MATCHER_LOSS_NAMES):  # the mean over the two pairs that have a value
        assert res[k] == float((got[0, i] + got[1, i]) / 2), k
    # the default evaluator has no such key whatever it is fed, and its other keys are the same
    ev0 = pkg.DifferentTimeEvaluator(lg, 5)
    ev0._metric_mean.add(metric)
    ev0._nll_mean.add(got)
    assert ev0.result() == before


def test_matcher_loss_needs_a_lightglue_matcher():
    mnn = types.SimpleNamespace(matcher=import_module(pkg.__name__ + ".core.modules.Matchers").Matcher(pkg.default_config("SP_MNN"), None, device="cpu"))
    with pytest.raises(ValueError, match="LightGlue"):
        pkg.DifferentTimeEvaluator(mnn, 5, matcher_loss=True)
    pkg.DifferentTimeEvaluator(mnn, 5)  # the default asks nothing of the matcher
    with pytest.raises(ValueError, match="LightGlue"):
        pkg.DifferentTimeEvaluator(types.SimpleNamespace(matcher=types.SimpleNamespace(matcher=None)), 5, matcher_loss=True)
