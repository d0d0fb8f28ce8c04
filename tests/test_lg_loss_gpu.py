"""GPU tests (-m gpu), component: LightGlue.loss in eval mode on the device (einx_lg_assign_nll in csrc/lightglue.hip)
against the float64 restatement (tests/lg_loss_ref.py on tests/lg_f64.py) and the reference's recorded values
(tests/golden/lg_loss.npz).

Bound (no new constant): every nll* value is a mean of log_assignment entries, so it is held to the bound this project puts on
those entries against float64 on identical inputs, helpers.la_bound_f64([error of lg_f64's float32 run on the same inputs],
max |la|); row_norm is a mean of sums of exp(la) and is held to that bound times max(1, row_norm_f64); counts are compared exactly."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import gt_matches_ref as GR
import lg_loss_ref as R
from helpers import Golden, close_and_record, la_bound_f64, lg_inputs, state_dict_for, synth, synth_raw_events
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu

N = pkg.native
LGM = import_module(pkg.__name__ + ".core.modules.matchers.lightglue")
GT = import_module(pkg.__name__ + ".core.geometry.gt_generation")
H = import_module(pkg.__name__ + ".harness")
G = Golden("lg_loss")
FAIL = G.meta["failures"]
COUNT_KEYS = ("num_matchable", "num_unmatchable")
GUARD, PATTERN = 4096, 0xA5
_SD = {}


def _sd(name):
    if name not in _SD:
        _SD[name] = state_dict_for(G.cases[name])
    return _SD[name]


def _head(name):
    c = G.cases[name]
    return R.head_dict(_sd(name), f"log_assignment.{c['n_layers'] - 1}.")


def _head_dev(head):
    return tuple(_t(head[k]) for k in ("final_proj.weight", "final_proj.bias", "matchability.weight", "matchability.bias"))


def check_values(tag, got, exp, bound):
    """got / exp: {key: value} of R.LOSS_KEYS for one pair; exp the float64 restatement (or the reference)"""
    for k in R.LOSS_KEYS:
        g, e = float(got[k]), float(exp[k])
        if np.isnan(e):
            assert np.isnan(g), (tag, k, g)
        elif k in COUNT_KEYS:
            assert g == e, (tag, k, g, e)
        else:
            close_and_record(f"{tag}.{k}", [g], [e], atol=bound * (max(1.0, abs(e)) if k == "row_norm" else 1.0))


def restate(x0, x1, head, gt0, gt1, W, balancing=0.5):
    """one pair on the CPU: (float64 values, float64 sums, the bound from the float32 peer on the same inputs)"""
    v, rows, la = R.loss(x0, x1, head, gt0, gt1, W, balancing)
    la32 = R.log_assignment(x0, x1, head, torch.float32)
    return v, rows, la_bound_f64([np.abs(la32.astype(np.float64) - la).max()], np.abs(la).max())


@pytest.fixture
def guards(monkeypatch):
    made = []

    def guarded(nbytes, device):
        nbytes = int(nbytes)
        buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=device)
        buf[nbytes:] = PATTERN
        made.append((nbytes, buf[nbytes:]))
        return buf[:nbytes]

    monkeypatch.setattr(N, "_workspace", guarded)
    return made


def _intact(made, at_least):
    torch.cuda.synchronize()
    assert len(made) >= at_least
    for nbytes, tail in made:
        assert int((tail != PATTERN).sum()) == 0, f"guard bytes behind a workspace of {nbytes} bytes were overwritten"


# ------------------------------------------------------------------------------------------------ the op against float64
def _batch(model, cap0, cap1, ns, ms, kinds, seed):
    """padded inputs of one op call: rows past a pair's count hold what would show if the counts were not honoured (NaN
    descriptors, -1 labels, positives)"""
    d = G.cases[model]["descriptor_dim"]
    B = len(ns)
    x0, x1 = np.full((B, cap0, d), np.nan, np.float32), np.full((B, cap1, d), np.nan, np.float32)
    gt0, gt1 = np.full((B, cap0), -1, np.int64), np.full((B, cap1), -1, np.int64)
    pos0, W = np.zeros((B, cap0), np.int32), np.ones((B, cap0, cap1), np.uint8)
    pairs = []
    for b, (n, m, kind) in enumerate(zip(ns, ms, kinds)):
        if n and m:
            a0, a1, _, _ = lg_inputs(dict(seed=seed + 7 * b, n=n, m=m, input_dim=d, shared=min(n, m) // 2))
            g0, g1, p = R.labels(kind, n, m)
            x0[b, :n], x1[b, :m], gt0[b, :n], gt1[b, :m], pos0[b, :n] = a0, a1, g0, g1, p
            W[b, :n, :m] = R.scatter(p, m)
            pairs.append((a0, a1, g0, g1, p))
        else:
            pairs.append(None)
    return x0, x1, gt0, gt1, pos0, W, pairs


OP_CASES = [
    # tag, model, cap0, cap1, n, m, kinds
    ("130x130", "d256", 130, 130, [130], [130], ["edges"]),
    ("70x200", "d64", 70, 200, [70], [200], ["edges"]),
    ("1x1", "d64", 1, 1, [1], [1], ["edges"]),
    ("129x64", "d256", 129, 64, [129], [64], ["edges"]),
    ("130x130.d64", "d64", 130, 130, [130, 130], [130, 130], ["nopos", "ignore"]),
    ("ragged", "d64", 256, 256, [256, 130, 1, 0], [200, 256, 1, 50], ["edges", "edges", "edges", "edges"]),
    ("ragged.m0", "d256", 256, 256, [256, 40], [256, 0], ["edges", "edges"]),
    ("1024x1023", "d256", 1024, 1023, [1024], [1023], ["edges"]),
]


@pytest.mark.parametrize("case", OP_CASES, ids=[c[0] for c in OP_CASES])
def test_op_against_float64(case, guards):
    tag, model, cap0, cap1, ns, ms, kinds = case
    head = _head(model)
    x0, x1, gt0, gt1, pos0, W, pairs = _batch(model, cap0, cap1, ns, ms, kinds, seed=900 + cap0)
    hd = _head_dev(head)
    n, m = _t(np.array(ns, np.int32)), _t(np.array(ms, np.int32))
    call = lambda **kw: N.lg_assign_nll(hd, _t(x0), _t(x1), _t(gt0), _t(gt1), n=n, m=m, **kw)  # noqa: E731
    rows = call(pos0=_t(pos0))
    again = call(pos0=_t(pos0))
    dense = call(assignment=_t(W).bool())
    dense_t = call(assignment=_t(np.ascontiguousarray(W.transpose(0, 2, 1))).transpose(1, 2))  # other strides, same matrix
    _intact(guards, at_least=4)
    assert rows.dtype == torch.float64 and rows.shape == (len(ns), 8)
    r = _np(rows)
    assert r.tobytes() == _np(again).tobytes()  # two calls in a row: the same bits
    assert r.tobytes() == _np(dense).tobytes() == _np(dense_t).tobytes()  # the scatter of pos0 as a dense matrix: the same bits
    vals, row_norm = N.lg_nll_values(rows, 0.5)
    vals, row_norm = _np(vals), _np(row_norm)
    for b, p in enumerate(pairs):
        if p is None:
            assert (r[b] == 0).all() and np.isnan(vals[b]).all() and np.isnan(row_norm[b])
            continue
        a0, a1, g0, g1, ps = p
        v, s, bound = restate(a0, a1, head, g0, g1, R.scatter(ps, ms[b]))
        assert [r[b, 1], r[b, 3], r[b, 5], r[b, 7]] == [s[1], s[3], s[5], s[7]], (tag, b, r[b], s)  # the counts, exactly
        got = dict(zip(("total", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable"), vals[b]), row_norm=row_norm[b])
        got["last"] = got["assignment_nll"] = got["total"]
        check_values(f"lg_loss.op.{tag}", got, v, bound)


def test_op_dense_form_takes_any_zero_one_matrix():
    """several positives in a row, and a balancing other than 1/2"""
    head = _head("d64")
    n, m = 140, 150
    a0, a1, _, _ = lg_inputs(dict(seed=77, n=n, m=m, input_dim=64, shared=60))
    g0, g1, _ = R.labels("edges", n, m)
    W = R.dense_multi(n, m)
    rows = N.lg_assign_nll(_head_dev(head), _t(a0[None]), _t(a1[None]), _t(g0[None]), _t(g1[None]), assignment=_t(W[None]))
    v, s, bound = restate(a0, a1, head, g0, g1, W, 0.3)
    assert _np(rows)[0, 1] == s[1] == W.sum() and W.sum(1).max() > 1
    vals, row_norm = N.lg_nll_values(rows, 0.3)
    got = dict(zip(("total", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable"), _np(vals)[0]), row_norm=_np(row_norm)[0])
    got["last"] = got["assignment_nll"] = got["total"]
    check_values("lg_loss.op.dense_multi", got, v, bound)


def test_op_graph_capture_and_replay():
    """the raw call captured in a graph and replayed twice into a poisoned workspace and output: the eager bits"""
    head = _head("d64")
    x0, x1, gt0, gt1, pos0, W, _ = _batch("d64", 256, 256, [256, 130, 1, 0], [200, 256, 1, 50], ["edges"] * 4, seed=1156)
    t = dict(x0=_t(x0), x1=_t(x1), gt0=_t(gt0), gt1=_t(gt1), pos0=_t(pos0), n=_t(np.array([256, 130, 1, 0], np.int32)),
             m=_t(np.array([200, 256, 1, 50], np.int32)))
    hd = _head_dev(head)
    eager = _np(N.lg_assign_nll(hd, t["x0"], t["x1"], t["gt0"], t["gt1"], pos0=t["pos0"], n=t["n"], m=t["m"]))
    L, P = N.lib(), N._ptr
    need = L.einx_lg_assign_nll_ws_bytes(4, 256, 256, 64)
    assert need > 0
    ws = torch.empty(need + GUARD, dtype=torch.uint8, device=DEV)
    out = torch.empty((4, 8), dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        rc = L.einx_lg_assign_nll(*[P(w) for w in hd], 64, P(t["x0"]), P(t["n"]), 256, P(t["x1"]), P(t["m"]), 256, 4, P(t["gt0"]), P(t["gt1"]),
                                  P(t["pos0"]), None, 0, 0, 0, P(ws), P(out), N._stream(out))
    assert rc == 0
    for _ in range(2):
        ws[:need] = 0xAB
        ws[need:] = PATTERN
        out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert _np(out).tobytes() == eager.tobytes()
        assert int((ws[need:] != PATTERN).sum()) == 0


def test_op_refuses_bad_arguments():
    L = N.lib()
    assert L.einx_lg_assign_nll_ws_bytes(0, 8, 8, 64) == 0 and L.einx_lg_assign_nll_ws_bytes(1, 8, 8, 30) == 0
    assert L.einx_lg_assign_nll_ws_bytes(2, 130, 70, 64) > 0
    assert L.einx_lg_assign_nll(*[None] * 4, 64, None, None, 8, None, None, 8, 1, None, None, None, None, 0, 0, 0, None, None, None) == -1
    hd = _head_dev(_head("d64"))
    x, g = torch.zeros(1, 8, 64, device=DEV), torch.zeros(1, 8, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="one of the two"):
        N.lg_assign_nll(hd, x, x, g, g)
    with pytest.raises(ValueError, match="one of the two"):
        N.lg_assign_nll(hd, x, x, g, g, pos0=g.int(), assignment=torch.zeros(1, 8, 8, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError):
        N.lg_assign_nll(hd, x.cpu(), x.cpu(), g, g, pos0=g.int())  # there is no CPU path


# ------------------------------------------------------------------------------------------------ LightGlue.loss
def _model(name):
    c = G.cases[name]
    lg = LGM.LightGlue({k: c[k] for k in ("input_dim", "descriptor_dim", "num_heads", "n_layers")})
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(name).items()}, strict=False)
    return lg.to(DEV).eval()


def _fixture_call(name):
    c = G.cases[name]
    g0, g1, p = zip(*[R.labels(kind, c["n"], c["m"]) for kind in c["kinds"]])
    pos0 = _t(np.stack(p))
    gt = GT.FeatsDict()
    gt.update({"assignment": GT._LazyAssignment(pos0, c["m"]), "matches0": _t(np.stack(g0)), "matches1": _t(np.stack(g1))})
    pred = {"ref_descriptors0": _t(G[f"{name}.ref0"])[:, None], "ref_descriptors1": _t(G[f"{name}.ref1"])[:, None],
            "matches0": _t(np.stack(g0)).clamp_min(-1), "matching_scores0": torch.full((c["B"], c["n"]), 0.5, device=DEV)}
    return c, pred, GT.prefixed(gt)


@pytest.mark.parametrize("name", list(G.cases))
def test_loss_on_the_fixture(name):
    c, pred, data = _fixture_call(name)
    lg = _model(name)
    losses, metrics = lg.loss(pred, data)
    assert data.lazy_keys() == ["gt_assignment"]  # the lazy entry was handed over as pos0 and is still lazy
    assert list(losses) == list(R.LOSS_KEYS) == list(LGM.LOSS_KEYS)
    for k, v in losses.items():
        assert v.dtype == torch.float32 and v.shape == (c["B"],) and v.device.type == "cuda", k
    assert list(metrics) == ["match_recall", "match_precision", "accuracy", "average_precision"]
    assert all(torch.equal(metrics[k], LGM.matcher_metrics(pred, data)[k]) for k in metrics)
    assert torch.equal(losses["total"], losses["last"]) and torch.equal(losses["total"], losses["assignment_nll"])
    assert losses["last"].data_ptr() != losses["total"].data_ptr()  # `last` is a copy, as the reference's clone().detach()
    bound = la_bound_f64([c["peer_la_err"]], c["la_absmax"])
    for b in range(c["B"]):
        got = {k: float(losses[k][b]) for k in R.LOSS_KEYS}
        check_values(f"lg_loss.loss_vs_reference.{name}", got, dict(zip(R.LOSS_KEYS, G[f"{name}.ref_values"][b])), bound)
        check_values(f"lg_loss.loss_vs_f64.{name}", got, dict(zip(R.LOSS_KEYS, G[f"{name}.f64_values"][b])), bound)
    # resolved (val_matcher.py:82 goes through .items()): the dense form, the same values
    resolved = {k: v for k, v in data.items()}
    assert torch.is_tensor(resolved["gt_assignment"]) and resolved["gt_assignment"].dtype == torch.bool
    again, _ = lg.loss(pred, resolved)
    assert all(torch.equal(again[k], losses[k]) for k in losses)
    # another balancing is read from the conf at the call
    lg.conf.loss["nll_balancing"] = 0.25
    other, _ = lg.loss(pred, resolved)
    exp = 0.25 * losses["nll_pos"].double() + 0.75 * losses["nll_neg"].double()
    np.testing.assert_allclose(_np(other["total"]), _np(exp), rtol=1e-6, atol=1e-6)


def test_loss_follows_edited_head_weights():
    """the head's weights are read where the parameters live: an edit through .data shows in the next call"""
    c, pred, data = _fixture_call("d64")
    lg = _model("d64")
    before, _ = lg.loss(pred, data)
    head = lg.log_assignment[-1]
    head.matchability.bias.data += 1.0
    after, _ = lg.loss(pred, data)
    sd = dict(_sd("d64"))
    key = f"log_assignment.{c['n_layers'] - 1}.matchability.bias"
    sd[key] = sd[key] + np.float32(1.0)
    hd = R.head_dict(sd, f"log_assignment.{c['n_layers'] - 1}.")
    g0, g1, p = R.labels(c["kinds"][0], c["n"], c["m"])
    v, _, bound = restate(G["d64.ref0"][0], G["d64.ref1"][0], hd, g0, g1, R.scatter(p, c["m"]))
    assert not torch.equal(before["total"], after["total"])
    check_values("lg_loss.loss_edited_head", {k: float(after[k][0]) for k in R.LOSS_KEYS}, v, bound)


def test_loss_mirrors_the_reference_failures():
    lg = _model("d64")

    def fake(B, n, m, layers=1):
        pred = {"ref_descriptors0": torch.zeros(B, layers, n, 64, device=DEV), "ref_descriptors1": torch.zeros(B, layers, m, 64, device=DEV)}
        data = {"gt_matches0": torch.full((B, n), -1, device=DEV), "gt_matches1": torch.full((B, m), -1, device=DEV),
                "gt_assignment": torch.zeros(B, n, m, dtype=torch.bool, device=DEV)}
        return pred, data

    for tag in ("n_gt_m", "n_lt_m"):
        f = FAIL[tag]
        with pytest.raises(RuntimeError) as e:
            lg.loss(*fake(f["B"], f["n"], f["m"]))
        assert type(e.value).__name__ == f["raises"] and str(e.value) == f["message"]
    with pytest.raises(NotImplementedError, match="broadcast"):
        lg.loss(*fake(2, FAIL["m_is_1"]["n"], 1))
    with pytest.raises(KeyError) as e:
        lg.loss(*fake(2, 12, 12, layers=2))
    assert e.value.args[0] == FAIL["eval_two_layers"]["arg"]
    lg.train()
    with pytest.raises(NotImplementedError, match="DESIGN.md 8"):
        lg.loss(*fake(2, 12, 12, layers=2))
    lg.eval()


# ------------------------------------------------------------------------------------------------ end to end
def test_forward_gt_matches_loss_end_to_end():
    """model.eval(), forward, gt_matches_from_pose_depth, loss, as val_matcher.py:66-84 chains them, on an integer-built scene; the
    restatement is fed the forward's own ref_descriptors and the labels the ground-truth call returned"""
    name, B, n = "d64", 2, 96
    c = G.cases[name]
    lg = _model(name)
    sc = GR.scene(71, B, n, n, (120, 160), (120, 160), f0=128.0, f1=128.0, n_corr=40)
    feats = []
    for side in (0, 1):
        d = np.stack([lg_inputs(dict(seed=500 + b, n=n, m=n, input_dim=64, shared=40))[side] for b in range(B)])
        kp = np.concatenate([sc[f"kp{side}"], np.zeros((B, n, 1), np.float32)], -1)
        feats.append({"sparse_descriptors": _t(d), "sparse_positions": _t(kp), "image_size": [torch.tensor([120, 160])] * B})
    pred = lg(*feats)
    assert pred["ref_descriptors0"].shape == (B, 1, n, 64)
    gt = GT.gt_matches_from_pose_depth(_t(sc["kp0"]), _t(sc["kp1"]), _t(sc["K0"]), _t(sc["K1"]), _t(sc["depth0"]), _t(sc["depth1"]), _t(sc["T01"]),
                                       _t(sc["T10"]), ordering="xy")
    data = GT.prefixed(gt)
    losses, metrics = lg.loss(pred, data)
    assert "gt_assignment" in data.lazy_keys() and "assignment" in gt.lazy_keys()
    assert int((gt["matches0"] > -1).sum()) > 0
    resolved = {f"gt_{k}": v for k, v in gt.items()}  # the reference's line, which builds the dense entries
    again, metrics2 = lg.loss(pred, resolved)
    assert all(torch.equal(again[k], losses[k]) for k in losses) and all(torch.equal(metrics[k], metrics2[k]) for k in metrics)
    head = _head(name)
    for b in range(B):
        v, _, bound = restate(_np(pred["ref_descriptors0"])[b, 0], _np(pred["ref_descriptors1"])[b, 0], head, _np(gt["matches0"])[b],
                              _np(gt["matches1"])[b], _np(gt["assignment"])[b])
        check_values("lg_loss.e2e", {k: float(losses[k][b]) for k in R.LOSS_KEYS}, v, bound)
    exp_pr = np.stack([GR.match_pr(_np(pred["matches0"])[b], _np(gt["matches0"])[b], _np(pred["matching_scores0"])[b]) for b in range(B)])
    for i, k in enumerate(metrics):
        np.testing.assert_allclose(_np(metrics[k]), exp_pr[:, i], rtol=1e-6, atol=1e-7, err_msg=k)


# ------------------------------------------------------------------------------------------------ the evaluation harness
def test_different_time_evaluator_with_matcher_loss():
    """two batches of 4 synthetic pairs with scene depth and pose through an SP + LightGlue model (2 layers): result()'s new keys
    are the means of the restatement over the same pairs, fed the forward's last-layer descriptors and the batch's labels at each
    pair's own counts; the default evaluator's result() is what it was"""
    Hh, Wd, B, bins = 260, 346, 4, 5
    cfg = pkg.default_config("SP_LG", event_channels=bins)
    cfg.matcher.LightGlue.n_layers = 2
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=33)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    head = R.head_dict(sdn, "matcher.matcher.log_assignment.1.")
    with_loss = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh), matcher_loss=True)
    default = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh))
    with pytest.raises(ValueError, match="LightGlue"):
        pkg.DifferentTimeEvaluator(pkg.EIM(pkg.default_config("SP_MNN", event_channels=bins), device=DEV).eval(), bins=bins, matcher_loss=True)
    expect, bounds, counts = [], [], []
    for k in range(2):
        evs = [synth_raw_events(dict(seed=800 + 10 * k + b, n=20000 if b else 4000, H=Hh, W=Wd, bins=bins, frac=False, pneg=False)) for b in range(B)]
        img = synth.synth_image(95 + k, B, Hh, Wd)
        img[1, :, :, Wd // 2:] = 0  # a pair with fewer keypoints on the image side
        sc = GR.scene(45 + k, B, 4, 4, (Hh, Wd), (Hh, Wd), f0=256.0, f1=256.0, n_corr=0)
        pose, depth = (_t(sc["K0"]), _t(sc["K1"]), _t(sc["T01"])), (_t(sc["depth0"]), _t(sc["depth1"]))
        rows, (ef, imf, _) = with_loss.step(evs, _t(img.copy()), None, pose=pose, depth=depth)
        gt, mr = with_loss.last_gt, model._last_match
        n, m = _np(ef._batched.det.counts), _np(imf._batched.det.counts)
        x0, x1, g0, g1, p0 = _np(mr.ref0), _np(mr.ref1), _np(gt["matches0"]), _np(gt["matches1"]), _np(gt["pos0"])
        rows0, _ = default.step(evs, _t(img.copy()), None, pose=pose, depth=depth)
        assert _np(rows).tobytes() == _np(rows0).tobytes()
        for b in range(B):
            assert n[b] > 1 and m[b] > 1
            v, _, bound = restate(x0[b, :n[b]], x1[b, :m[b]], head, g0[b, :n[b]], g1[b, :m[b]], R.scatter(p0[b, :n[b]], m[b]))
            expect.append([v[k2] for k2 in ("total", "nll_pos", "nll_neg", "row_norm")])
            bounds.append(bound)
            counts.append((int(n[b]), int(m[b])))
    print("keypoint counts per pair:", counts)
    res, res0 = with_loss.result(), default.result()
    expect = np.array(expect)
    assert list(res)[-4:] == list(H.MATCHER_LOSS_NAMES) and not set(H.MATCHER_LOSS_NAMES) & set(res0)
    for i, k in enumerate(H.MATCHER_LOSS_NAMES):
        exp = float(expect[:, i].mean())
        close_and_record(f"lg_loss.harness.{k}", [res[k]], [exp], atol=max(bounds) * (max(1.0, abs(exp)) if k == "matcher_row_norm" else 1.0))
    assert list(res0) == [k for k in res if k not in H.MATCHER_LOSS_NAMES]
    assert all(np.array_equal(res[k], res0[k], equal_nan=True) for k in res0)  # every other key is what the default reports
