"""GPU tests (-m gpu), component: LightGlue early stopping, per-pair adaptive depth (einx_lightglue_early_stop).

The shipped model (d = 256, 4 x 64, 9 layers) with name-synthesised weights.  Its confidences put r = 1 - below / (n + m) near 0.2
after layer 1, near 0.3-0.4 after layer 7 and near 0 elsewhere for every pair, so two token biases are moved by INTEGERS (layer 3 by
+2, layer 7 by +1): with depth_confidence 0.7 the pairs (31,33) and (40,300) then stop after layer 3 (r 0.77 and 0.74, against
0.52-0.66 for the others), the rest after layer 7 (r >= 0.73); every decision any pair meets is at least four rows away from
flipping (measured on the CPU with the restatement; the one-row sides of (1,1) give r in {0, 0.5, 1}).  `stop` is compared
with the float64 restatement (tests/lg_early_stop_ref.py) only after asserting, on the CPU side, that every such decision is safe.
The outputs of a pair are compared BIT FOR BIT with the existing full-depth path on that pair alone, through a model truncated to
`stop` layers, and against float64 by the rules of tests/test_lightglue_f64_gpu.py::_check_pair on that truncated model."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import lg_early_stop_ref as R
import test_lightglue_f64_gpu as T
from helpers import lgf64_pair, lgf64_shipped_state_dict, state_dict_for, synth, synth_raw_events
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu
N = pkg.native
DEPTH = 0.7
SHIFTS = {3: 2.0, 7: 1.0}
SIZE = (260, 346)
STACKED = [(31, 33), (64, 64), (130, 130), (1, 1), (0, 5)]  # cap0 == cap1 == 130: the sides stacked, one launch over 2B entries
UNSTACKED = [(129, 300), (40, 300), (31, 33), (5, 0)]  # cap0 = 129, cap1 = 300: one launch per side
# The one cell of the GEMM launch table that no shipped-width case reaches at test sizes: EPI_DIV_HEAD on the WIDE
# kernel.  d = 96 (3 heads of 32) is no multiple of the small kernel's 64 columns, so every linear of this model runs lg_gemm_kernel
# whatever the grid; three layers, token bias 0 at -30 and 1 at +30: every pair with rows stops after layer 2, far from any
# threshold, and is read by head 1 (not the last one); the empty pair keeps stop = 0
OTHER_WIDTH = dict(input_dim=96, descriptor_dim=96, num_heads=3, n_layers=3)
OTHER_WIDTH_COUNTS = [(129, 130), (33, 1), (0, 130)]  # stacked at cap 130


def _state_dict(shifts=SHIFTS):
    sd = lgf64_shipped_state_dict(7)
    for i, s in shifts.items():
        sd[f"token_confidence.{i}.token.0.bias"] = sd[f"token_confidence.{i}.token.0.bias"] + np.float32(s)
    return sd


def _pair(b, n, m, seed=11):
    """(k0, d0, k1, d1, size0, size1); an empty side is cut from a pair that has rows"""
    d0, d1, k0, k1 = lgf64_pair(seed, max(n, 1), max(m, 1))
    return k0[:n], d0[:n], k1[:m], d1[:m], SIZE, SIZE


def _model(sd, n_layers=9, early_stop=True, depth=DEPTH):
    lg = T._model(dict(T.SHIPPED, n_layers=n_layers, depth_confidence=depth), sd)
    lg.early_stop = early_stop
    return lg


def _batches(pairs):
    cap0, cap1 = max(len(p[0]) for p in pairs), max(len(p[2]) for p in pairs)
    pb0 = T._batch([p[0] for p in pairs], [p[1] for p in pairs], cap0, SIZE)
    pb1 = T._batch([p[2] for p in pairs], [p[3] for p in pairs], cap1, SIZE, dfill=-3.0)
    return pb0, pb1


def _cut(r, b, n, m):
    """pair b of a MatchResult at its own counts"""
    return {"la": _np(r.la)[b, :n + 1, :m + 1], "m0": _np(r.matches0)[b, :n], "m1": _np(r.matches1)[b, :m], "s0": _np(r.scores0)[b, :n],
            "s1": _np(r.scores1)[b, :m], "ref0": _np(r.ref0)[b, :n], "ref1": _np(r.ref1)[b, :m], "layers": None}


def _same_bits(tag, a, b):
    empty = a["m0"].size == 0 or a["m1"].size == 0  # (an empty pair's log_assignment block is not written by either op)
    for k in ("m0", "m1", "s0", "s1", "ref0", "ref1") + (() if empty else ("la",)):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (tag, k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))


class World:
    """one run of each batch with early stopping on, the restatement of every pair and the truncated models, shared by the tests"""

    def __init__(self):
        self.sd = _state_dict()
        self.lg = _model(self.sd)
        self.truncated = {}
        self.cases = {}
        for name, counts in (("stacked", STACKED), ("unstacked", UNSTACKED)):
            pairs = [_pair(b, n, m) for b, (n, m) in enumerate(counts)]
            pb0, pb1 = _batches(pairs)
            n0, m0 = pb0.counts.clone(), pb1.counts.clone()
            r = self.lg.match_batched(pb0, pb1)
            torch.cuda.synchronize()
            assert torch.equal(pb0.counts, n0) and torch.equal(pb1.counts, m0)  # the caller's counts are never written
            ref = [R.run(self.sd, *p[:4], DEPTH) for p in pairs]
            self.cases[name] = dict(counts=counts, pairs=pairs, r=r, stop=_np(r.stop).tolist(), ref=ref, pb=(pb0, pb1))

    def other_width(self):
        """the d = 96 case, built when its test asks for it"""
        if "other_width" not in self.cases:
            probe = pkg.LightGlue(OTHER_WIDTH).to(DEV)
            sd = state_dict_for(dict(wseed=829, state_keys={k: list(v.shape) for k, v in probe.state_dict().items()}))
            for i, v in ((0, -30.0), (1, 30.0)):
                sd[f"token_confidence.{i}.token.0.bias"] = np.full_like(sd[f"token_confidence.{i}.token.0.bias"], v)
            lg = T._model(dict(OTHER_WIDTH, depth_confidence=DEPTH), sd)
            lg.early_stop = True
            pairs = []
            for b, (n, m) in enumerate(OTHER_WIDTH_COUNTS):
                d0, d1, k0, k1 = lgf64_pair(40 + b, max(n, 1), max(m, 1), 96)
                pairs.append((k0[:n], d0[:n], k1[:m], d1[:m], SIZE, SIZE))
            pb0 = T._batch([p[0] for p in pairs], [p[1] for p in pairs], 130, SIZE)
            pb1 = T._batch([p[2] for p in pairs], [p[3] for p in pairs], 130, SIZE, dfill=-3.0)
            r = lg.match_batched(pb0, pb1)
            torch.cuda.synchronize()
            ref = [R.run(sd, *p[:4], DEPTH) for p in pairs]
            self.cases["other_width"] = dict(counts=OTHER_WIDTH_COUNTS, pairs=pairs, r=r, stop=_np(r.stop).tolist(), ref=ref, pb=(pb0, pb1), sd=sd,
                                             conf=OTHER_WIDTH)
        return self.cases["other_width"]

    def model_of(self, stop):
        if stop not in self.truncated:
            self.truncated[stop] = _model(R.truncated_state_dict(self.sd, stop), n_layers=stop, early_stop=False)
        return self.truncated[stop]


@pytest.fixture(scope="module")
def world():
    return World()


def _alone(lg, pair):
    """the existing full-depth path on one pair, at its own capacities"""
    k0, d0, k1, d1 = pair[:4]
    n, m = len(k0), len(k1)
    r = lg.match_batched(T._batch([k0], [d0], n, SIZE), T._batch([k1], [d1], m, SIZE, dfill=-3.0))
    assert r.stop is None
    return _cut(r, 0, n, m)


# ------------------------------------------------------------------------------------------------ 1. the switch off
def test_switch_off_is_the_existing_op(world):
    """early_stop False, and early_stop True with depth_confidence -1: einx_lightglue, bit for bit; and the new op with a
    depth_confidence no ratio can exceed (nothing stops) gives einx_lightglue's bits with stop = n_layers"""
    for name in ("stacked", "unstacked"):
        c = world.cases[name]
        pb0, pb1 = c["pb"]
        off = _model(world.sd, early_stop=False)
        base = off.match_batched(pb0, pb1)
        assert base.stop is None
        minus = _model(world.sd, early_stop=True, depth=-1)
        r1 = minus.match_batched(pb0, pb1)
        assert r1.stop is None
        w, _, _, heads = off._pack()
        never = N.lightglue(w, pb0, pb1, want_la=True, want_ref=True, early_stop=(heads, 2.0))
        for b, (n, m) in enumerate(c["counts"]):
            _same_bits((name, b, "depth -1"), _cut(r1, b, n, m), _cut(base, b, n, m))
            _same_bits((name, b, "never"), _cut(never, b, n, m), _cut(base, b, n, m))
        assert _np(never.stop).tolist() == [9 if n and m else 0 for n, m in c["counts"]]


# ------------------------------------------------------------------------------------------------ 2. stop against the restatement
@pytest.mark.parametrize("name", ["stacked", "unstacked"])
def test_ragged_batch_stops_where_the_restatement_does(world, name):
    c = world.cases[name]
    for b, ref in enumerate(c["ref"]):
        assert all(ref["safe"]), (name, b, ref["below"], ref["near"], ref["r"])  # the margin condition, before any comparison
    print(name, "stop", c["stop"], "r per pair", [[round(v, 3) for v in ref["r"]] for ref in c["ref"]])
    assert c["stop"] == [ref["stop"] for ref in c["ref"]]
    stops = set(c["stop"])
    assert 0 in stops and len(stops - {0}) >= 2, stops  # an empty pair and pairs leaving at different layers


# ------------------------------------------------------------------------------------------------ 3. truncated-model equality
@pytest.mark.parametrize("name", ["stacked", "unstacked"])
def test_each_pair_equals_the_truncated_model_alone(world, name):
    """a pair that stopped after `stop` layers holds, bit for bit, what the existing full-depth path gives on that pair ALONE with a
    model of `stop` layers whose last head is log_assignment[stop - 1]: its rows were frozen and read by the right head"""
    c = world.cases[name]
    for b, (n, m) in enumerate(c["counts"]):
        got = _cut(c["r"], b, n, m)
        if c["stop"][b] == 0:
            assert (got["m0"] == -1).all() and (got["m1"] == -1).all() and not got["s0"].any() and not got["s1"].any()
            continue
        _same_bits((name, b, c["stop"][b]), got, _alone(world.model_of(c["stop"][b]), c["pairs"][b]))


# ------------------------------------------------------------------------------------------------ 4. against float64
@pytest.mark.parametrize("name", ["stacked", "unstacked", "other_width"])
def test_each_pair_against_float64(world, oracle, name):
    """the rules of test_lightglue_f64_gpu._check_pair (la_bound_f64 over the float32 peers, the float64 decision margins), applied
    with the truncated state dict: its full-depth float64 forward IS the restatement of a pair that stopped there.  other_width:
    the wide kernel's EPI_DIV_HEAD (see OTHER_WIDTH), every decision safe and as the restatement takes it"""
    c = world.other_width() if name == "other_width" else world.cases[name]
    sd, conf = c.get("sd", world.sd), c.get("conf", T.SHIPPED)
    if name == "other_width":
        assert all(all(ref["safe"]) for ref in c["ref"]) and c["stop"] == [ref["stop"] for ref in c["ref"]] == [2, 2, 0]
    for b, (n, m) in enumerate(c["counts"]):
        stop = c["stop"][b]
        if stop == 0:
            continue
        sdt = R.truncated_state_dict(sd, stop)
        ex = T._check_pair(f"lg_early_stop.{name}.{b}", sdt, dict(conf, n_layers=stop), c["pairs"][b], _cut(c["r"], b, n, m), oracle)
        assert np.array_equal(ex["log_assignment"], c["ref"][b]["log_assignment"])
        x0 = c["ref"][b]["x0"]
        assert np.abs(_cut(c["r"], b, n, m)["ref0"] - x0).max() <= 1e-3 * max(1.0, np.abs(x0).max())  # (a sanity check; the bits are test 3's)


# ------------------------------------------------------------------------------------------------ 5. / 6. one pair, edited weights
def _front_door(lg, pair):
    k0, d0, k1, d1 = pair[:4]
    out = lg(T._feats(k0, d0, SIZE), T._feats(k1, d1, SIZE))
    return out, {"la": _np(out["log_assignment"])[0], "m0": _np(out["matches0"])[0], "m1": _np(out["matches1"])[0],
                 "s0": _np(out["matching_scores0"])[0], "s1": _np(out["matching_scores1"])[0],
                 "ref0": _np(out["ref_descriptors0"])[0, 0], "ref1": _np(out["ref_descriptors1"])[0, 0]}


@pytest.mark.parametrize("n,m", [(31, 33), (64, 64)])
def test_single_pair_first_layer_middle_and_never(world, n, m):
    """B = 1 (lg_gemm_small_kernel, lg_attn16_kernel): stop = 1 after moving token bias 0 by +8 IN PLACE (an edited weight changes
    stop at the next forward), the middle of the model, and never (depth_confidence 0.99: bit-equal to early stopping off)"""
    pair = _pair(0 if (n, m) == (31, 33) else 1, n, m)
    lg = _model(world.sd)
    ref = R.run(world.sd, *pair[:4], DEPTH)
    assert all(ref["safe"]) and 1 < ref["stop"] < 9
    out, got = _front_door(lg, pair)
    assert _np(out["stop"]).tolist() == [ref["stop"]] and out["ref_descriptors0"].shape == (1, 1, n, 256)
    assert float(out["prune0"][0, 0]) == 9.0
    _same_bits("middle", got, _alone(world.model_of(ref["stop"]), pair))
    # edited in place: the version counter moves, _pack repacks
    with torch.no_grad():
        lg.token_confidence[0].token[0].bias.add_(8.0)
    sd1 = dict(world.sd)
    sd1["token_confidence.0.token.0.bias"] = world.sd["token_confidence.0.token.0.bias"] + np.float32(8.0)
    ref1 = R.run(sd1, *pair[:4], DEPTH)
    assert all(ref1["safe"]) and ref1["stop"] == 1
    out1, got1 = _front_door(lg, pair)
    assert _np(out1["stop"]).tolist() == [1]
    _same_bits("first", got1, _alone(world.model_of(1), pair))
    # edited through .data: found by the weight watch, the forward runs again on rebuilt images
    lg.token_confidence[0].token[0].bias.data.copy_(_t(world.sd["token_confidence.0.token.0.bias"]))
    out2, got2 = _front_door(lg, pair)
    assert _np(out2["stop"]).tolist() == [ref["stop"]]
    _same_bits("restored", got2, got)
    # never: read at every call
    lg.conf["depth_confidence"] = 0.99
    refn = R.run(world.sd, *pair[:4], 0.99)
    assert all(refn["safe"]) and refn["stop"] == 9
    outn, gotn = _front_door(lg, pair)
    assert _np(outn["stop"]).tolist() == [9]
    lg.early_stop = False
    outf, gotf = _front_door(lg, pair)
    assert "stop" not in outf
    _same_bits("never", gotn, gotf)


def test_stacked_forward_carries_stop(world):
    """LightGlue.forward on stacked [B,n,*] tensors (the reference's batched call)"""
    pairs = [_pair(b, 64, 64, seed=11 + 17 * b) for b in range(2)]
    feats = [{"sparse_descriptors": _t(np.stack([p[1 + 2 * s] for p in pairs])), "sparse_positions": _t(np.stack([p[2 * s] for p in pairs])),
              "image_size": [torch.tensor(SIZE)] * 2} for s in (0, 1)]
    out = world.lg(*feats)
    ref = [R.run(world.sd, *p[:4], DEPTH) for p in pairs]
    assert all(all(r["safe"]) for r in ref)
    assert out["stop"].dtype == torch.int32 and _np(out["stop"]).tolist() == [r["stop"] for r in ref]
    with pytest.raises(ValueError, match="stop"):
        world.lg.loss(out, {})


# ------------------------------------------------------------------------------------------------ 7. repeatability and memory
@pytest.mark.parametrize("name", ["stacked", "unstacked"])
def test_repeatable_capturable_and_inside_its_workspace(world, monkeypatch, name):
    GUARD, PATTERN = 4096, 0xA5
    made = []

    def guarded(nbytes, device):
        buf = torch.empty(int(nbytes) + GUARD, dtype=torch.uint8, device=device)
        buf[int(nbytes):] = PATTERN
        made.append(buf[int(nbytes):])
        return buf[:int(nbytes)]

    c = world.cases[name]
    pb0, pb1 = c["pb"]
    n0, m0 = pb0.counts.clone(), pb1.counts.clone()
    w, _, _, heads = world.lg._pack()
    call = lambda: N.lightglue(w, pb0, pb1, want_la=True, want_ref=True, early_stop=(heads, DEPTH))  # noqa: E731
    monkeypatch.setattr(N, "_workspace", guarded)
    a, b = call(), call()
    torch.cuda.synchronize()
    assert len(made) == 2 and all(bool((g == PATTERN).all()) for g in made)
    monkeypatch.undo()
    assert int(N.lib().einx_lightglue_early_stop_ws_bytes(pb0.B, pb0.cap, pb1.cap, 256, 4, 256, 9)) > \
        int(N.lib().einx_lg_ws_bytes_heads(pb0.B, pb0.cap, pb1.cap, 256, 4, 256))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call()  # warm-up on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        g = call()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pb0.counts, n0) and torch.equal(pb1.counts, m0)
    assert _np(a.stop).tolist() == c["stop"] == _np(b.stop).tolist() == _np(g.stop).tolist()
    for k, (n, m) in enumerate(c["counts"]):
        _same_bits((name, k, "second call"), _cut(b, k, n, m), _cut(a, k, n, m))
        _same_bits((name, k, "replay"), _cut(g, k, n, m), _cut(a, k, n, m))
        _same_bits((name, k, "world"), _cut(c["r"], k, n, m), _cut(a, k, n, m))


def test_native_refusals(world):
    pb0, pb1 = world.cases["stacked"]["pb"]
    w, _, _, heads = world.lg._pack()
    assert N.lib().einx_lightglue_early_stop_ws_bytes(2, 64, 64, 256, 4, 256, 33) == 0
    with pytest.raises(ValueError, match="every layer"):
        N.lightglue(w, pb0, pb1, all_layers=True, want_ref=True, early_stop=(heads, DEPTH))
    bad = (type(heads[0]) * 9)()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    rc = N.lib().einx_lightglue_early_stop(ctypes.byref(w), bad, ctypes.sizeof(type(heads[0])) + 8, 0.5, *([None] * 3), 64, *([None] * 3), 64, 2,
                                           1.0, 1.0, 1.0, 1.0, ws.data_ptr(), *([None] * 7), ws.data_ptr(), None)
    assert rc != 0 and b"head_size" in N.lib().einx_last_error()


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_matcher_eim_and_evaluator_carry_stop():
    """Matcher's frozen path, EIM.forward / forward_graph and DifferentTimeEvaluator over two ragged batches on an SP + LightGlue
    model (3 layers, token bias 1 moved by +8: whatever still runs leaves after layer 2)"""
    Hh, Wd, B, bins = 260, 346, 3, 5
    cfg = pkg.default_config("SP_LG", event_channels=bins)
    cfg.matcher.LightGlue.n_layers = 3
    cfg.matcher.LightGlue.depth_confidence = 0.5
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=33)
    sdn["matcher.matcher.token_confidence.1.token.0.bias"] = sdn["matcher.matcher.token_confidence.1.token.0.bias"] + np.float32(8.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    lg = model.matcher.matcher
    plain = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh))
    evs = [synth_raw_events(dict(seed=800 + b, n=20000 if b else 4000, H=Hh, W=Wd, bins=bins, frac=False, pneg=False)) for b in range(B)]
    img = synth.synth_image(95, B, Hh, Wd)
    _, (ef, imf, m_off) = plain.step(evs, _t(img.copy()))
    assert "stop" not in m_off and "matcher_stop_layer" not in plain.result()
    lg.early_stop = True
    with pytest.raises(ValueError, match="early stopping"):
        pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh), matcher_loss=True).step(evs, _t(img.copy()))
    m = model.matcher(ef, imf)  # the frozen path on the feature dicts
    assert len(m["stop"]) == B and all(1 <= int(s) <= 2 for s in m["stop"])
    rep, mask = plain.last_inputs
    _, _, m1 = model(rep, _t(img.copy()), mask)
    _, _, m2 = model.forward_graph(rep, _t(img.copy()), mask)
    assert [int(s) for s in m1["stop"]] == [int(s) for s in m["stop"]] == [int(s) for s in m2["stop"]]
    assert all(torch.equal(a, b) for a, b in zip(m1["matches0"], m2["matches0"]))
    before = len(model._graphs)
    lg.conf["depth_confidence"] = 0.25  # baked into a capture: a new graph
    model.forward_graph(rep, _t(img.copy()), mask)
    lg.early_stop = False
    _, _, m3 = model.forward_graph(rep, _t(img.copy()), mask)
    assert len(model._graphs) == before + 2 and "stop" not in m3
    lg.early_stop, lg.conf["depth_confidence"] = True, 0.5
    stepped = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh))
    seen = []
    for k in range(2):
        evs = [synth_raw_events(dict(seed=800 + 10 * k + b, n=20000 if b else 4000, H=Hh, W=Wd, bins=bins, frac=False, pneg=False)) for b in range(B)]
        img = synth.synth_image(95 + k, B, Hh, Wd)
        img[1, :, :, Wd // 2:] = 0  # a pair with fewer keypoints on the image side
        _, (_, _, mm) = stepped.step(evs, _t(img.copy()))
        seen += [int(s) for s in mm["stop"]]
    print("stop per pair:", seen)
    assert len(seen) == 2 * B and stepped.result()["matcher_stop_layer"] == pytest.approx(sum(seen) / len(seen), abs=1e-12)
