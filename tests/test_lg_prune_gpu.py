"""GPU tests (-m gpu), component: LightGlue point pruning, per-pair and per-side adaptive width (einx_lightglue_adaptive).

The shipped model (d = 256, 4 x 64, 9 layers) with name-synthesised weights.  Its matchability logits lie above -3.9 in every layer
on the fixed pairs, so with width_confidence = 0.99 (keep sigmoid > 0.01, logit > -4.6) nothing is pruned until two matchability
biases are moved: layer 1 by -5.78 (every side of the fixed pairs loses between a tenth and a quarter of its rows there) and layer 5 by
-5.52 (more than half of what is left).  Chosen on the CPU with the restatement (tests/lg_prune_ref.py): every row of every fixed
pair is at least 3.6e-5 away from the threshold at the two moved layers (NEAR = 1e-5), the other layers prune nothing, and the row
counts cross 128 (130 -> 117, 129 -> 116, 255 -> 97), 64 (64 -> 52, 117 -> 50) and 32 (33 -> 27, 40 -> 33 -> 13); the (1, 1) pair loses
both rows at layer 5 (a pair finished by an empty side) and side 0 of the single pair (5, 33) ends with exactly one row.  With early
stopping on as well (token bias 5 moved by +5, depth_confidence 0.95, matchability bias 5 by -5.6): the pair (31, 33) runs on (r = 0.94
after layer 5) and is pruned there, every other pair stops after layer 5 (r >= 0.96) and keeps the rows it had.
Every comparison with the restatement comes after asserting that each decision it took is SAFE."""
import ctypes

import numpy as np
import pytest
import torch

import lg_f64
import lg_prune_ref as P
import test_lightglue_f64_gpu as T
from helpers import close_and_record, la_bound_f64, lgf64_pair, lgf64_shipped_state_dict, record_flips, synth, synth_raw_events
from gpu_support import DEV, FTOL, _np, _t, pkg

pytestmark = pytest.mark.gpu
N = pkg.native
WIDTH = 0.99
MSHIFTS = {1: -5.78, 5: -5.52}
ES_MSHIFTS, ES_TSHIFTS, DEPTH = {1: -5.78, 5: -5.6}, {5: 5.0}, 0.95
SIZE = (260, 346)
L = 9
CASES = {  # name -> [(seed, n, m)]
    "stacked": [(11, 31, 33), (11, 64, 64), (11, 130, 130), (11, 1, 1), (11, 0, 5)],  # cap0 == cap1 == 130: one launch over 2B entries
    "unstacked": [(11, 129, 300), (11, 40, 300), (11, 31, 33), (11, 5, 0)],  # cap0 = 129, cap1 = 300: one launch per side
    "single": [(12, 5, 33)],  # B = 1 (the latency kernels); side 0 ends with one row
}


def _state_dict(mshifts=MSHIFTS, tshifts=None):
    sd = lgf64_shipped_state_dict(7)
    for i, s in mshifts.items():
        sd[f"log_assignment.{i}.matchability.bias"] = sd[f"log_assignment.{i}.matchability.bias"] + np.float32(s)
    for i, s in (tshifts or {}).items():
        sd[f"token_confidence.{i}.token.0.bias"] = sd[f"token_confidence.{i}.token.0.bias"] + np.float32(s)
    return sd


def _pair(seed, n, m):
    """(k0, d0, k1, d1, size0, size1); an empty side is cut from a pair that has rows"""
    d0, d1, k0, k1 = lgf64_pair(seed, max(n, 1), max(m, 1))
    return k0[:n], d0[:n], k1[:m], d1[:m], SIZE, SIZE


def _model(sd, pruning=True, width=WIDTH, depth=-1, min_kpts=0, n_layers=L):
    lg = T._model(dict(T.SHIPPED, n_layers=n_layers, depth_confidence=depth, width_confidence=width), sd)
    lg.point_pruning = pruning
    lg.early_stop = depth > 0
    if min_kpts is not None:
        lg.pruning_keypoint_thresholds["cuda"] = min_kpts
    return lg


def _batches(pairs):
    cap0, cap1 = max(max(len(p[0]) for p in pairs), 1), max(max(len(p[2]) for p in pairs), 1)
    pb0 = T._batch([p[0] for p in pairs], [p[1] for p in pairs], cap0, SIZE)
    pb1 = T._batch([p[2] for p in pairs], [p[3] for p in pairs], cap1, SIZE, dfill=-3.0)
    return pb0, pb1


class Host:
    """a MatchResult of the pruning op on the host, cut per pair"""

    def __init__(self, r, counts):
        self.B = len(counts)
        self.counts = counts
        self.a = {k: _np(getattr(r, k)) for k in ("matches0", "matches1", "scores0", "scores1", "ref0", "ref1", "prune0", "prune1", "kept0", "kept1",
                                                  "live")}
        self.stop = None if r.stop is None else _np(r.stop).tolist()
        assert r.la is None

    def pair(self, b):
        n, m = self.counts[b]
        a = self.a
        l0, l1 = int(a["live"][b]), int(a["live"][self.B + b])
        return dict(m0=a["matches0"][b, :n], m1=a["matches1"][b, :m], s0=a["scores0"][b, :n], s1=a["scores1"][b, :m], ref0=a["ref0"][b],
                    ref1=a["ref1"][b], prune0=a["prune0"][b], prune1=a["prune1"][b], kept0=a["kept0"][b], kept1=a["kept1"][b], live=(l0, l1))

    def bits(self, b):
        p = self.pair(b)
        return b"".join(np.ascontiguousarray(p[k]).tobytes() for k in ("m0", "m1", "s0", "s1", "ref0", "ref1", "prune0", "prune1", "kept0", "kept1")) \
            + repr(p["live"]).encode()


class World:
    """one run of each batch with pruning on, and the restatement of every pair, shared by the tests"""

    def __init__(self, es):
        self.es = es
        self.sd = _state_dict(ES_MSHIFTS, ES_TSHIFTS) if es else _state_dict()
        self.depth = DEPTH if es else -1
        self.lg = _model(self.sd, depth=self.depth)
        self.links = {}
        self.cases = {}
        for name, spec in CASES.items():
            pairs = [_pair(*s) for s in spec]
            counts = [(n, m) for _, n, m in spec]
            pb0, pb1 = _batches(pairs)
            n0, m0 = pb0.counts.clone(), pb1.counts.clone()
            r = self.lg.match_batched(pb0, pb1)
            torch.cuda.synchronize()
            assert torch.equal(pb0.counts, n0) and torch.equal(pb1.counts, m0)  # the caller's counts are never written
            ref = [P.run(self.sd, *p[:4], WIDTH, 0, self.depth) for p in pairs]
            self.cases[name] = dict(counts=counts, pairs=pairs, r=r, host=Host(r, counts), ref=ref, pb=(pb0, pb1))

    def link(self, layer, head):
        """the one-layer model: transformer `layer` as the only one, log_assignment[head] as its head, identity input projection"""
        if (layer, head) not in self.links:
            self.links[(layer, head)] = T._model(dict(T.SHIPPED, n_layers=1), _segment_state_dict(self.sd, [layer], head))
        return self.links[(layer, head)]


def _segment_state_dict(sd, layers, head):
    """the model that runs `layers` (renumbered from 0) and ends in log_assignment[head]"""
    out = {"posenc.Wr.weight": sd["posenc.Wr.weight"]}
    for j, i in enumerate(layers):
        for k, v in sd.items():
            if k.startswith(f"transformers.{i}."):
                out[f"transformers.{j}." + k[len(f"transformers.{i}."):]] = v
    for k, v in sd.items():
        if k.startswith(f"log_assignment.{head}."):
            out[f"log_assignment.{len(layers) - 1}." + k[len(f"log_assignment.{head}."):]] = v
    for j in range(len(layers) - 1):  # (any heads for the inner layers: they are not read)
        for k, v in sd.items():
            if k.startswith(f"log_assignment.{head}."):
                out[f"log_assignment.{j}." + k[len(f"log_assignment.{head}."):]] = v
            if k.startswith("token_confidence.0."):
                out[f"token_confidence.{j}." + k[len("token_confidence.0."):]] = v
    return out


@pytest.fixture(scope="module")
def world():
    return World(False)


@pytest.fixture(scope="module")
def world_es():
    return World(True)


def _layers_run(ref):
    """how many layers the restatement ran on the pair, and the kept sets after each of them"""
    steps = {s["layer"]: s["kept"] for s in ref["steps"]}
    if ref["stop"] is not None and ref["stop"] > 0:
        last = ref["stop"]
    elif ref["head"] is None:  # finished by an empty side, no early stopping
        last = max(steps) + 1
    else:
        last = L
    return last, steps


def _assert_state(tag, got, ref, n, m):
    """kept, prune and live against the restatement"""
    assert ref["safe"], (tag, [(s["layer"], s["near_w"], s["near_t"]) for s in ref["steps"]], ref["safe_stop"])
    assert got["live"] == ref["live"], (tag, got["live"], ref["live"])
    for s, cnt in ((0, n), (1, m)):
        kept, prune, lv = got[f"kept{s}"], got[f"prune{s}"], got["live"][s]
        assert kept.dtype == np.int64 and prune.dtype == np.float32
        assert np.array_equal(kept[:lv], ref[f"kept{s}"]) and (kept[lv:] == -1).all(), (tag, s)
        assert np.array_equal(prune[:cnt], ref[f"prune{s}"]) and not prune[cnt:].any(), (tag, s)
        assert not got[f"ref{s}"][lv:].any(), (tag, s, "rows past the live count are zero")


# ------------------------------------------------------------------------------------------------ 1. the switch off / nothing pruned
@pytest.mark.parametrize("name", ["stacked", "unstacked"])
def test_switch_off_and_keep_everything_are_the_existing_op(world, name):
    """point_pruning False (whatever width_confidence says), and True with width_confidence -1: einx_lightglue, bit for bit; the new
    op with width_confidence 1 (keep sigmoid > 0: every row) gives einx_lightglue's bits with prune == n_layers, ind the identity"""
    c = world.cases[name]
    pb0, pb1 = c["pb"]
    base = _model(world.sd, pruning=False, width=-1).match_batched(pb0, pb1)
    off = _model(world.sd, pruning=False).match_batched(pb0, pb1)
    minus = _model(world.sd, pruning=True, width=-1).match_batched(pb0, pb1)
    for r in (base, off, minus):
        assert r.live is None and r.kept0 is None and r.prune0 is None and r.la is not None
    every = _model(world.sd, pruning=True, width=1.0).match_batched(pb0, pb1)
    assert every.la is None and every.stop is None
    h = Host(every, c["counts"])
    for b, (n, m) in enumerate(c["counts"]):
        for r in (off, minus):
            for k in ("matches0", "matches1", "scores0", "scores1", "ref0", "ref1"):
                cnt = n if k.endswith("0") else m
                assert _np(getattr(r, k))[b, :cnt].tobytes() == _np(getattr(base, k))[b, :cnt].tobytes(), (name, b, k)
            assert _np(r.la)[b, :n + 1, :m + 1].tobytes() == _np(base.la)[b, :n + 1, :m + 1].tobytes() or not (n and m)
        g = h.pair(b)
        for k, bk in (("m0", "matches0"), ("m1", "matches1"), ("s0", "scores0"), ("s1", "scores1")):
            cnt = n if k.endswith("0") else m
            assert g[k].tobytes() == _np(getattr(base, bk))[b, :cnt].tobytes(), (name, b, k)
        assert g["ref0"][:n].tobytes() == _np(base.ref0)[b, :n].tobytes() and g["ref1"][:m].tobytes() == _np(base.ref1)[b, :m].tobytes()
        assert g["live"] == (n, m)
        full = float(L) if n and m else 1.0  # an empty pair takes no step
        assert (g["prune0"][:n] == full).all() and (g["prune1"][:m] == full).all(), (name, b)
        assert np.array_equal(g["kept0"][:n], np.arange(n)) and np.array_equal(g["kept1"][:m], np.arange(m))


# ------------------------------------------------------------------------------------------------ 2. the default gate
def test_default_gate_leaves_the_shipped_size_untouched(world):
    """pruning_keypoint_thresholds at its default (cuda: 1024): a side of 1024 rows does not pass `rows > 1024`, so the op equals
    einx_lightglue and prune stays 1 everywhere (upstream increments inside the `if`)"""
    lg = _model(world.sd, min_kpts=None)
    assert lg.pruning_keypoint_thresholds == {"cpu": -1, "mps": -1, "cuda": 1024, "flash": 1536} and lg.pruning_min_kpts(DEV) == 1024
    pair = _pair(11, 1024, 1024)
    pb0, pb1 = _batches([pair])
    r = lg.match_batched(pb0, pb1)
    base = _model(world.sd, pruning=False).match_batched(pb0, pb1)
    assert r.live is not None and _np(r.live).tolist() == [1024, 1024]
    for k in ("matches0", "matches1", "scores0", "scores1", "ref0", "ref1"):
        assert torch.equal(getattr(r, k), getattr(base, k)), k
    assert bool((r.prune0 == 1).all()) and bool((r.prune1 == 1).all())
    assert torch.equal(r.kept0[0], torch.arange(1024, device=DEV)) and torch.equal(r.kept1[0], torch.arange(1024, device=DEV))


# ------------------------------------------------------------------------------------------------ 3. state against the restatement
def test_the_fixed_pairs_cover_the_crossings(world):
    """what the shapes were chosen for, asserted on the restatement: both sides lose rows (not all) at a first layer and more at a
    later one; counts cross 128, 64 and 32; one side ends with exactly one row; one pair is finished by an empty side"""
    before_after = []
    for name, c in world.cases.items():
        for (n, m), ref in zip(c["counts"], c["ref"]):
            assert ref["safe"], (name, n, m)
            if not (n and m):
                assert ref["steps"] == [] and ref["live"] == (n, m)
                continue
            sizes = [(n, m)] + [(len(s["kept"][0]), len(s["kept"][1])) for s in ref["steps"]]
            before_after += [(a[s], b[s]) for a, b in zip(sizes, sizes[1:]) for s in (0, 1)]
            if n >= 31:
                changes = [i for i, (a, b) in enumerate(zip(sizes, sizes[1:])) if a != b]
                assert len(changes) == 2 and all(0 < b[s] < a[s] for i in changes for a, b in [(sizes[i], sizes[i + 1])] for s in (0, 1)), sizes
    for edge in (128, 64, 32):
        assert any(a >= edge > b > 0 for a, b in before_after), edge
    assert any(b == 1 and a > 1 for a, b in before_after)
    assert any(b == 0 for a, b in before_after)


@pytest.mark.parametrize("name", list(CASES))
def test_kept_prune_and_live_equal_the_restatement(world, name):
    c = world.cases[name]
    print(name, "live", [c["host"].pair(b)["live"] for b in range(len(c["counts"]))])
    for b, (n, m) in enumerate(c["counts"]):
        _assert_state((name, b), c["host"].pair(b), c["ref"][b], n, m)
    assert c["host"].stop is None


# ------------------------------------------------------------------------------------------------ 4. the chain of the existing op
def _chain(world, pair, ref):
    """The EXISTING op on the pair alone, one layer at a time: link i is the one-layer model of layer i, fed the keypoints still
    kept and the previous link's ref_descriptors; the rows the restatement keeps after layer i go on.  The last link carries the
    head the pair ended at.  Returns the last link's x0, x1 and its matches / scores (in survivor indexing), or None for those
    when an empty side finished the pair."""
    k0, d0, k1, d1 = pair[:4]
    last, steps = _layers_run(ref)
    ind = [np.arange(len(k0)), np.arange(len(k1))]
    x = [d0, d1]
    for i in range(last):
        final = i == last - 1 and ref["head"] is not None
        lg = world.link(i, ref["head"] if final else i)
        r = lg.match_batched(T._batch([k0[ind[0]]], [x[0]], len(ind[0]), SIZE), T._batch([k1[ind[1]]], [x[1]], len(ind[1]), SIZE, dfill=-3.0))
        assert r.live is None and r.stop is None
        x = [_np(r.ref0)[0], _np(r.ref1)[0]]
        if final:
            return x, ind, dict(m0=_np(r.matches0)[0], m1=_np(r.matches1)[0], s0=_np(r.scores0)[0], s1=_np(r.scores1)[0])
        if i in steps:
            for s in (0, 1):
                pos = np.searchsorted(ind[s], steps[i][s])
                assert np.array_equal(ind[s][pos], steps[i][s])
                x[s], ind[s] = x[s][pos], steps[i][s]
    return x, ind, None


def _assert_chain(tag, world, pair, ref, got):
    n, m = len(pair[0]), len(pair[2])
    if not (n and m):
        assert (got["m0"] == -1).all() and (got["m1"] == -1).all() and not got["s0"].any() and not got["s1"].any()
        return
    x, ind, res = _chain(world, pair, ref)
    for s in (0, 1):
        assert got[f"ref{s}"][:len(ind[s])].tobytes() == np.ascontiguousarray(x[s]).tobytes(), (tag, "ref", s)
    if res is None:
        assert (got["m0"] == -1).all() and (got["m1"] == -1).all() and not got["s0"].any() and not got["s1"].any(), tag
        return
    e0, es0 = P.scatter_back(res["m0"], res["s0"], ind[0], ind[1], n)
    e1, es1 = P.scatter_back(res["m1"], res["s1"], ind[1], ind[0], m)
    assert np.array_equal(got["m0"], e0) and np.array_equal(got["m1"], e1), tag
    assert got["s0"].tobytes() == es0.astype(np.float32).tobytes() and got["s1"].tobytes() == es1.astype(np.float32).tobytes(), tag
    assert (e0 >= 0).any(), (tag, "the pair keeps matches")


@pytest.mark.parametrize("name", list(CASES))
def test_each_pair_equals_the_chain_of_the_existing_op(world, name):
    """BIT FOR BIT, no tolerance: compaction changes no arithmetic"""
    c = world.cases[name]
    for b, pair in enumerate(c["pairs"]):
        _assert_chain((name, b), world, pair, c["ref"][b], c["host"].pair(b))


# ------------------------------------------------------------------------------------------------ 5. against float64
def _oracle_chain(oracle, sd, pair, ref):
    """the oracle as a float32 peer on the survivor sets: one run per stretch of layers between two steps that dropped rows"""
    k0, d0, k1, d1 = pair[:4]
    last, steps = _layers_run(ref)
    ind = [np.arange(len(k0)), np.arange(len(k1))]
    x = [d0, d1]
    start = 0
    for i in range(last):
        drops = i in steps and (len(steps[i][0]) < len(ind[0]) or len(steps[i][1]) < len(ind[1]))
        if not (drops or i == last - 1):
            continue
        layers = list(range(start, i + 1))
        seg = _segment_state_dict(sd, layers, ref["head"] if i == last - 1 else i)
        o = oracle.lightglue(seg, k0[ind[0]], x[0], k1[ind[1]], x[1], n_layers=len(layers), heads=4, capture_layers=(len(layers) - 1,))
        x = list(o["layers"][len(layers) - 1])
        if i == last - 1:
            return o, x
        for s in (0, 1):
            pos = np.searchsorted(ind[s], steps[i][s])
            x[s], ind[s] = x[s][pos], steps[i][s]
        start = i + 1


def _check_survivors(tag, sd, pair, ref, got, oracle, depth):
    """test_lightglue_f64_gpu._check_pair's rules on the survivor sets, without the log_assignment the op does not produce: the
    descriptors the head read within la_bound_f64 of the float64 restatement (peers: the restatement in float32, the oracle run
    on the same survivor sets), assignments equal to the float64 decisions outside the rows / columns whose float64 margin is
    inside the log_assignment bound of the same peers, scores to FTOL; pruned points hold -1 / 0 exactly."""
    n, m = len(pair[0]), len(pair[2])
    f32 = P.run(sd, *pair[:4], WIDTH, 0, depth, dtype=torch.float32)
    assert np.array_equal(f32["kept0"], ref["kept0"]) and np.array_equal(f32["kept1"], ref["kept1"]) and f32["stop"] == ref["stop"]
    orc, ox = _oracle_chain(oracle, sd, pair, ref)
    la = ref["log_assignment"]
    bound = la_bound_f64([np.abs(f32["log_assignment"] - la).max(), np.abs(orc["log_assignment"] - la).max()], np.abs(la).max())
    close_and_record(f"{tag}.log_assignment float32 vs float64", f32["log_assignment"], la, atol=bound)
    close_and_record(f"{tag}.log_assignment oracle vs float64", orc["log_assignment"], la, atol=bound)
    ind = [ref["kept0"], ref["kept1"]]
    for s in (0, 1):
        xe = ref[f"x{s}"]
        xb = la_bound_f64([np.abs(f32[f"x{s}"] - xe).max(), np.abs(ox[s] - xe).max()], np.abs(xe).max())
        close_and_record(f"{tag}.descriptors{s} gpu vs float64", got[f"ref{s}"][:len(ind[s])], xe, atol=xb)
    sc = la[:-1, :-1]
    max0 = sc.max(1)
    row_ok = (lg_f64.top2_gaps(sc, 1) < bound) | (np.abs(max0 - lg_f64.filter_edge(0.0)) < bound)
    col_ok = lg_f64.top2_gaps(sc, 0) < bound
    # the op's results in survivor indexing
    inv1, inv0 = np.full(m, -1), np.full(n, -1)
    inv0[ind[0]], inv1[ind[1]] = np.arange(len(ind[0])), np.arange(len(ind[1]))
    m0 = np.where(got["m0"][ind[0]] >= 0, inv1[np.clip(got["m0"][ind[0]], 0, None)], -1)
    m1 = np.where(got["m1"][ind[1]] >= 0, inv0[np.clip(got["m1"][ind[1]], 0, None)], -1)
    assert ((got["m0"][ind[0]] >= 0) == (m0 >= 0)).all() and ((got["m1"][ind[1]] >= 0) == (m1 >= 0)).all(), (tag, "a match with a pruned point")
    ex = lg_f64.filter_matches(torch.from_numpy(la), 0.0)
    e0, e1, es0, es1 = ex[:4]
    for i in np.nonzero(m0 != e0)[0]:
        assert row_ok[i] or any(col_ok[j] for j in (m0[i], e0[i]) if j >= 0), (tag, "row", int(i), int(m0[i]), int(e0[i]))
    for j in np.nonzero(m1 != e1)[0]:
        assert col_ok[j] or any(row_ok[i] for i in (m1[j], e1[j]) if i >= 0), (tag, "column", int(j), int(m1[j]), int(e1[j]))
    record_flips(f"{tag}.matches0 gpu vs float64", m0, e0, la)
    record_flips(f"{tag}.matches1 gpu vs float64", m1, e1, la.T)
    same0, same1 = m0 == e0, m1 == e1
    close_and_record(f"{tag}.matching_scores0 gpu vs float64", got["s0"][ind[0]][same0], es0[same0], atol=FTOL)
    close_and_record(f"{tag}.matching_scores1 gpu vs float64", got["s1"][ind[1]][same1], es1[same1], atol=FTOL)
    gone0, gone1 = np.setdiff1d(np.arange(n), ind[0]), np.setdiff1d(np.arange(m), ind[1])
    assert (got["m0"][gone0] == -1).all() and not got["s0"][gone0].any() and (got["m1"][gone1] == -1).all() and not got["s1"][gone1].any()


@pytest.mark.parametrize("name", list(CASES))
def test_each_pair_against_float64(world, oracle, name):
    c = world.cases[name]
    for b, pair in enumerate(c["pairs"]):
        if c["ref"][b]["head"] is None:  # no assignment: an empty pair, or a pair finished by an empty side (tests 3 and 4)
            continue
        _check_survivors(f"lg_prune.{name}.{b}", world.sd, pair, c["ref"][b], c["host"].pair(b), oracle, -1)


# ------------------------------------------------------------------------------------------------ 6. with early stopping
@pytest.mark.parametrize("name", list(CASES))
def test_early_stopping_and_pruning_together(world, world_es, oracle, name):
    """the stop decision first, then the step: a pair that stops after layer 5 keeps the rows it had (the moved matchability bias
    of that layer would have dropped more than half of them); the token term keeps low-confidence rows (after layer 1 more rows
    survive than without early stopping); stop, kept, prune and live are the restatement's, the outputs the chain's and
    float64's"""
    c, plain = world_es.cases[name], world.cases[name]
    stops = [r["stop"] for r in c["ref"]]
    print(name, "stop", c["host"].stop, "live", [c["host"].pair(b)["live"] for b in range(len(stops))])
    for b, (n, m) in enumerate(c["counts"]):
        ref, got = c["ref"][b], c["host"].pair(b)
        _assert_state((name, b), got, ref, n, m)
        if not (n and m):
            continue
        after1 = [s["kept"] for s in ref["steps"] if s["layer"] == 1][0]
        after1_plain = [s["kept"] for s in plain["ref"][b]["steps"] if s["layer"] == 1][0]
        assert all(set(q) <= set(p) for p, q in zip(after1, after1_plain))  # the token term only ever keeps more
        if ref["stop"] == 6:  # stopped after layer 5: not pruned there
            assert got["live"] == (len(after1[0]), len(after1[1])) and max(s["layer"] for s in ref["steps"]) == 4
            assert (got["prune0"][after1[0]] == 6).all() and (got["prune1"][after1[1]] == 6).all()
        _assert_chain((name, b, "es"), world_es, c["pairs"][b], ref, got)
        assert ref["head"] is not None
        _check_survivors(f"lg_prune_es.{name}.{b}", world_es.sd, c["pairs"][b], ref, got, oracle, DEPTH)
    assert c["host"].stop == stops
    if name == "stacked":
        assert stops == [9, 6, 6, 6, 0]
        ref = c["ref"][0]  # (31, 33) ran on and lost rows at layer 5
        sizes = {s["layer"]: (len(s["kept"][0]), len(s["kept"][1])) for s in ref["steps"]}
        assert sizes[5][0] < sizes[4][0] and sizes[5][1] < sizes[4][1] and sum(sizes[1]) > sum(len(k) for k in [s["kept"] for s in plain["ref"][0]["steps"] if s["layer"] == 1][0])


def test_an_empty_side_finishes_the_pair_with_its_stop(world_es):
    """early stopping on, token bias 5 moved by +2 only: the (1, 1) pair does not stop after layer 5 (r = 0.5), and the step
    there drops the row of side 1: the pair is finished, stop = 6, no matches"""
    sd = _state_dict(ES_MSHIFTS, {5: 2.0})
    pair = _pair(11, 1, 1)
    ref = P.run(sd, *pair[:4], WIDTH, 0, DEPTH)
    assert ref["safe"] and ref["stop"] == 6 and ref["live"] == (1, 0) and ref["head"] is None
    pb0, pb1 = _batches([pair])
    r = _model(sd, depth=DEPTH).match_batched(pb0, pb1)
    got = Host(r, [(1, 1)])
    _assert_state("finished", got.pair(0), ref, 1, 1)
    assert got.stop == [6] and _np(r.matches0).tolist() == [[-1]] and _np(r.matches1).tolist() == [[-1]]
    assert _np(r.scores0).tolist() == [[0.0]] and _np(r.scores1).tolist() == [[0.0]]


# ------------------------------------------------------------------------------------------------ 7. repeatability and memory
@pytest.mark.parametrize("name,es", [("stacked", False), ("unstacked", True)])
def test_repeatable_capturable_and_inside_its_workspace(world, world_es, monkeypatch, name, es):
    GUARD, PATTERN = 4096, 0xA5
    made = []

    def guarded(nbytes, device):
        buf = torch.empty(int(nbytes) + GUARD, dtype=torch.uint8, device=device)
        buf[int(nbytes):] = PATTERN
        made.append(buf[int(nbytes):])
        return buf[:int(nbytes)]

    w_ = world_es if es else world
    c = w_.cases[name]
    pb0, pb1 = c["pb"]
    n0, m0 = pb0.counts.clone(), pb1.counts.clone()
    w, _, _, heads = w_.lg._pack()
    call = lambda: N.lightglue(w, pb0, pb1, want_la=True, want_ref=True, early_stop=(heads, DEPTH) if es else None,  # noqa: E731
                               pruning=(heads, WIDTH, 0))
    monkeypatch.setattr(N, "_workspace", guarded)
    a, b = call(), call()
    torch.cuda.synchronize()
    assert len(made) == 2 and all(bool((g == PATTERN).all()) for g in made)
    monkeypatch.undo()
    assert int(N.lib().einx_lightglue_adaptive_ws_bytes(pb0.B, pb0.cap, pb1.cap, 256, 4, 256, 9)) > \
        int(N.lib().einx_lightglue_early_stop_ws_bytes(pb0.B, pb0.cap, pb1.cap, 256, 4, 256, 9))
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
    ha, hb, hg = Host(a, c["counts"]), Host(b, c["counts"]), Host(g, c["counts"])
    assert ha.stop == hb.stop == hg.stop == c["host"].stop
    for k in range(len(c["counts"])):
        assert ha.bits(k) == hb.bits(k) == hg.bits(k) == c["host"].bits(k), (name, k)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_native_refusals(world):
    pb0, pb1 = world.cases["stacked"]["pb"]
    w, _, _, heads = world.lg._pack()
    lib = N.lib()
    assert lib.einx_lightglue_adaptive_ws_bytes(2, 64, 64, 256, 4, 256, 33) == 0
    with pytest.raises(ValueError, match="every layer"):
        N.lightglue(w, pb0, pb1, all_layers=True, want_ref=True, pruning=(heads, WIDTH, 0))
    with pytest.raises(ValueError, match="width_confidence"):
        N.lightglue(w, pb0, pb1, want_ref=True, pruning=(heads, 0.0, 0))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    p = ws.data_ptr()

    def rc(heads_, head_size, depth, width, la=None, live=p):
        return lib.einx_lightglue_adaptive(ctypes.byref(w), heads_, head_size, depth, width, 0, *([None] * 3), 64, *([None] * 3), 64, 2, 1.0, 1.0, 1.0,
                                           1.0, p, *([None] * 4), la, None, None, None, p, p, p, p, live, None)

    hs = ctypes.sizeof(type(heads[0]))
    assert rc(heads, hs + 8, -1.0, 0.5) != 0 and b"head_size" in lib.einx_last_error()
    assert rc(heads, hs, -1.0, 0.0) != 0 and b"width_confidence" in lib.einx_last_error()
    assert rc(heads, hs, -1.0, 1.5) != 0 and b"width_confidence" in lib.einx_last_error()
    assert rc(heads, hs, -1.0, 0.5, la=p) != 0 and b"log_assignment" in lib.einx_last_error()
    assert rc(heads, hs, -1.0, 0.5, live=None) != 0 and b"null pointer" in lib.einx_last_error()
    bad = (type(heads[0]) * 9)()
    assert rc(bad, hs, -1.0, 0.5) != 0 and b"log_assignment head" in lib.einx_last_error()
    no_token = (type(heads[0]) * 9)()
    for i in range(9):
        for f in ("proj_w", "proj_b", "match_w", "match_b"):
            setattr(no_token[i], f, getattr(heads[i], f))
    assert rc(no_token, hs, 0.5, 0.5) != 0 and b"token_confidence" in lib.einx_last_error()


# ------------------------------------------------------------------------------------------------ 9. end to end
def test_front_door_single_pair_and_stacked_forward(world):
    """LightGlue.forward: B = 1 slices kept0/1 to the live counts; stacked [B,n,*] tensors give [B,cap] padded with -1; neither
    carries log_assignment, and the loss refuses both"""
    pair = world.cases["single"]["pairs"][0]
    ref = world.cases["single"]["ref"][0]
    out = world.lg(T._feats(pair[0], pair[1], SIZE), T._feats(pair[2], pair[3], SIZE))
    assert "log_assignment" not in out and "stop" not in out
    assert out["kept0"].dtype == torch.int64 and _np(out["kept0"]).tolist() == [ref["kept0"].tolist()] and _np(out["kept1"]).tolist() == [ref["kept1"].tolist()]
    assert np.array_equal(_np(out["prune0"])[0], ref["prune0"]) and out["prune0"].dtype == torch.float32
    assert np.array_equal(_np(out["matches0"])[0], world.cases["single"]["host"].pair(0)["m0"])
    assert out["ref_descriptors0"].shape == (1, 1, 5, 256) and not _np(out["ref_descriptors0"])[0, 0, ref["live"][0]:].any()
    with pytest.raises(ValueError, match="kept0"):
        world.lg.loss(out, {})
    pairs = [_pair(11 + 17 * b, 64, 64) for b in range(2)]
    feats = [{"sparse_descriptors": _t(np.stack([p[1 + 2 * s] for p in pairs])), "sparse_positions": _t(np.stack([p[2 * s] for p in pairs])),
              "image_size": [torch.tensor(SIZE)] * 2} for s in (0, 1)]
    out = world.lg(*feats)
    refs = [P.run(world.sd, *p[:4], WIDTH, 0, -1) for p in pairs]
    assert all(r["safe"] for r in refs) and "log_assignment" not in out
    for b, r in enumerate(refs):
        k0 = _np(out["kept0"])[b]
        assert k0.shape == (64,) and np.array_equal(k0[:r["live"][0]], r["kept0"]) and (k0[r["live"][0]:] == -1).all()
        assert np.array_equal(_np(out["prune1"])[b], r["prune1"])


def test_matcher_eim_and_evaluator_carry_the_keys():
    """Matcher's frozen path, EIM.forward / forward_graph and DifferentTimeEvaluator on an SP + LightGlue model (3 layers).  The
    matchability bias of layer 0 is set from the model's own logits on the batch (their median lands on the threshold), so about
    half of every side leaves after the first layer whatever the synthetic weights are"""
    Hh, Wd, B, bins = 260, 346, 3, 5
    cfg = pkg.default_config("SP_LG", event_channels=bins)
    cfg.matcher.LightGlue.n_layers = 3
    cfg.matcher.LightGlue.width_confidence = 0.5
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=33)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    lg = model.matcher.matcher
    lg.pruning_keypoint_thresholds["cuda"] = 0
    plain = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh))
    evs = [synth_raw_events(dict(seed=800 + b, n=20000 if b else 4000, H=Hh, W=Wd, bins=bins, frac=False, pneg=False)) for b in range(B)]
    img = synth.synth_image(95, B, Hh, Wd)
    _, (ef, imf, m_off) = plain.step(evs, _t(img.copy()))
    assert "kept0" not in m_off and "live" not in m_off and "matcher_kept_ratio" not in plain.result()
    from importlib import import_module
    from_feats = import_module(pkg.__name__ + ".core.modules.matchers._batched").from_feats
    pb0, pb1 = from_feats(ef), from_feats(imf)
    layers = lg.match_batched(pb0, pb1, all_layers=True)
    head = lg.log_assignment[0].matchability
    z = torch.cat([(layers.ref0[b, 0, :int(pb0.counts[b])] @ head.weight[0]) for b in range(B)]
                  + [(layers.ref1[b, 0, :int(pb1.counts[b])] @ head.weight[0]) for b in range(B)])
    with torch.no_grad():
        head.bias.fill_(-float(z.median()))  # width_confidence 0.5: keep logit > 0
        for i in (1,):
            lg.log_assignment[i].matchability.bias.fill_(100.0)  # the second step keeps what it gets
    lg.point_pruning = True
    with pytest.raises(ValueError, match="point pruning"):
        pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh), matcher_loss=True).step(evs, _t(img.copy()))
    m = model.matcher(ef, imf)  # the frozen path on the feature dicts
    n, mm = pb0.counts.tolist(), pb1.counts.tolist()
    live = [[int(v) for v in lv] for lv in m["live"]]
    print("counts", n, mm, "live", live)
    assert len(m["kept0"]) == B and all(0 < live[b][0] < n[b] and 0 < live[b][1] < mm[b] for b in range(B))
    for b in range(B):
        k0 = m["kept0"][b]
        assert k0.dtype == torch.int64 and bool((k0[:live[b][0]] >= 0).all()) and bool((k0[live[b][0]:] == -1).all())
        assert bool((k0[1:live[b][0]] > k0[:live[b][0] - 1]).all())  # the survivors keep their order
        p0 = m["prune0"][b][:n[b]]
        assert int((p0 == 3).sum()) == live[b][0] and int((p0 == 1).sum()) == n[b] - live[b][0]
        gone = torch.ones(n[b], dtype=torch.bool, device=DEV)
        gone[k0[:live[b][0]]] = False
        assert bool((m["matches0"][b][0][gone] == -1).all()) and not bool(m["matching_scores0"][b][0][gone].any())
    rep, mask = plain.last_inputs
    _, _, m1 = model(rep, _t(img.copy()), mask)
    _, _, m2 = model.forward_graph(rep, _t(img.copy()), mask)
    for k in ("kept0", "kept1", "prune0", "prune1", "live", "matches0", "matches1"):
        assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(m[k], m1[k], m2[k])), k
    before = len(model._graphs)
    lg.conf["width_confidence"] = 0.75  # baked into a capture: a new graph
    model.forward_graph(rep, _t(img.copy()), mask)
    lg.pruning_keypoint_thresholds["cuda"] = 4096  # so is the gate
    _, _, m4 = model.forward_graph(rep, _t(img.copy()), mask)
    assert [[int(v) for v in lv] for lv in m4["live"]] == [[n[b], mm[b]] for b in range(B)]
    lg.point_pruning = False
    _, _, m3 = model.forward_graph(rep, _t(img.copy()), mask)
    assert len(model._graphs) == before + 3 and "kept0" not in m3 and "live" not in m3
    lg.point_pruning, lg.conf["width_confidence"] = True, 0.5
    lg.pruning_keypoint_thresholds["cuda"] = 0
    stepped = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh))
    _, (_, _, ms) = stepped.step(evs, _t(img.copy()))
    ratio = [(int(lv[0]) + int(lv[1])) / (n[b] + mm[b]) for b, lv in enumerate(ms["live"])]
    assert stepped.result()["matcher_kept_ratio"] == pytest.approx(sum(ratio) / B, abs=1e-12)
