"""GPU tests (-m gpu), component: LightGlue `flash: True`, attention in fp16 on the matrix cores (lg_attn_f16_kernel,
einx_lightglue_flash).  The judge is the contract's float64 restatement (tests/lg_flash_ref.py "spec"); the bound of
every float comparison is the project's rule, helpers.la_bound_f64: twice the worse of the two independent float peers (peer_a:
torch's scaled_dot_product_attention on half tensors; peer_b: fp16 probabilities, fp32 accumulation) against the spec on the same
inputs.  The kernel alone is first tested on inputs whose answer is exact: there the comparison is bit for bit."""
import numpy as np
import pytest
import torch

import lg_early_stop_ref as ES
import lg_f64
import lg_flash_ref as FR
import lg_prune_ref as P
from helpers import close_and_record, la_bound_f64, lgf64_pair, lgf64_shipped_state_dict, record_flips, synth, synth_raw_events
from gpu_support import DEV, FTOL, _np, _t, pkg

pytestmark = pytest.mark.gpu
N = pkg.native
PairBatch = __import__("importlib").import_module(pkg.__name__ + ".core.modules.matchers._batched").PairBatch
SIZE = (260, 346)
GUARD = 1024  # floats behind O


# ------------------------------------------------------------------------------------------------ the kernel hook
def _hook(Q, K, V, nq, nk, heads, dh, ld, kv_shift=0):
    """Q [B, capq, d], K / V [B, capk, d] float32 numpy -> O [B, capq, d] (NaN where the kernel did not write).  The operands are laid
    out at row stride ld with 1e30 in the columns past d (never read); O is followed by guard floats that must stay untouched."""
    B, capq, d = Q.shape
    capk = K.shape[1]
    assert d == heads * dh and ld >= d

    def wide(a):
        w = np.full(a.shape[:2] + (ld,), 1e30, np.float32)
        w[..., :d] = a
        return _t(w)

    buf = torch.full((B * capq * d + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    buf[B * capq * d:] = -77.0
    q, k, v = wide(Q), wide(K), wide(V)
    cq, ck = _t(np.asarray(nq, np.int32)), _t(np.asarray(nk, np.int32))
    rc = N.lib().einx_lg_attention_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), buf.data_ptr(), cq.data_ptr(), ck.data_ptr(), capq, capk, B,
                                       heads, dh, ld, kv_shift, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, N.lib().einx_last_error()
    torch.cuda.synchronize()
    out = _np(buf)
    assert (out[B * capq * d:] == -77.0).all(), "guard behind O overwritten"
    return out[:B * capq * d].reshape(B, capq, d)


def _rn16(x):
    """float64 -> RN16(RN32(x)) as float32"""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float16).astype(np.float32)


def _same_bits(tag, got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad[0].size == 0, (tag, bad[0].size, [int(b[0]) for b in bad], float(got[tuple(b[0] for b in bad)]), float(want[tuple(b[0] for b in bad)]))


def _check_rows(tag, O, want, nq, nk, kv_shift):
    """rows below nq of an entry with keys: bit-equal to `want`; every other row still NaN"""
    B = O.shape[0]
    for b in range(B):
        live = min(nq[b], O.shape[1]) if nk[(b + kv_shift) % B] > 0 else 0
        _same_bits((tag, b), O[b, :live], want[b, :live])
        assert np.isnan(O[b, live:]).all(), (tag, b, "rows past nq written")


# (heads, dh): the four instantiations, the shipped one (4 x 64 at d = 256), a zero-padded width (48 -> 64)
WIDTHS = [(2, 32), (4, 64), (2, 64), (1, 128), (1, 256), (2, 48)]
NK = [1, 15, 16, 17, 31, 32, 33, 63, 65, 200]
NQ = [1, 31, 33, 127, 129]


@pytest.mark.parametrize("heads,dh", WIDTHS)
@pytest.mark.parametrize("wide", [False, True])
def test_uniform_attention_is_the_exact_mean(heads, dh, wide):
    """Q = 0: every logit is 0, every probability 2^0 = 1 (exact in fp16), V holds small integers, so the fp32 sums are exact and
    O = RN16(RN32(sum v / nk)), bit for bit (53 >= 2 x 24 + 2 bits: rounding the float64 quotient to fp32 is the correctly rounded
    fp32 division).  Entries of 3 with every key count and query count of the lists, an entry without queries and one without keys;
    self (kv_shift 0) and cross over the stacked buffer (kv_shift = B / 2, n != m)."""
    d = heads * dh
    ld = 2 * d if wide else d
    rng = np.random.default_rng(dh * 7 + heads + wide)
    for kv_shift in (0, 2):
        for i in range(0, len(NK), 3):  # 4 entries per launch: two "sides" of two pairs; entry 3 has no keys / no queries in turn
            nks = (NK + NK)[i:i + 3]
            nqs = (NQ + NQ)[i // 3:i // 3 + 3]
            nq = [nqs[0], nqs[1], 0 if i % 2 else nqs[2], 5]
            nk = [nks[0], nks[1], nks[2], 0] if kv_shift == 0 else [nks[0], 0 if i % 2 else nks[1], nks[2], 7]
            capq, capk = max(nq), max(max(nk), 1)
            Q = np.zeros((4, capq, d), np.float32)
            K = rng.standard_normal((4, capk, d)).astype(np.float32)
            V = rng.integers(-8, 9, (4, capk, d)).astype(np.float32)
            O = _hook(Q, K, V, nq, nk, heads, dh, ld, kv_shift)
            want = np.zeros((4, capq, d), np.float32)
            for b in range(4):
                m = nk[(b + kv_shift) % 4]
                if m > 0:
                    want[b] = _rn16(V[(b + kv_shift) % 4, :m].astype(np.float64).sum(0) / m)[None]
            _check_rows(("uniform", heads, dh, ld, kv_shift, i), O, want, nq, nk, kv_shift)


@pytest.mark.parametrize("heads,dh", WIDTHS)
def test_one_hot_attention_returns_the_key(heads, dh):
    """one key per (query, head) far above the rest (see _one_hot): every other probability is 0 after its fp16 rounding and adds
    less than half an ulp to the fp32 row sum, and the running sums are rescaled by exactly 0 when the key arrives, so the row is
    RN16(v) of that key, bit for bit -- a different key for every (entry, query, head), random V: a wrong lane map, key permutation
    or head offset returns another key's row"""
    d = heads * dh
    rng = np.random.default_rng(dh + heads)
    B = 3
    for nq_, nk_ in ((129, 200), (33, 65), (127, 17), (31, 33), (1, 1), (5, 63)):
        nq, nk = [nq_, max(nq_ // 2, 1), 1], [nk_, nk_, max(nk_ // 3, 1)]
        V = (rng.standard_normal((B, nk_, d)) * 3).astype(np.float32)
        hot = lambda b, q, h: (7 * q + 3 * h + b) % nk[b]  # noqa: E731
        Q, K, want = _one_hot(B, nq_, nk_, nq, nk, heads, dh, V, hot)
        O = _hook(Q, K, V, nq, nk, heads, dh, d)
        _check_rows(("one hot", heads, dh, nq_, nk_), O, want, nq, nk, 0)


def _one_hot(B, capq, capk, nq, nk, heads, dh, V, hot):
    """Key j is +-32 on dims 3 .. 10 of its head (not aligned to an 8-dim fragment) with the signs spelling j in binary (up to 256
    keys), 0 elsewhere; the query carries the sign pattern of its hot key: q . k = 1024 (agreements - disagreements) = 8192 for the hot
    key and at most 6144 for any other.  All values fp16-exact; the gap 2048 / sqrt(dh) is at least 128 base-e units (dh = 256):
    exp(-128) rounds to 0 in fp16, 199 of them add nothing to 1.0f, and 2^(-128 log2 e) underflows to 0 in fp32."""
    d = heads * dh
    bits = 8
    Q, K = np.zeros((B, capq, d), np.float32), np.zeros((B, capk, d), np.float32)
    want = np.zeros((B, capq, d), np.float32)
    sign = lambda j: np.asarray([32.0 if (j >> t) & 1 else -32.0 for t in range(bits)], np.float32)  # noqa: E731
    for b in range(B):
        for h in range(heads):
            c0 = h * dh
            for j in range(nk[b]):
                K[b, j, c0 + 3:c0 + 3 + bits] = sign(j)  # (dims 3 .. 10: not aligned to a fragment)
            for q in range(nq[b]):
                j = hot(b, q, h)
                Q[b, q, c0 + 3:c0 + 3 + bits] = sign(j)
                want[b, q, c0:c0 + dh] = V[b, j, c0:c0 + dh].astype(np.float16).astype(np.float32)
    return Q, K, want


def test_keys_equal_after_rounding_share_the_weight():
    """The discriminator between fp16 and fp32 attention: two keys whose components differ by 2^-12 relative (8 and 8 (1 + 2^-12):
    both 8 in binary16) under a query of 2048 on every dim.  In fp32 their logits differ by 64 x 2048 x 8 x 2^-12 / 8 = 32: softmax
    puts 1 - 1e-14 on the larger one and lg_attn_kernel returns its row.  Under the contract they are the same key: the context is
    the mean of the two rows, RN16((v_a + v_b) / 2), exactly (integer rows).  Every other key sits at -8: logit -131072."""
    heads, dh, d = 4, 64, 256
    rng = np.random.default_rng(5)
    nq, nk = [40, 3], [40, 70]
    Q = np.full((2, 40, d), 2048.0, np.float32)
    K = np.full((2, 70, d), -8.0, np.float32)
    V = rng.integers(-100, 101, (2, 70, d)).astype(np.float32)
    pairs = [(5, 37), (66, 2)]
    want = np.zeros((2, 40, d), np.float32)
    for b, (ka, kb) in enumerate(pairs):
        K[b, ka], K[b, kb] = 8.0, np.float32(8.0 * (1 + 2.0 ** -12))
        assert K[b, kb, 0] != K[b, ka, 0] and np.float16(K[b, kb, 0]) == np.float16(8.0)
        want[b] = _rn16((V[b, ka].astype(np.float64) + V[b, kb]) / 2)[None]
        assert np.abs(want[b] - V[b, kb]).max() > 10  # far from what fp32 attention returns
    for ld in (d, 2 * d):
        _check_rows(("equal keys", ld), _hook(Q, K, V, nq, nk, heads, dh, ld), want, nq, nk, 0)


@pytest.mark.parametrize("heads,dh,nq,nk", [(4, 64, 150, 200), (2, 128, 70, 64), (3, 48, 33, 129)])
def test_random_attention_against_the_spec(heads, dh, nq, nk):
    """random q, k, v at LightGlue's magnitudes: within twice the worse peer of the float64 spec (plus 8 fp32 ulps, la_bound_f64)"""
    d = heads * dh
    rng = np.random.default_rng(nq + nk)
    Q, K, V = ((rng.standard_normal((2, r, d)) * s).astype(np.float32) for r, s in ((nq, 1.5), (nk, 1.5), (nk, 1.0)))
    O = _hook(Q, K, V, [nq, nq - 3], [nk, nk - 5], heads, dh, d)
    for b, (n, m) in enumerate(((nq, nk), (nq - 3, nk - 5))):
        split = lambda a, r: a[b, :r].reshape(r, heads, dh).transpose(1, 0, 2)  # noqa: E731
        q, k, v = split(Q, n), split(K, m), split(V, m)
        spec = FR.attention_np(q, k, v, "spec")
        errs = [np.abs(FR.attention_np(q, k, v, mode) - spec).max() for mode in ("peer_a", "peer_b")]
        got = O[b, :n].reshape(n, heads, dh).transpose(1, 0, 2)
        assert np.array_equal(got, got.astype(np.float16).astype(np.float32))  # every element binary16-representable
        close_and_record(f"lgflash.attention.{heads}x{dh}.{n}x{m} gpu vs spec", got, spec, atol=la_bound_f64(errs, np.abs(spec).max()))
        assert np.isnan(O[b, n:]).all()


# ------------------------------------------------------------------------------------------------ the whole forward
def _cut_sd(sd, layers):
    keep = lambda k: k.split(".")[0] not in ("transformers", "log_assignment", "token_confidence") or int(k.split(".")[1]) < layers  # noqa: E731
    return {k: v for k, v in sd.items() if keep(k) and not (k.startswith("token_confidence.") and int(k.split(".")[1]) >= layers - 1)}


def _conf(layers, **kw):
    return dict(input_dim=256, descriptor_dim=256, num_heads=4, n_layers=layers, **kw)


def _model(conf, sd):
    lg = pkg.LightGlue(conf).to(DEV)
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    lg.refresh()
    return lg.eval()


def _pair(seed, n, m):
    """(k0, d0, k1, d1); an empty side is cut from a pair that has rows"""
    d0, d1, k0, k1 = lgf64_pair(seed, max(n, 1), max(m, 1))
    return k0[:n], d0[:n], k1[:m], d1[:m]


def _batch(ks, ds, cap, kfill=1e6, dfill=7.0):
    B, din = len(ks), ds[0].shape[1]
    K, D = np.full((B, cap, 3), kfill, np.float32), np.full((B, cap, din), dfill, np.float32)
    for b in range(B):
        K[b, :len(ks[b])], D[b, :len(ds[b])] = ks[b], ds[b]
    pb = PairBatch()
    pb.kpts, pb.desc, pb.counts = _t(K), _t(D), _t(np.asarray([len(k) for k in ks], np.int32))
    pb.cap, pb.B, pb.image_size, pb.counts_host = cap, B, SIZE, None
    return pb


def _batches(pairs, cap0=None, cap1=None):
    cap0 = cap0 or max(max(len(p[0]) for p in pairs), 1)
    cap1 = cap1 or max(max(len(p[2]) for p in pairs), 1)
    return _batch([p[0] for p in pairs], [p[1] for p in pairs], cap0), _batch([p[2] for p in pairs], [p[3] for p in pairs], cap1, dfill=-3.0)


def _bits(r, pairs):
    """what a call defines, per pair: the rows below the pair's counts (the outputs are torch.empty: the padding is not written)"""
    out = []
    for b, p in enumerate(pairs):
        n, m = len(p[0]), len(p[2])
        e = {"matches0": _np(r.matches0)[b, :n], "matches1": _np(r.matches1)[b, :m], "scores0": _np(r.scores0)[b, :n], "scores1": _np(r.scores1)[b, :m]}
        if r.la is not None and n and m:
            e["la"] = _np(r.la)[b, :n + 1, :m + 1]
        if r.ref0 is not None:
            e["ref0"], e["ref1"] = _np(r.ref0)[b][..., :n, :], _np(r.ref1)[b][..., :m, :]
        out.append({k: np.ascontiguousarray(v).copy() for k, v in e.items()})
    return out


def _equal_bits(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)) for k in x)
                                    for x, y in zip(a, b))


def _peer_bound(spec, peers, absmax):
    return la_bound_f64([np.abs(p - spec).max() for p in peers], absmax)


def _check_pair(tag, sd, pair, got):
    """test_lightglue_f64_gpu.py::_check_pair's rule with the flash spec as the exact answer and its two float peers: log_assignment
    and the descriptors after every layer within la_bound_f64 of the spec, assignments equal to the spec's decisions except at rows /
    columns whose spec margin is inside that bound"""
    k0, d0, k1, d1 = pair
    n, m = len(k0), len(k1)
    if n == 0 or m == 0:  # no assignment to speak of
        assert (got["m0"] == -1).all() and (got["m1"] == -1).all(), tag
        return None
    ex = FR.forward(sd, *pair)
    peers = [FR.forward(sd, *pair, mode=mode) for mode in ("peer_a", "peer_b")]
    la = ex["log_assignment"]
    assert got["la"].shape == (n + 1, m + 1) and got["la"][n, m] == 0
    bound = _peer_bound(la, [p["log_assignment"] for p in peers], np.abs(la).max())
    for name, p in zip(("peer_a", "peer_b"), peers):
        close_and_record(f"{tag}.log_assignment {name} vs spec", p["log_assignment"], la, atol=bound)
    close_and_record(f"{tag}.log_assignment gpu vs spec", got["la"], la, atol=bound)
    worst = None
    for i, xs in enumerate(ex["layers"]):
        for s, x in enumerate(xs):
            b = _peer_bound(x, [p["layers"][i][s] for p in peers], np.abs(x).max())
            err = float(np.abs(got["layers"][i][s].astype(np.float64) - x).max())
            assert err <= b, f"{tag}: layer {i} side {s}: |gpu - spec| = {err:.3e} > {b:.3e}"
            if worst is None or err / b > worst[0]:
                worst = (err / b, i, s, b)
    _, i, s, b = worst
    close_and_record(f"{tag}.descriptors (worst layer) gpu vs spec", got["layers"][i][s], ex["layers"][i][s], atol=b)
    _check_matches(tag, got, ex, bound)
    return ex


def _check_matches(tag, got, ex, bound, la=None):
    la = ex["log_assignment"] if la is None else la
    n, m = la.shape[0] - 1, la.shape[1] - 1
    s = la[:-1, :-1]
    row_gap, col_gap = lg_f64.top2_gaps(s, 1), lg_f64.top2_gaps(s, 0)
    edge = np.abs(s.max(1) - lg_f64.filter_edge(0.0))
    row_ok, col_ok = (row_gap < bound) | (edge < bound), col_gap < bound
    m0, m1, e0, e1 = got["m0"], got["m1"], ex["matches0"], ex["matches1"]
    assert (m0 < m).all() and (m1 < n).all()
    for i in np.nonzero(m0 != e0)[0]:
        assert row_ok[i] or any(col_ok[j] for j in (m0[i], e0[i]) if j >= 0), (tag, "row", int(i), int(m0[i]), int(e0[i]))
    for j in np.nonzero(m1 != e1)[0]:
        assert col_ok[j] or any(row_ok[i] for i in (m1[j], e1[j]) if i >= 0), (tag, "column", int(j), int(m1[j]), int(e1[j]))
    record_flips(f"{tag}.matches0 gpu vs spec", m0, e0, la)
    record_flips(f"{tag}.matches1 gpu vs spec", m1, e1, la.T)
    same0, same1 = m0 == e0, m1 == e1
    close_and_record(f"{tag}.matching_scores0 gpu vs spec", got["s0"][same0], ex["scores0"][same0], atol=max(FTOL, bound))
    close_and_record(f"{tag}.matching_scores1 gpu vs spec", got["s1"][same1], ex["scores1"][same1], atol=max(FTOL, bound))


def _cut(r, pairs):
    la, ref0, ref1 = _np(r.la), _np(r.ref0), _np(r.ref1)
    m0, m1, s0, s1 = _np(r.matches0), _np(r.matches1), _np(r.scores0), _np(r.scores1)
    out = []
    for b, p in enumerate(pairs):
        n, m = len(p[0]), len(p[2])
        assert (m0[b, n:] == -1).all() and (m1[b, m:] == -1).all(), (b, "padding rows matched")
        out.append({"la": la[b, :n + 1, :m + 1], "layers": [(ref0[b, i, :n], ref1[b, i, :m]) for i in range(ref0.shape[1])],
                    "m0": m0[b, :n], "m1": m1[b, :m], "s0": s0[b, :n], "s1": s1[b, :m]})
    return out


# (case, layers, [(n, m)], cap0, cap1): counts from {0, 1, 33, 129, 300}; equal caps stack the sides (cross attention through
# kv_shift, the merged to_qk | to_v buffer at row stride 512), unequal caps run one launch per side.  A count of 1 is always paired
# with a longer side: in a (1, 1) pair every softmax runs over one key and every context is RN16(v), so the two peers -- which share
# their float32 projections bit for bit and differ only inside the attention -- are the SAME computation there, and "twice the worse
# of two independent peers" has one sample that measures fp32 rounding alone (4e-6 after layer 0), while one binary16 rounding that
# falls the other way behind a kernel's differently summed projection is worth 8e-5 (measured: DESIGN.md 8k).  With a longer partner
# the cross attention gives the peers their own rounding.  One query over one key is tested bit for bit on the kernel hook above.
FORWARD = [
    ("stacked_l3", 3, [(33, 129), (300, 1), (0, 33)], 300, 300),
    ("unstacked_l3", 3, [(129, 300), (1, 33), (33, 0)], 129, 300),
    ("stacked_l9", 9, [(300, 129), (33, 33), (1, 300)], 300, 300),
]


@pytest.mark.parametrize("case", [f[0] for f in FORWARD])
def test_forward_every_pair_against_the_spec(case):
    _, layers, counts, cap0, cap1 = next(f for f in FORWARD if f[0] == case)
    sd = _cut_sd(lgf64_shipped_state_dict(811), layers)
    pairs = [_pair(8800 + 17 * b + layers, n, m) for b, (n, m) in enumerate(counts)]
    on, off, plain = _model(_conf(layers, flash=True), sd), _model(_conf(layers, flash=False), sd), _model(_conf(layers), sd)
    assert (on.attention_mode, off.attention_mode, plain.attention_mode) == ("fp16", "fp32", "fp32")
    pb0, pb1 = _batches(pairs, cap0, cap1)
    r_on, r_off, r_plain = (lg.match_batched(pb0, pb1, all_layers=True) for lg in (on, off, plain))
    torch.cuda.synchronize()
    # flash: False is the model built without the key, bit for bit; flash: True is another computation
    b_on, b_off = _bits(r_on, pairs), _bits(r_off, pairs)
    assert _equal_bits(b_off, _bits(r_plain, pairs))
    for x, y in zip(b_on, b_off):
        if "la" in x:
            assert not np.array_equal(x["la"], y["la"]) and not np.array_equal(x["ref0"], y["ref0"]) and not np.array_equal(x["ref1"], y["ref1"])
    for b, got in enumerate(_cut(r_on, pairs)):
        _check_pair(f"lgflash.{case}", sd, pairs[b], got)
    # the front door on one pair (B = 1: the same kernel, no latency twin) and LightGlue.loss on its pred
    k0, d0, k1, d1 = pairs[0]
    if len(k0) and len(k1):
        feats = lambda k, d: {"sparse_descriptors": _t(d)[None], "sparse_positions": _t(k)[None], "image_size": [torch.tensor(SIZE)]}  # noqa: E731
        pred = on(feats(k0, d0), feats(k1, d1))
        one = {"la": _np(pred["log_assignment"])[0], "m0": _np(pred["matches0"])[0], "m1": _np(pred["matches1"])[0],
               "s0": _np(pred["matching_scores0"])[0], "s1": _np(pred["matching_scores1"])[0]}
        ex = FR.forward(sd, *pairs[0])
        peers = [FR.forward(sd, *pairs[0], mode=mode)["log_assignment"] for mode in ("peer_a", "peer_b")]
        bound = _peer_bound(ex["log_assignment"], peers, np.abs(ex["log_assignment"]).max())
        close_and_record(f"lgflash.{case}.single.log_assignment gpu vs spec", one["la"], ex["log_assignment"], atol=bound)
        _check_matches(f"lgflash.{case}.single", one, ex, bound)


def test_loss_takes_a_flash_pred_unchanged():
    """LightGlue.loss (eval) reads the forward's ref_descriptors and the last head: no attention in it, so on a flash forward's pred
    it gives what the fp32 model's loss gives on the same pred, bit for bit"""
    sd = _cut_sd(lgf64_shipped_state_dict(813), 3)
    on, off = _model(_conf(3, flash=True), sd), _model(_conf(3), sd)
    k0, d0, k1, d1 = _pair(8950, 33, 33)
    feats = lambda k, d: {"sparse_descriptors": _t(d)[None], "sparse_positions": _t(k)[None], "image_size": [torch.tensor(SIZE)]}  # noqa: E731
    pred = on(feats(k0, d0), feats(k1, d1))
    m0 = pred["matches0"]
    data = {"gt_matches0": m0.clone(), "gt_matches1": pred["matches1"].clone(),
            "gt_assignment": (m0[:, :, None] == torch.arange(33, device=DEV)[None, None, :])}
    a, _ = on.loss(pred, data)
    b, _ = off.loss(pred, data)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) and bool(torch.isfinite(a["total"]).all())


# ------------------------------------------------------------------------------------------------ early stopping and pruning
# The shipped model with two biases moved (chosen on the CPU with the restatement over the flash blocks, pairs (31, 33) and (64, 64)
# of seed 11): matchability bias 1 by -5.4918 puts the pruning threshold (sigmoid > 0.01, logit > -4.595) into the widest gap of the
# layer-1 logits, 0.053 wide, where the peers' logits deviate by 5.5e-4: 22 of the 192 rows are pruned there, no other layer prunes;
# token bias 5 by +5 with depth_confidence 0.9: both pairs stop after layer 5 (r = 0.94 / 0.96), every earlier r is below 0.2.
WIDTH, DEPTH = 0.99, 0.9
MSHIFT, TSHIFT = {1: -5.4918}, {5: 5.0}
LAYERS = 9
ADAPTIVE_PAIRS = [(11, 31, 33), (11, 64, 64), (11, 0, 5)]


def _shifted_sd(mshifts, tshifts):
    sd = lgf64_shipped_state_dict(7)
    for i, s in mshifts.items():
        sd[f"log_assignment.{i}.matchability.bias"] = sd[f"log_assignment.{i}.matchability.bias"] + np.float32(s)
    for i, s in tshifts.items():
        sd[f"token_confidence.{i}.token.0.bias"] = sd[f"token_confidence.{i}.token.0.bias"] + np.float32(s)
    return sd


def _adaptive_case(mode):
    prune, stop = mode != "stop", mode != "prune"
    return prune, stop, (WIDTH if prune else -1), (DEPTH if stop else -1), _shifted_sd(MSHIFT if prune else {}, TSHIFT if stop else {})


def _logit(s):
    s = np.asarray(s, np.float64)
    return np.log(s) - np.log1p(-s)


def _safe_refs(mode, sd, pair, width, depth):
    """The restatement of point pruning / early stopping (lg_prune_ref.run / lg_early_stop_ref.run: their decision logic, untouched)
    over the flash blocks: the spec and the two peers.  Before anything is compared with the spec's decisions they are shown to be
    out of the rounding's reach, by the peers' own scatter (the la_bound_f64 idea on decisions):
      pruning: the peers took the spec's decisions, and every matchability logit the spec compared is further from the threshold
               than twice the largest deviation of a peer's logit from the spec's;
      stopping: at every layer the count of unconfident rows is further from the count at which the decision flips than twice the
               largest deviation of a peer's count from the spec's, plus one row."""
    prune, stop = mode != "stop", mode != "prune"
    refs = {}
    for m in ("spec", "peer_a", "peer_b"):
        with FR.blocks(m):
            refs[m] = P.run(sd, *pair, width, 0, depth, dtype=FR.DTYPE[m]) if prune else ES.run(sd, *pair, depth, dtype=FR.DTYPE[m])
    spec = refs["spec"]
    total = len(pair[0]) + len(pair[2])
    for m in ("peer_a", "peer_b"):
        assert refs[m]["stop"] == spec["stop"], (mode, m)
    if prune:
        thr = float(_logit(P.width_threshold(width)))
        margin, dev = np.inf, 0.0
        for m in ("peer_a", "peer_b"):
            assert len(refs[m]["steps"]) == len(spec["steps"]), (mode, m)
            for a, b in zip(spec["steps"], refs[m]["steps"]):
                assert a["layer"] == b["layer"] and all(np.array_equal(x, y) for x, y in zip(a["kept"], b["kept"])), (mode, m)
                for s in range(2):
                    if a["sig"][s] is not None:
                        margin = min(margin, float(np.abs(_logit(a["sig"][s]) - thr).min()))
                        dev = max(dev, float(np.abs(_logit(a["sig"][s]) - _logit(b["sig"][s])).max()))
        assert margin > 2 * dev, (mode, "pruning margin", margin, dev)
    if stop:
        flip = (1.0 - depth) * total  # the stop decision: 1 - below / total > depth
        dev = max(abs(a - b) for m in ("peer_a", "peer_b") for a, b in zip(spec["below"], refs[m]["below"]))
        margin = min(abs(b - flip) for b in spec["below"])
        assert margin > 2 * dev + 1, (mode, "stop margin in rows", margin, dev)
    return refs


@pytest.mark.parametrize("mode", ["prune", "stop", "both"])
def test_adaptive_runs_follow_the_spec_decisions(mode):
    """point pruning, early stopping and both on one small ragged batch each: stop, kept0/1, prune0/1 and live equal the spec's run of
    the same decision logic (see _safe_refs); matches as in the plain forward.  The fp32 run of the same model gives other bits."""
    prune, stop, width, depth, sd = _adaptive_case(mode)
    pairs = [_pair(*p) for p in ADAPTIVE_PAIRS]
    lg = _model(_conf(LAYERS, flash=True, depth_confidence=depth, width_confidence=width), sd)
    off = _model(_conf(LAYERS, depth_confidence=depth, width_confidence=width), sd)
    for model, gate in ((lg, "flash"), (off, "cuda")):
        model.point_pruning, model.early_stop = prune, stop
        model.pruning_keypoint_thresholds[gate] = 0  # (the gate each model reads)
    pb0, pb1 = _batches(pairs)
    r, r_off = lg.match_batched(pb0, pb1), off.match_batched(pb0, pb1)
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(r, pairs)[1]["ref0"], _bits(r_off, pairs)[1]["ref0"])
    B = len(pairs)
    did = 0
    for b, pair in enumerate(pairs):
        n, m = len(pair[0]), len(pair[2])
        tag = f"lgflash.{mode}.{n}x{m}"
        m0, m1 = _np(r.matches0)[b, :n], _np(r.matches1)[b, :m]
        if n == 0 or m == 0:
            assert (m0 == -1).all() and (m1 == -1).all()
            assert not stop or int(_np(r.stop)[b]) == 0
            continue
        refs = _safe_refs(mode, sd, pair, width, depth)
        spec = refs["spec"]
        la = spec["log_assignment"]
        bound = None if la is None else _peer_bound(la, [refs[pm]["log_assignment"] for pm in ("peer_a", "peer_b")], np.abs(la).max())
        if stop:
            assert int(_np(r.stop)[b]) == spec["stop"], (tag, int(_np(r.stop)[b]), spec["stop"])
            did += spec["stop"] < LAYERS
        if not prune:
            close_and_record(f"{tag}.log_assignment gpu vs spec", _np(r.la)[b, :n + 1, :m + 1], la, atol=bound)
            _check_matches(tag, {"m0": m0, "m1": m1, "s0": _np(r.scores0)[b, :n], "s1": _np(r.scores1)[b, :m]}, spec, bound)
            continue
        l0, l1 = int(_np(r.live)[b]), int(_np(r.live)[B + b])
        assert (l0, l1) == spec["live"], (tag, (l0, l1), spec["live"])
        assert np.array_equal(_np(r.kept0)[b, :l0], spec["kept0"]) and np.array_equal(_np(r.kept1)[b, :l1], spec["kept1"]), tag
        assert np.array_equal(_np(r.prune0)[b, :n], spec["prune0"]) and np.array_equal(_np(r.prune1)[b, :m], spec["prune1"]), tag
        did += l0 < n or l1 < m
        if la is None:
            assert (m0 == -1).all() and (m1 == -1).all()
            continue
        # matches over the survivors, in the survivors' indexing: the plain forward's rule on the spec's log_assignment
        k0, k1 = spec["kept0"], spec["kept1"]
        inv0, inv1 = {int(o): i for i, o in enumerate(k0)}, {int(o): i for i, o in enumerate(k1)}
        loc = lambda mm, kept, inv: np.asarray([inv[int(j)] if j >= 0 else -1 for j in mm[kept]], np.int64)  # noqa: E731
        assert (np.delete(m0, k0) == -1).all() and (np.delete(m1, k1) == -1).all(), (tag, "a pruned point matched")
        got = {"m0": loc(m0, k0, inv1), "m1": loc(m1, k1, inv0), "s0": _np(r.scores0)[b, :n][k0], "s1": _np(r.scores1)[b, :m][k1]}
        exm = {"matches0": loc(spec["matches0"], k0, inv1), "matches1": loc(spec["matches1"], k1, inv0),
               "scores0": spec["scores0"][k0], "scores1": spec["scores1"][k1]}
        _check_matches(tag, got, exm, bound, la)
    assert did > 0, "nothing stopped early and nothing was pruned: the case tests nothing"


# ------------------------------------------------------------------------------------------------ repeatability, capture, EIM
def test_twice_and_on_graph_replay_bit_equal():
    sd = _cut_sd(lgf64_shipped_state_dict(812), 3)
    pairs = [_pair(8900 + b, n, m) for b, (n, m) in enumerate([(129, 33), (300, 300), (1, 0)])]
    lg = _model(_conf(3, flash=True), sd)
    pb0, pb1 = _batches(pairs)
    call = lambda: lg.match_batched(pb0, pb1, all_layers=True)  # noqa: E731
    a, b = _bits(call(), pairs), _bits(call(), pairs)
    torch.cuda.synchronize()
    assert _equal_bits(a, b)
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
    assert _equal_bits(_bits(g, pairs), a)


def test_eim_forward_graph_equals_the_eager_flash_forward():
    Hh, Wd, B, bins = 260, 346, 2, 5
    cfg = pkg.default_config("SP_LG", event_channels=bins)
    cfg.matcher.LightGlue.n_layers = 3
    cfg.matcher.LightGlue.flash = True
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=34)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    lg = model.matcher.matcher
    assert lg.attention_mode == "fp16"
    ev = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh))
    evs = [synth_raw_events(dict(seed=810 + b, n=20000 if b else 4000, H=Hh, W=Wd, bins=bins, frac=False, pneg=False)) for b in range(B)]
    img = synth.synth_image(96, B, Hh, Wd)
    ev.step(evs, _t(img.copy()))
    rep, mask = ev.last_inputs
    _, _, m1 = model(rep, _t(img.copy()), mask)
    m1 = {k: [t.clone() for t in m1[k]] for k in ("matches0", "matching_scores0")}
    _, _, m2 = model.forward_graph(rep, _t(img.copy()), mask)
    assert all(torch.equal(a, b) for a, b in zip(m1["matches0"], m2["matches0"]))
    assert all(torch.equal(a, b) for a, b in zip(m1["matching_scores0"], m2["matching_scores0"]))
    before = len(model._graphs)
    lg.conf["flash"] = False  # baked into a capture: a new graph, and the fp32 result
    _, _, m3 = model.forward_graph(rep, _t(img.copy()), mask)
    assert len(model._graphs) == before + 1
    assert not all(torch.equal(a, b) for a, b in zip(m1["matching_scores0"], m3["matching_scores0"]))
