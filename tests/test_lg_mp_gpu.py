"""GPU tests (-m gpu), component: LightGlue `mp: True`, the layers' linears in fp16 on the matrix cores (lg_gemm_kernel on the f16
tile engine, einx_lightglue_mp).  The judge is the contract's float64 restatement (tests/lg_mp_ref.py "spec").  The
kernel alone is tested first: bit for bit on inputs whose answer is exact in every accumulation order, on values that tell the
rounding modes apart, and on random inputs under the a-priori bound of K fp32 additions.  The whole forward is bounded by the
project's rule, helpers.la_bound_f64: twice the worse of the two independent fp32 peers (peer_a: torch's matmul of the rounded
operands; peer_b: a blocked k-ascending chain) against the spec on the same inputs."""
import numpy as np
import pytest
import torch

import lg_mp_ref as MR
import lg_mp_support as S
from helpers import close_and_record, lgf64_pair, lgf64_shipped_state_dict, state_dict_for, synth, synth_raw_events
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu
N = pkg.native
GUARD = 256  # elements behind every buffer
MARK = -77.0


# ------------------------------------------------------------------------------------------------ the kernel hook
def _guarded(a, dtype=torch.float32):
    """the array on the device, flat, followed by GUARD elements of MARK"""
    a = np.ascontiguousarray(a)
    t = torch.full((a.size + GUARD,), MARK, dtype=dtype, device=DEV)
    t[:a.size] = torch.from_numpy(a.reshape(-1)).to(DEV).to(dtype)
    return t


def _guards_intact(tag, *bufs):
    for i, t in enumerate(bufs):
        if t is not None:
            assert bool((t[-GUARD:].float() == MARK).all()), (tag, "guard behind buffer", i)


class Hook:
    """one problem on the device: X [B, cap, K1] (+ X2 [B, cap, K - K1]), W [N, K] (rounded to binary16 on the device, as _pack does),
    bias [N], counts [B]; run(ldy, resid) -> Y [B, cap, ldy] float32 numpy, NaN where the kernel did not write.  Rows past a count
    hold 1e30 in X: a kernel that reads them shows it."""

    def __init__(self, X, X2, W, bias, counts):
        self.B, self.cap, self.K1 = X.shape
        self.K = self.K1 + (X2.shape[2] if X2 is not None else 0)
        self.Nn = W.shape[0]
        X, X2 = X.copy(), None if X2 is None else X2.copy()
        for b, c in enumerate(counts):
            X[b, c:] = 1e30
            if X2 is not None:
                X2[b, c:] = 1e30
        self.x, self.x2 = _guarded(X), None if X2 is None else _guarded(X2)
        self.w, self.bias = _guarded(W, torch.float16), _guarded(bias)
        self.cnt = _t(np.asarray(counts, np.int32))
        self.counts = list(counts)

    def prefill(self, ldy, resid):
        y = np.full((self.B, self.cap, ldy), np.nan, np.float32)
        if resid is not None:
            for b, c in enumerate(self.counts):
                y[b, :c, :self.Nn] = resid[b, :c]
        return _guarded(y)

    def launch(self, y, ldy, resid):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        rc = N.lib().einx_lg_linear_f16(p(self.x), p(self.x2), self.K1 if self.x2 is not None else 0, self.K, p(self.w), p(self.bias), self.Nn, p(y), ldy,
                                        p(y) if resid is not None else None, p(self.cnt), self.cap, self.B, 1 if resid is not None else 0,
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.lib().einx_last_error()

    def run(self, ldy, resid=None, tag=None):
        y = self.prefill(ldy, resid)
        self.launch(y, ldy, resid)
        torch.cuda.synchronize()
        _guards_intact(tag, self.x, self.x2, self.w, self.bias, y)
        return _np(y)[:-GUARD].reshape(self.B, self.cap, ldy)


def _check_written(tag, Y, want, counts, Nn):
    """rows below the count and columns below N equal `want` bit for bit; everything else still NaN"""
    for b, c in enumerate(counts):
        got = Y[b, :c, :Nn]
        bad = np.nonzero(got.view(np.uint32) != np.ascontiguousarray(want[b, :c], np.float32).view(np.uint32))
        assert bad[0].size == 0, (tag, b, bad[0].size, [int(i[0]) for i in bad], float(got[bad[0][0], bad[1][0]]), float(want[b, bad[0][0], bad[1][0]]))
        assert np.isnan(Y[b, c:]).all(), (tag, b, "rows past the count written")
        assert np.isnan(Y[b, :, Nn:]).all(), (tag, b, "columns past N written")


KS = [(4, 0), (60, 0), (64, 0), (68, 0), (256, 0), (256, 256)]  # (K1, K2): K = 512 as 256 | 256 through X2
NS = [4, 124, 128, 132, 256, 512]
CAP = 384
COUNTS = [[0, 1, 127], [128, 129, 300], [300, 0, 129], [1, 128, 127]]


@pytest.mark.parametrize("K1,K2", KS)
def test_exact_inputs_bit_for_bit(K1, K2):
    """X holds integers in [-8, 8], W, the bias and the residual multiples of 1/16 in [-1, 1] (the residual in [-8, 8]): every partial
    sum is a multiple of 1/16 below 2^13, exactly representable in fp32, so the output must equal the float64 result in ANY
    accumulation order.  K below, at and above the 32-deep slab and the 64 of two slabs; N below, at and above the 128-column tile,
    one to four tiles; counts 0, 1, around the 128-row tile and three tiles at cap 384; both row strides of Y; with and without the
    residual -- all crossed.  Rows past the count and columns past N keep their NaN prefill, the guards behind all five buffers stay untouched."""
    rng = np.random.default_rng(1000 + K1 + K2)
    K = K1 + K2
    for Nn in NS:
        X = rng.integers(-8, 9, (3, CAP, K)).astype(np.float32)
        W = (rng.integers(-16, 17, (Nn, K)) / 16.0).astype(np.float32)
        bias = (rng.integers(-16, 17, Nn) / 16.0).astype(np.float32)
        R = (rng.integers(-128, 129, (3, CAP, Nn)) / 16.0).astype(np.float32)
        prod = X.astype(np.float64) @ W.astype(np.float64).T + bias.astype(np.float64)
        for counts in COUNTS:  # every count set meets every (N, row stride, epilogue)
            h = Hook(X[..., :K1], X[..., K1:] if K2 else None, W, bias, counts)
            for ldy in (Nn, Nn + 12):
                for resid in (None, R):
                    tag = ("exact", K1, K2, Nn, ldy, resid is not None, tuple(counts))
                    want = prod + (R if resid is not None else 0.0)
                    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
                    _check_written(tag, h.run(ldy, resid, tag), want.astype(np.float32), counts, Nn)


def test_twice_and_on_graph_replay_bit_equal():
    """the widest case (K = 256 | 256, N = 512, residual) on random inputs: two launches and a captured replay give the same bits"""
    rng = np.random.default_rng(7)
    counts = [300, 129, 1]
    X, X2 = (rng.standard_normal((3, CAP, 256)).astype(np.float32) for _ in range(2))
    W, bias = (rng.standard_normal((512, 512)) / 16).astype(np.float32), rng.standard_normal(512).astype(np.float32)
    R = rng.standard_normal((3, CAP, 512)).astype(np.float32)
    h = Hook(X, X2, W, bias, counts)
    a, b = h.run(512, R, "twice a"), h.run(512, R, "twice b")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    y0 = h.prefill(512, R)
    y = y0.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        h.launch(y, 512, R)  # warm-up on the capture stream
        y.copy_(y0)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        h.launch(y, 512, R)
    graph.replay()
    torch.cuda.synchronize()
    _guards_intact("graph", y)
    assert np.array_equal(_np(y)[:-GUARD].view(np.uint32), a.reshape(-1).view(np.uint32))


def test_the_rounding_is_nearest_even_with_overflow_to_infinity():
    """W = identity (K = N = 64): the output is the rounded input, bit for bit x.half().float().  1 + 2^-11 is a tie and goes to the
    even 1; 1 + 3 2^-11 is a tie and goes to the even 1 + 2^-9 (round toward zero gives 1 + 2^-10); 65519 is below the overflow
    threshold 65520 and gives 65504; random values of every binade of the normal range.  One row of all-positive weights over an x
    of 65520 gives +inf: overflow goes to infinity, not to the largest finite value."""
    rng = np.random.default_rng(11)
    rows = 200
    X = (rng.standard_normal((1, rows, 64)) * np.exp2(rng.integers(-12, 15, (1, rows, 64)))).astype(np.float32)
    X[np.abs(X) < 2.0 ** -14] = 1.0  # (operands below the binary16 normal range are not part of the contract)
    X[np.abs(X) > 65000] = 3.0
    e = 2.0 ** -11
    special = np.asarray([1 + e, 1 + 3 * e, -(1 + e), -(1 + 3 * e), 65519.0, -65519.0, 1 + e + 2.0 ** -23, 1 + e - 2.0 ** -23, 2.0 ** -14, 1e-9, -1e-9, 0.0],
                         np.float32)
    X[0, 0, :len(special)] = special
    h = Hook(X, None, np.eye(64, dtype=np.float32), np.zeros(64, np.float32), [rows])
    Y = h.run(64, None, "identity")
    want = torch.from_numpy(X).half().float().numpy()
    assert want[0, 0, :6].tolist() == [1.0, 1.0 + 2.0 ** -9, -1.0, -(1.0 + 2.0 ** -9), 65504.0, -65504.0]
    assert np.array_equal(Y[0], want[0])
    Xo = np.ones((1, 3, 64), np.float32)
    Xo[0, 1, 37] = 65520.0
    Yo = Hook(Xo, None, np.ones((64, 64), np.float32), np.zeros(64, np.float32), [3]).run(64, None, "overflow")
    assert (Yo[0, 0] == 64.0).all() and (Yo[0, 2] == 64.0).all() and np.isposinf(Yo[0, 1]).all()


def test_probe_operands_below_the_normal_range_recorded_not_gated():
    """Operands whose rounded magnitude is below 2^-14 are outside the contract; what the hardware does with them is RECORDED here
    (parity_errors.json), not asserted: the distance of the kernel from `x.half().float()` for binary16-subnormal
    inputs under a weight of 1, and from the exact product for normal inputs under a binary16-subnormal weight of 2^-20.  0 in both
    rows means the f16 matrix instruction keeps subnormals in that operand; a flush shows as the operand's own magnitude."""
    vals = np.asarray([2.0 ** -15, 2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, 1023 * 2.0 ** -24], np.float32)
    X = np.zeros((1, 2, 64), np.float32)
    X[0, 0, :len(vals)], X[0, 1, :len(vals)] = vals, -vals
    want = torch.from_numpy(X).half().float().numpy().astype(np.float64)
    zero = np.zeros(64, np.float32)
    Y = Hook(X, None, np.eye(64, dtype=np.float32), zero, [2]).run(64, None, "subnormal x")
    close_and_record("lgmp.probe.subnormal x under w = 1, gpu vs x.half() (not a gate; 0 = kept)", Y[0], want[0], atol=np.inf)
    Xn = X * np.float32(1024.0)  # normal in binary16
    Yw = Hook(Xn, None, np.eye(64, dtype=np.float32) * np.float32(2.0 ** -20), zero, [2]).run(64, None, "subnormal w")
    wantw = torch.from_numpy(Xn).half().double().numpy() * 2.0 ** -20
    close_and_record("lgmp.probe.normal x under subnormal w = 2^-20, gpu vs exact (not a gate; 0 = kept)", Yw[0], wantw[0], atol=np.inf)
    assert np.isfinite(Y).all() and np.isfinite(Yw).all()


@pytest.mark.parametrize("K1,K2,Nn", [(256, 0, 768), (256, 256, 512), (512, 0, 256), (68, 0, 132)])
def test_random_inputs_against_the_spec(K1, K2, Nn):
    """random inputs at LightGlue's magnitudes against the float64 spec on the rounded operands, per output under the a-priori bound
    of K fp32 additions on exact products, K 2^-24 sum_k |x_k w_k| (x, w the rounded operands): no measured tolerance"""
    rng = np.random.default_rng(K1 + K2 + Nn)
    K = K1 + K2
    counts = [300, 129, 33]
    X = (rng.standard_normal((3, CAP, K)) * 1.5).astype(np.float32)
    W = (rng.standard_normal((Nn, K)) / np.sqrt(K)).astype(np.float32)
    bias = (rng.standard_normal(Nn) * 0.05).astype(np.float32)
    R = rng.standard_normal((3, CAP, Nn)).astype(np.float32)
    h = Hook(X[..., :K1], X[..., K1:] if K2 else None, W, bias, counts)
    r16 = lambda a: a.astype(np.float16).astype(np.float64)  # noqa: E731
    for resid in (None, R):
        Y = h.run(Nn, resid, ("random", K, Nn))
        for b, c in enumerate(counts):
            spec = MR.linear_np(X[b, :c], W, bias, "spec")
            bound = K * 2.0 ** -24 * (np.abs(r16(X[b, :c])) @ np.abs(r16(W)).T)
            got = Y[b, :c].astype(np.float64) - (resid[b, :c] if resid is not None else 0.0)
            if resid is not None:  # one more fp32 addition, of the residual
                bound = bound + 2.0 ** -24 * (np.abs(spec) + np.abs(resid[b, :c]))
            err = np.abs(got - spec)
            close_and_record(f"lgmp.linear.{K}x{Nn}{'.resid' if resid is not None else ''} gpu vs spec (worst err / bound)", (err / bound).max(), 0.0,
                             atol=1.0)
            assert np.isnan(Y[b, c:]).all()


# ------------------------------------------------------------------------------------------------ the whole forward
def _model(conf, sd, mixed=True):
    return S.model(conf, sd, mixed=mixed)


def _check_pair(tag, sd, pair, got, flash, **kw):
    """the project's rule for a pair (tests/test_lightglue_f64_gpu.py) with the mp spec (over the flash spec when `flash`) as the exact answer and its
    two fp32 peers: log_assignment and the descriptors after every layer within la_bound_f64 of the spec, assignments equal to the
    spec's decisions except at rows / columns whose spec margin is inside that bound"""
    k0, d0, k1, d1 = pair
    n, m = len(k0), len(k1)
    if n == 0 or m == 0:
        assert (got["m0"] == -1).all() and (got["m1"] == -1).all(), tag
        return None
    ex = MR.forward(sd, *pair, flash=flash, **kw)
    peers = [MR.forward(sd, *pair, mode=mode, flash=flash, **kw) for mode in ("peer_a", "peer_b")]
    la = ex["log_assignment"]
    assert got["la"].shape == (n + 1, m + 1) and got["la"][n, m] == 0
    bound = S.peer_bound(la, [p["log_assignment"] for p in peers], np.abs(la).max())
    for name, p in zip(("peer_a", "peer_b"), peers):
        close_and_record(f"{tag}.log_assignment {name} vs spec", p["log_assignment"], la, atol=bound)
    close_and_record(f"{tag}.log_assignment gpu vs spec", got["la"], la, atol=bound)
    if got.get("layers") is not None:
        worst = None
        for i, xs in enumerate(ex["layers"]):
            for s, x in enumerate(xs):
                b = S.peer_bound(x, [p["layers"][i][s] for p in peers], np.abs(x).max())
                err = float(np.abs(got["layers"][i][s].astype(np.float64) - x).max())
                assert err <= b, f"{tag}: layer {i} side {s}: |gpu - spec| = {err:.3e} > {b:.3e}"
                if worst is None or err / b > worst[0]:
                    worst = (err / b, i, s, b)
        _, i, s, b = worst
        for name, p in zip(("peer_a", "peer_b"), peers):
            close_and_record(f"{tag}.descriptors (gpu's worst layer) {name} vs spec", p["layers"][i][s], ex["layers"][i][s], atol=b)
        close_and_record(f"{tag}.descriptors (worst layer) gpu vs spec", got["layers"][i][s], ex["layers"][i][s], atol=b)
    S.check_matches(tag, got, ex, bound)
    return ex


_feats = S.feats


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("case", [f[0] for f in S.FORWARD])
def test_forward_every_pair_against_the_spec(case, flash):
    """3 and 9 layers, ragged batches of counts 0 / 1 / 33 / 129 / 300 (a count of 1 paired with a longer side), stacked
    and unstacked sides; mp alone and mp + flash.  Off is off: with the attribute false, or with `mp: False`, the outputs are
    torch.equal to those of a model built without the key."""
    _, layers, counts, cap0, cap1 = next(f for f in S.FORWARD if f[0] == case)
    sd = S.cut_sd(lgf64_shipped_state_dict(821), layers)
    pairs = [S.pair(9800 + 17 * b + layers, n, m) for b, (n, m) in enumerate(counts)]
    on = _model(S.conf(layers, mp=True, flash=flash), sd)
    attr_off = _model(S.conf(layers, mp=True, flash=flash), sd, mixed=False)
    key_off = _model(S.conf(layers, mp=False, flash=flash), sd)
    plain = S.model(S.conf(layers, flash=flash), sd)
    assert [lg.linear_mode for lg in (on, attr_off, key_off, plain)] == ["fp16", "fp32", "fp32", "fp32"]
    assert {lg.attention_mode for lg in (on, attr_off, key_off, plain)} == {"fp16" if flash else "fp32"}
    pb0, pb1 = S.batches(pairs, cap0, cap1)
    r_on, r_attr, r_key, r_plain = (lg.match_batched(pb0, pb1, all_layers=True) for lg in (on, attr_off, key_off, plain))
    torch.cuda.synchronize()
    b_on, b_plain = S.bits(r_on, pairs), S.bits(r_plain, pairs)
    assert S.equal_bits(S.bits(r_attr, pairs), b_plain) and S.equal_bits(S.bits(r_key, pairs), b_plain)
    for x, y in zip(b_on, b_plain):
        if "la" in x:
            assert not np.array_equal(x["la"], y["la"]) and not np.array_equal(x["ref0"], y["ref0"]) and not np.array_equal(x["ref1"], y["ref1"])
    tag = f"lgmp{'.flash' if flash else ''}.{case}"
    for b, got in enumerate(S.cut(r_on, pairs)):
        _check_pair(tag, sd, pairs[b], got, flash)
    # the front door on one pair (B = 1: the wide kernel, there is no small-grid twin)
    k0, d0, k1, d1 = pairs[0]
    if len(k0) and len(k1):
        pred = on(_feats(k0, d0), _feats(k1, d1))
        one = {"la": _np(pred["log_assignment"])[0], "m0": _np(pred["matches0"])[0], "m1": _np(pred["matches1"])[0],
               "s0": _np(pred["matching_scores0"])[0], "s1": _np(pred["matching_scores1"])[0]}
        _check_pair(tag + ".single", sd, pairs[0], one, flash)


def test_loss_takes_an_mp_pred_unchanged():
    """LightGlue.loss (eval) reads the forward's ref_descriptors and the last head, which stays fp32 under the mode: on an mp
    forward's pred it gives what the fp32 model's loss gives on the same pred, bit for bit"""
    sd = S.cut_sd(lgf64_shipped_state_dict(824), 3)
    on, off = _model(S.conf(3, mp=True), sd), S.model(S.conf(3), sd)
    k0, d0, k1, d1 = S.pair(9960, 33, 33)
    pred = on(_feats(k0, d0), _feats(k1, d1))
    m0 = pred["matches0"]
    data = {"gt_matches0": m0.clone(), "gt_matches1": pred["matches1"].clone(),
            "gt_assignment": (m0[:, :, None] == torch.arange(33, device=DEV)[None, None, :])}
    a, _ = on.loss(pred, data)
    b, _ = off.loss(pred, data)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) and bool(torch.isfinite(a["total"]).all())


@pytest.mark.parametrize("flash", [False, True])
def test_other_widths_one_layer_against_the_spec(flash):
    """d = 128 with 4 heads of 32 (the rotary epilogue for any width, EPI_ROPE_ANY; no merged to_qk | to_v; LayerNorm over 256) behind
    an input_proj from 64 columns, which stays fp32; one layer, so the q / k / v the rotary epilogue wrote are one attention and five
    linears away from the descriptors compared.  (d = 256 with 4 heads of 64, EPI_ROPE, is every case of the test above.)"""
    conf = dict(input_dim=64, descriptor_dim=128, num_heads=4, n_layers=1, mp=True, flash=flash)
    lg = pkg.LightGlue(conf).to(DEV)
    sd = state_dict_for(dict(wseed=823, state_keys={k: list(v.shape) for k, v in lg.state_dict().items()}))
    lg = _model(conf, sd)
    assert lg.linear_mode == "fp16" and lg._pack(True)[1][0].Wqk_v_h is None and lg._pack(True)[0].in_w
    pairs = []
    for b, (n, m) in enumerate([(129, 33), (1, 130), (40, 0)]):
        d0, d1, k0, k1 = lgf64_pair(9900 + b, max(n, 1), max(m, 1), 64)
        pairs.append((k0[:n], d0[:n], k1[:m], d1[:m]))
    for caps in ((130, 130), (129, 130)):  # stacked, unstacked
        pb0, pb1 = S.batches(pairs, *caps)
        r = lg.match_batched(pb0, pb1, all_layers=True)
        torch.cuda.synchronize()
        for b, got in enumerate(S.cut(r, pairs)):
            _check_pair(f"lgmp{'.flash' if flash else ''}.d128h4.cap{caps[0]}", sd, pairs[b], got, flash, num_heads=4)


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("mode", ["prune", "stop", "both"])
def test_adaptive_runs_follow_the_spec_decisions(mode, flash):
    """point pruning, early stopping and both under the mode (the model and pairs of lg_mp_support, whose spec decisions are out of
    the rounding's reach under this contract: lg_mp_ref.safe_refs, checked in tests/test_lg_mp_cpu.py): stop, kept0/1,
    prune0/1 and live equal the spec's run of the same decision logic; matches as in the plain forward"""
    prune, stop, width, depth, sd = S.adaptive_case(mode)
    pairs = [S.pair(*p) for p in S.ADAPTIVE_PAIRS]
    lg = _model(S.conf(S.LAYERS, mp=True, flash=flash, depth_confidence=depth, width_confidence=width), sd)
    off = S.model(S.conf(S.LAYERS, flash=flash, depth_confidence=depth, width_confidence=width), sd)
    for model in (lg, off):
        model.point_pruning, model.early_stop = prune, stop
        model.pruning_keypoint_thresholds["flash" if flash else "cuda"] = 0
    pb0, pb1 = S.batches(pairs)
    r, r_off = lg.match_batched(pb0, pb1), off.match_batched(pb0, pb1)
    torch.cuda.synchronize()
    assert not np.array_equal(S.bits(r, pairs)[1]["ref0"], S.bits(r_off, pairs)[1]["ref0"])
    B = len(pairs)
    did = 0
    for b, pair in enumerate(pairs):
        n, m = len(pair[0]), len(pair[2])
        tag = f"lgmp{'.flash' if flash else ''}.{mode}.{n}x{m}"
        m0, m1 = _np(r.matches0)[b, :n], _np(r.matches1)[b, :m]
        if n == 0 or m == 0:
            assert (m0 == -1).all() and (m1 == -1).all()
            assert not stop or int(_np(r.stop)[b]) == 0
            continue
        refs = MR.safe_refs(mode, sd, pair, width, depth, flash)
        spec = refs["spec"]
        la = spec["log_assignment"]
        bound = None if la is None else S.peer_bound(la, [refs[pm]["log_assignment"] for pm in ("peer_a", "peer_b")], np.abs(la).max())
        if stop:
            assert int(_np(r.stop)[b]) == spec["stop"], (tag, int(_np(r.stop)[b]), spec["stop"])
            did += spec["stop"] < S.LAYERS
        if not prune:
            close_and_record(f"{tag}.log_assignment gpu vs spec", _np(r.la)[b, :n + 1, :m + 1], la, atol=bound)
            S.check_matches(tag, {"m0": m0, "m1": m1, "s0": _np(r.scores0)[b, :n], "s1": _np(r.scores1)[b, :m]}, spec, bound)
            continue
        l0, l1 = int(_np(r.live)[b]), int(_np(r.live)[B + b])
        assert (l0, l1) == spec["live"], (tag, (l0, l1), spec["live"])
        assert np.array_equal(_np(r.kept0)[b, :l0], spec["kept0"]) and np.array_equal(_np(r.kept1)[b, :l1], spec["kept1"]), tag
        assert np.array_equal(_np(r.prune0)[b, :n], spec["prune0"]) and np.array_equal(_np(r.prune1)[b, :m], spec["prune1"]), tag
        did += l0 < n or l1 < m
        if la is None:
            assert (m0 == -1).all() and (m1 == -1).all()
            continue
        k0, k1 = spec["kept0"], spec["kept1"]
        inv0, inv1 = {int(o): i for i, o in enumerate(k0)}, {int(o): i for i, o in enumerate(k1)}
        loc = lambda mm, kept, inv: np.asarray([inv[int(j)] if j >= 0 else -1 for j in mm[kept]], np.int64)  # noqa: E731
        assert (np.delete(m0, k0) == -1).all() and (np.delete(m1, k1) == -1).all(), (tag, "a pruned point matched")
        got = {"m0": loc(m0, k0, inv1), "m1": loc(m1, k1, inv0), "s0": _np(r.scores0)[b, :n][k0], "s1": _np(r.scores1)[b, :m][k1]}
        exm = {"matches0": loc(spec["matches0"], k0, inv1), "matches1": loc(spec["matches1"], k1, inv0),
               "scores0": spec["scores0"][k0], "scores1": spec["scores1"][k1]}
        S.check_matches(tag, got, exm, bound, la)
    assert did > 0, "nothing stopped early and nothing was pruned: the case tests nothing"


# ------------------------------------------------------------------------------------------------ repeatability, capture, EIM
def test_forward_twice_and_on_graph_replay_bit_equal():
    sd = S.cut_sd(lgf64_shipped_state_dict(822), 3)
    pairs = [S.pair(9950 + b, n, m) for b, (n, m) in enumerate([(129, 33), (300, 300), (1, 0)])]
    lg = _model(S.conf(3, mp=True), sd)
    pb0, pb1 = S.batches(pairs)
    call = lambda: lg.match_batched(pb0, pb1, all_layers=True)  # noqa: E731
    a, b = S.bits(call(), pairs), S.bits(call(), pairs)
    torch.cuda.synchronize()
    assert S.equal_bits(a, b)
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
    assert S.equal_bits(S.bits(g, pairs), a)
    lg.mixed_precision = False  # read at every call: the next forward is the fp32 one, and back
    c = S.bits(call(), pairs)
    lg.mixed_precision = True
    d = S.bits(call(), pairs)
    torch.cuda.synchronize()
    assert not S.equal_bits(c, a) and S.equal_bits(d, a)
    assert S.equal_bits(c, S.bits(S.model(S.conf(3), sd).match_batched(pb0, pb1, all_layers=True), pairs))


def test_eim_forward_graph_equals_the_eager_mp_forward():
    Hh, Wd, B, bins = 260, 346, 2, 5
    cfg = pkg.default_config("SP_LG", event_channels=bins)
    cfg.matcher.LightGlue.n_layers = 3
    cfg.matcher.LightGlue.mp = True
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=35)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    lg = model.matcher.matcher
    assert lg.linear_mode == "fp32"  # the key alone does nothing
    lg.mixed_precision = True
    assert lg.linear_mode == "fp16"
    ev = pkg.DifferentTimeEvaluator(model, bins=bins, resolution=(Wd, Hh))
    evs = [synth_raw_events(dict(seed=820 + b, n=20000 if b else 4000, H=Hh, W=Wd, bins=bins, frac=False, pneg=False)) for b in range(B)]
    img = synth.synth_image(97, B, Hh, Wd)
    ev.step(evs, _t(img.copy()))
    rep, mask = ev.last_inputs
    _, _, m1 = model(rep, _t(img.copy()), mask)
    m1 = {k: [t.clone() for t in m1[k]] for k in ("matches0", "matching_scores0")}
    _, _, m2 = model.forward_graph(rep, _t(img.copy()), mask)
    assert all(torch.equal(a, b) for a, b in zip(m1["matches0"], m2["matches0"]))
    assert all(torch.equal(a, b) for a, b in zip(m1["matching_scores0"], m2["matching_scores0"]))
    before = len(model._graphs)
    lg.mixed_precision = False  # baked into a capture: a new graph, and the fp32 result
    _, _, m3 = model.forward_graph(rep, _t(img.copy()), mask)
    assert len(model._graphs) == before + 1
    assert not all(torch.equal(a, b) for a, b in zip(m1["matching_scores0"], m3["matching_scores0"]))
    m3 = {k: [t.clone() for t in m3[k]] for k in ("matches0", "matching_scores0")}
    # and back, twice: the first graphs are replayed (no new capture), and what they read -- both weight images and the ONE watch
    # the two modes share -- is still what they captured
    watch = lg._watch
    for mixed, want in ((True, m1), (False, m3), (True, m1)):
        lg.mixed_precision = mixed
        _, _, m = model.forward_graph(rep, _t(img.copy()), mask)
        assert len(model._graphs) == before + 1 and lg._watch is watch
        assert all(torch.equal(a, b) for a, b in zip(want["matches0"], m["matches0"]))
        assert all(torch.equal(a, b) for a, b in zip(want["matching_scores0"], m["matching_scores0"]))


def test_weight_edits_rebuild_the_fp16_images():
    """the binary16 images are made at pack time: an edit through `.data` (seen by the content watch, which makes forward() repack
    and match again) and an in-place edit (seen by the version counter) both reach them -- the result is that of a fresh model built
    on the edited weights, bit for bit"""
    sd = S.cut_sd(lgf64_shipped_state_dict(825), 3)
    lg = _model(S.conf(3, mp=True), sd)
    k0, d0, k1, d1 = S.pair(9970, 129, 33)
    la = lambda m: m(_feats(k0, d0), _feats(k1, d1))["log_assignment"].clone()  # noqa: E731
    first = la(lg)
    key = "transformers.1.cross_attn.to_out.weight"
    lg.transformers[1].cross_attn.to_out.weight.data.mul_(0.5)
    sd[key] = sd[key] * np.float32(0.5)
    second = la(lg)
    assert not torch.equal(first, second) and torch.equal(second, la(_model(S.conf(3, mp=True), sd)))
    key = "transformers.0.self_attn.ffn.3.weight"
    with torch.no_grad():
        lg.transformers[0].self_attn.ffn[3].weight.mul_(0.5)
    sd[key] = sd[key] * np.float32(0.5)
    third = la(lg)
    assert not torch.equal(second, third) and torch.equal(third, la(_model(S.conf(3, mp=True), sd)))


def test_switch_on_a_device_is_read_at_every_call():
    """key and attribute, eval mode, parameters on the GPU; independent of flash (the CPU side is tests/test_lg_mp_cpu.py)"""
    on = pkg.LightGlue({"mp": True}).to(DEV).eval()
    assert on.linear_mode == "fp32"
    on.mixed_precision = True
    assert on.linear_mode == "fp16" and on.attention_mode == "fp32"
    on.conf["mp"] = False
    assert on.linear_mode == "fp32"
    on.conf["mp"] = True
    assert on.train().linear_mode == "fp32" and on.eval().linear_mode == "fp16"
    both = pkg.LightGlue({"mp": True, "flash": True}).to(DEV).eval()
    both.mixed_precision = True
    assert (both.linear_mode, both.attention_mode) == ("fp16", "fp16")
    assert on.cpu().linear_mode == "fp32"


@pytest.mark.parametrize("first_mp", [False, True])
def test_weight_edits_between_mode_switches_reach_both_images(first_mp):
    """Both images (the folded fp32 one, the unfolded one with the binary16 weights) are cached side by side under ONE weight watch,
    whose reference is taken when the first of them is packed.  A forward in one mode, an edit through `.data`, a forward in the
    other mode (its image is packed from the new values; the watch still holds the old reference, raises the flag, both images are
    dropped), then back: every forward after the edit equals a fresh model built on the edited weights, bit for bit, in both modes
    and both orders."""
    sd = S.cut_sd(lgf64_shipped_state_dict(826), 3)
    lg = _model(S.conf(3, mp=True), sd, mixed=first_mp)
    k0, d0, k1, d1 = S.pair(9980, 129, 33)
    la = lambda m: m(_feats(k0, d0), _feats(k1, d1))["log_assignment"].clone()  # noqa: E731
    before = la(lg)
    watch = lg._watch
    for key, mod in (("transformers.0.self_attn.out_proj.weight", lg.transformers[0].self_attn.out_proj),  # folded into ffn.0 in fp32
                     ("transformers.2.cross_attn.to_v.weight", lg.transformers[2].cross_attn.to_v)):       # copied into Wqk_v
        mod.weight.data.mul_(0.5)
        sd[key] = sd[key] * np.float32(0.5)
    fresh = {mixed: la(_model(S.conf(3, mp=True), sd, mixed=mixed)) for mixed in (False, True)}
    lg.mixed_precision = not first_mp
    other = la(lg)
    assert lg._watch is not watch  # the edit was seen at the other mode's first forward: a new set of images, a new watch
    lg.mixed_precision = first_mp
    back = la(lg)
    assert torch.equal(other, fresh[not first_mp]) and torch.equal(back, fresh[first_mp]) and not torch.equal(back, before)
    # without an edit the two images share the watch: switching modes neither repacks nor replaces it
    watch = lg._watch
    images = (lg._packed, lg._packed_mp)
    assert all(im is not None for im in images)
    lg.mixed_precision = not first_mp
    assert torch.equal(la(lg), other) and lg._watch is watch and (lg._packed, lg._packed_mp) == images
