"""GPU tests (-m gpu), component: lightglue against its float64 forward (tests/lg_f64.py) across the kernel dispatch.
Every pair checked: log_assignment (dustbins included) and the descriptors after every layer within helpers.la_bound_f64 of the
exact answer -- twice the worse of the two independent fp32 peers on the same inputs (lg_f64 in float32, the oracle) --,
assignments equal to the float64 decisions outside the near-tie / filter-edge rows of the float64 margins, matching scores to FTOL.  Every comparison is recorded under lgf64.<case>.* (gpu / oracle / float32 side by side in parity_errors.json)."""
from importlib import import_module

import numpy as np
import pytest
import torch

import lg_f64
from helpers import LGF64_PAIRS, close_and_record, la_bound_f64, lgf64_pair, lgf64_shipped_state_dict, record_flips, synth
from gpu_support import DEV, FTOL, LGCFG, _conf, _lgcfg_model, _np, _t, pkg

pytestmark = pytest.mark.gpu
PairBatch = import_module(pkg.__name__ + ".core.modules.matchers._batched").PairBatch
SHIPPED = dict(input_dim=256, descriptor_dim=256, num_heads=4, n_layers=9)


def _model(conf, sd, merge=True, fold=True):
    lg = pkg.LightGlue(conf).to(DEV)
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    lg.merge_qk_v, lg.fold_message_projection = merge, fold
    lg.refresh()
    return lg.eval()


def _gate_layers(tag, got, ex, f32, orc):
    """descriptors after each layer: each layer within la_bound_f64 of ITS peers; the worst layer (largest error / bound) of every
    source is recorded"""
    worst = None
    for i, xs in enumerate(ex["layers"]):
        for s in range(2):
            x = xs[s]
            peers = {"float32": np.abs(f32["layers"][i][s] - x).max()}
            if orc is not None:
                peers["oracle"] = np.abs(orc["layers"][i][s] - x).max()
            bound = la_bound_f64(peers.values(), np.abs(x).max())
            err = float(np.abs(got[i][s].astype(np.float64) - x).max())
            assert err <= bound, f"{tag}: layer {i} side {s}: |gpu - float64| = {err:.3e} > {bound:.3e} (peers {peers})"
            if worst is None or err / bound > worst[0]:
                worst = (err / bound, i, s, bound)
    _, i, s, bound = worst
    x = ex["layers"][i][s]
    close_and_record(f"{tag}.descriptors (worst layer) gpu vs float64", got[i][s], x, atol=bound)
    close_and_record(f"{tag}.descriptors (worst layer) float32 vs float64", f32["layers"][i][s], x, atol=bound)
    if orc is not None:
        close_and_record(f"{tag}.descriptors (worst layer) oracle vs float64", orc["layers"][i][s], x, atol=bound)


def _check_pair(tag, sd, conf, pair, got, oracle=None, th=0.0, orc=None, fixture=None):
    """pair = (k0, d0, k1, d1, size0, size1); got = the GPU's {la [n+1, m+1], layers [(x0, x1)] or None, m0, m1, s0, s1}; `orc` =
    an oracle run already made on the pair, else the `oracle` fixture runs it; `fixture`: a helpers.la_bound tag the bound may not
    exceed.  The oracle is a peer on every pair: its k-ordered sums round like the kernels' (up to twice as far from the exact
    value as torch's blocked fp32 sums: lgf64.*.log_assignment float32 / oracle in parity_errors.json), so torch alone would
    not be a fair peer"""
    assert orc is not None or oracle is not None
    k0, d0, k1, d1, size0, size1 = pair
    n, m = len(k0), len(k1)
    kw = dict(size0=size0, size1=size1, filter_threshold=th)
    ex = lg_f64.forward(sd, k0, d0, k1, d1, **kw)
    f32 = lg_f64.forward(sd, k0, d0, k1, d1, dtype=torch.float32, **kw)
    if orc is None:
        orc = oracle.lightglue(sd, k0, d0, k1, d1, n_layers=conf["n_layers"], heads=conf["num_heads"],
                               capture_layers=range(conf["n_layers"]), **kw)
        orc["layers"] = [orc["layers"][i] for i in range(conf["n_layers"])]
    la = ex["log_assignment"]
    assert got["la"].shape == (n + 1, m + 1) and got["la"][n, m] == 0
    peers = [np.abs(f32["log_assignment"] - la).max()] + ([np.abs(orc["log_assignment"] - la).max()] if orc is not None else [])
    bound = la_bound_f64(peers, np.abs(la).max(), fixture)
    close_and_record(f"{tag}.log_assignment float32 vs float64", f32["log_assignment"], la, atol=bound)
    if orc is not None:
        close_and_record(f"{tag}.log_assignment oracle vs float64", orc["log_assignment"], la, atol=bound)
    close_and_record(f"{tag}.log_assignment gpu vs float64", got["la"], la, atol=bound)
    if got["layers"] is not None:
        _gate_layers(tag, got["layers"], ex, f32, orc)
    # assignments: equal to the float64 decisions except at rows / columns whose float64 margin is inside the bound
    row_ok = (ex["row_gap"] < bound) | (ex["edge_dist"] < bound)
    col_ok = ex["col_gap"] < bound
    m0, m1, e0, e1 = got["m0"], got["m1"], ex["matches0"], ex["matches1"]
    assert (m0 < m).all() and (m1 < n).all()
    for i in np.nonzero(m0 != e0)[0]:
        assert row_ok[i] or any(col_ok[j] for j in (m0[i], e0[i]) if j >= 0), (tag, "row", int(i), int(m0[i]), int(e0[i]))
    for j in np.nonzero(m1 != e1)[0]:
        assert col_ok[j] or any(row_ok[i] for i in (m1[j], e1[j]) if i >= 0), (tag, "column", int(j), int(m1[j]), int(e1[j]))
    record_flips(f"{tag}.matches0 gpu vs float64", m0, e0, la)
    record_flips(f"{tag}.matches1 gpu vs float64", m1, e1, la.T)
    if orc is not None:
        record_flips(f"{tag}.matches0 oracle vs float64", orc["matches0"], e0, la)
    record_flips(f"{tag}.matches0 float32 vs float64", f32["matches0"], e0, la)
    same0, same1 = m0 == e0, m1 == e1  # a flipped row's score may be 0 on one side (mutual best lost)
    close_and_record(f"{tag}.matching_scores0 gpu vs float64", got["s0"][same0], ex["scores0"][same0], atol=FTOL)
    close_and_record(f"{tag}.matching_scores1 gpu vs float64", got["s1"][same1], ex["scores1"][same1], atol=FTOL)
    return ex


def _feats(k, d, size):
    return {"sparse_descriptors": _t(d)[None], "sparse_positions": _t(k)[None], "image_size": [torch.tensor(size)]}


def _run_single(lg, pair):
    """front door (LightGlue.forward on one pair) + the same pair through match_batched(all_layers=True) for the layers"""
    k0, d0, k1, d1, size0, size1 = pair
    n, m = len(k0), len(k1)
    r = lg(_feats(k0, d0, size0), _feats(k1, d1, size1))
    pb0, pb1 = _batch([k0], [d0], n, size0), _batch([k1], [d1], m, size1)
    a = lg.match_batched(pb0, pb1, all_layers=True)
    la = _np(r["log_assignment"])[0]
    assert np.array_equal(_np(a.la)[0], la)  # all_layers only adds outputs
    ref0, ref1 = _np(a.ref0)[0], _np(a.ref1)[0]
    return {"la": la, "layers": [(ref0[i, :n], ref1[i, :m]) for i in range(ref0.shape[0])], "m0": _np(r["matches0"])[0],
            "m1": _np(r["matches1"])[0], "s0": _np(r["matching_scores0"])[0], "s1": _np(r["matching_scores1"])[0]}


def _batch(ks, ds, cap, size, kfill=1e6, dfill=7.0):
    """PairBatch of ragged entries; the padding rows hold garbage (far keypoints, a constant descriptor)"""
    B, din = len(ks), ds[0].shape[1]
    K, D = np.full((B, cap, 3), kfill, np.float32), np.full((B, cap, din), dfill, np.float32)
    for b in range(B):
        K[b, :len(ks[b])], D[b, :len(ds[b])] = ks[b], ds[b]
    pb = PairBatch()
    pb.kpts, pb.desc, pb.counts = _t(K), _t(D), _t(np.asarray([len(k) for k in ks], np.int32))
    pb.cap, pb.B, pb.image_size, pb.counts_host = cap, B, tuple(size), None
    return pb


def _run_batch(lg, pairs, cap0, cap1):
    size0, size1 = pairs[0][4], pairs[0][5]
    pb0 = _batch([p[0] for p in pairs], [p[1] for p in pairs], cap0, size0)
    pb1 = _batch([p[2] for p in pairs], [p[3] for p in pairs], cap1, size1, dfill=-3.0)
    r = lg.match_batched(pb0, pb1, all_layers=True)
    la, ref0, ref1 = _np(r.la), _np(r.ref0), _np(r.ref1)
    m0, m1, s0, s1 = _np(r.matches0), _np(r.matches1), _np(r.scores0), _np(r.scores1)
    out = []
    for b, p in enumerate(pairs):
        n, m = len(p[0]), len(p[2])
        assert (m0[b, n:] == -1).all(), (b, "padding rows of side 0 matched")
        assert (m1[b, m:] == -1).all(), (b, "padding rows of side 1 matched")
        out.append({"la": la[b, :n + 1, :m + 1], "layers": [(ref0[b, i, :n], ref1[b, i, :m]) for i in range(ref0.shape[1])],
                    "m0": m0[b, :n], "m1": m1[b, :m], "s0": s0[b, :n], "s1": s1[b, :m]})
    return out


def _pairs(seed, counts, din=256, size0=(260, 346), size1=(260, 346)):
    return [lgf64_pair(seed + 17 * b, n, m, din) + (size0, size1) for b, (n, m) in enumerate(counts)]


def _reorder(p):
    d0, d1, k0, k1, s0, s1 = p
    return k0, d0, k1, d1, s0, s1


# ------------------------------------------------------------------ the shipped model, one pair per forward
@pytest.mark.parametrize("n,m", LGF64_PAIRS)
def test_single_pair_vs_float64(oracle, n, m):
    """one pair: lg_gemm_small_kernel + lg_attn16_kernel<16> (the latency forms); n == m stacks the two sides (cross attention
    reads the partner entry through kv_shift), n != m runs them unstacked; count 1, partial and whole 32-key blocks"""
    sd = lgf64_shipped_state_dict(801)
    lg = _model(SHIPPED, sd)
    pair = _reorder(_pairs(8000 + n + 7 * m, [(n, m)])[0])
    _check_pair(f"lgf64.single.{n}x{m}", sd, SHIPPED, pair, _run_single(lg, pair), oracle)


# (case, B, counts, cap0, cap1, model options, paths) -- caps of 1024 stack the sides when equal; 2 stacked pairs run the latency
# attention lg_attn16_kernel<32> (2B entries x 32 key blocks x 4 heads <= 512), 3 and 8 the wide lg_attn_kernel<64, 256>; 8 pairs
# x 2 sides at cap 1024 take the persistent lg_gemm_kernel (>= 256 128x128 tiles), fewer the 64x64-tile lg_gemm_small_kernel
BATCHES = [
    ("stacked_b2", 2, [(1024, 1), (1, 1023)], 1024, 1024, {}),  # attn16<32>, gemm_small
    ("stacked_b3", 3, [(31, 1024), (1023, 31), (200, 500)], 1024, 1024, {}),  # attn_kernel<64,256>, gemm_small
    ("stacked_b8", 8, [(1024, 1023), (1, 31), (31, 1), (100, 90), (257, 300), (64, 65), (33, 32), (300, 212)], 1024, 1024, {}),  # persistent gemm
    ("unstacked_b3", 3, [(640, 1000), (1, 500), (333, 64)], 640, 1000, {}),  # cap0 != cap1: one launch per side, no kv_shift
    ("merge_off_b1", 1, [(300, 280)], 300, 300, dict(merge=False)),  # to_qk and to_v as two launches (gemm_small, attn16<256>)
    ("merge_off_b8", 8, [(400, 350), (50, 60), (500, 400), (1, 2), (90, 130), (31, 33), (200, 1), (64, 64)], 1024, 1024, dict(merge=False)),
    ("fold_off_b1", 1, [(300, 280)], 300, 300, dict(fold=False)),  # out_proj / to_out as their own launches
    ("fold_off_b8", 8, [(400, 350), (50, 60), (500, 400), (1, 2), (90, 130), (31, 33), (200, 1), (64, 64)], 1024, 1024, dict(fold=False)),
]


@pytest.mark.parametrize("case", [b[0] for b in BATCHES])
def test_batch_every_pair_vs_float64(oracle, case):
    _, B, counts, cap0, cap1, opt = next(b for b in BATCHES if b[0] == case)
    sd = lgf64_shipped_state_dict(802)
    lg = _model(SHIPPED, sd, **opt)
    pairs = [_reorder(p) for p in _pairs(8100 + B, counts)]
    for b, got in enumerate(_run_batch(lg, pairs, cap0, cap1)):
        _check_pair(f"lgf64.{case}", sd, SHIPPED, pairs[b], got, oracle)


@pytest.mark.parametrize("size0,size1", [((180, 240), (260, 346)), ((260, 346), (180, 240)), ((480, 270), (260, 346))])
def test_per_side_image_sizes_vs_float64(oracle, size0, size1):
    """each side's positional encoding normalises by ITS image size (lightglue.py:535-538); the keypoints lie inside both sizes"""
    sd = lgf64_shipped_state_dict(803)
    lg = _model(SHIPPED, sd)

    def pair(seed, n, m):
        d0, d1, k0, k1 = lgf64_pair(seed, n, m)
        k0[:, :2] = k0[:, :2] * np.float32(0.5)
        k1[:, :2] = k1[:, :2] * np.float32(0.5)
        return k0, d0, k1, d1, size0, size1

    pairs = [pair(8300 + size0[0], 200, 230), pair(8301, 150, 100)]
    tag = f"lgf64.sizes.{size0[0]}x{size0[1]}_{size1[0]}x{size1[1]}"
    _check_pair(tag, sd, SHIPPED, pairs[0], _run_single(lg, pairs[0]), oracle)
    for b, got in enumerate(_run_batch(lg, pairs, 256, 256)):  # the batch path too, stacked at cap 256
        _check_pair(tag + ".batch", sd, SHIPPED, pairs[b], got, oracle)


@pytest.mark.parametrize("name", list(LGCFG.cases))
def test_other_widths_ragged_batch_vs_float64(oracle, name):
    """every lgcfg configuration as a ragged 3-pair batch: head widths 16 .. 256 (zero-padded lg_attn_kernel<32|64|128|256, 0>,
    EPI_ROPE_ANY), d = 192 / 240 with partial 128-column tiles, lg_ln_gelu_any_kernel (2d != 512), input_proj"""
    c = LGCFG.cases[name]
    conf = _conf(c)
    lg, sd = _lgcfg_model(c)
    counts = [(c["n"], c["m"]), (1, c["m"] // 2 + 1), (c["n"] // 3 + 1, c["m"])]
    cap0, cap1 = max(n for n, _ in counts), max(m for _, m in counts)
    pairs = [_reorder(p) for p in _pairs(c["seed"] * 10, counts, din=c["input_dim"])]
    for b, got in enumerate(_run_batch(lg, pairs, cap0, cap1)):
        _check_pair(f"lgf64.lgcfg.{name}", sd, conf, pairs[b], got, oracle)


def _calibrated(seed, z_mean, pairs):
    """"same scene" assignment head: synth.lightglue_calibration from pair 0's final descriptors (as _calibrate_lightglue)"""
    sd = lgf64_shipped_state_dict(seed)
    k0, d0, k1, d1, s0, s1 = pairs[0]
    r = lg_f64.forward(sd, k0, d0, k1, d1, size0=s0, size1=s1, dtype=torch.float32)
    over, _ = synth.lightglue_calibration(sd, np.concatenate(r["layers"][-1], 0), z_mean=z_mean)
    sd.update(over)
    return sd


@pytest.mark.parametrize("B", [1, 8])
def test_calibrated_same_scene_vs_float64(oracle, B):
    """hundreds of confident matches per pair: the regime where the decisions matter"""
    counts = [(400, 420), (1024, 1024), (300, 200), (31, 33), (250, 260), (128, 128), (1, 40), (200, 190)][:B]
    pairs = [_reorder(p) for p in _pairs(8400, counts)]
    sd = _calibrated(804, 3.0, pairs)
    lg = _model(SHIPPED, sd)
    outs = [_run_single(lg, pairs[0])] if B == 1 else _run_batch(lg, pairs, 1024, 1024)
    for b, got in enumerate(outs):
        ex = _check_pair(f"lgf64.calibrated_b{B}", sd, SHIPPED, pairs[b], got, oracle)
        if b == 0:
            assert int((ex["matches0"] > -1).sum()) >= 200 and ((ex["scores0"] > 0.1) & (ex["scores0"] < 0.9)).sum() >= 50


def test_filter_underflow_edge_vs_float64(oracle):
    """matchability shifted to a mean logit of -50: logsigmoid(z0) + logsigmoid(z1) near -100, so the mutual bests sit around the
    fp32 exp's subnormal band (below -87.3) and its underflow to 0 (-103.97) -- the filter at threshold 0 keeps exactly those
    whose fp32 exp is still > 0"""
    pairs = [_reorder(p) for p in _pairs(8500, [(400, 420), (300, 350)])]
    sd = _calibrated(805, -50.0, pairs)
    lg = _model(SHIPPED, sd)
    outs = [(pairs[0], _run_single(lg, pairs[0]))] + list(zip(pairs, _run_batch(lg, pairs, 420, 420)))
    for pair, got in outs:
        ex = _check_pair("lgf64.underflow_edge", sd, SHIPPED, pair, got, oracle)
        la = ex["log_assignment"][:-1, :-1]
        mx = la.max(1)
        mutual = np.arange(len(mx)) == la.argmax(0)[la.argmax(1)]
        assert (mutual & (mx > -110) & (mx < -85)).sum() >= 20
        assert (mutual & (mx < lg_f64.EXP_F32_EDGE)).any() and (mutual & (mx < -87.3) & (ex["matches0"] > -1)).any()
