"""GPU tests (-m gpu), component: forward values of the extractor losses (csrc/loss.hip, core/loss).

The fused descriptor loss forms every element of the two normalised maps in registers, bit for bit as einx_upsample_normalize /
einx_normalize_map store them (their own parity is tested in test_desc_gpu.py), so the comparison is against the float64
evaluation of the same terms over the materialised maps, under an a-priori bound: n float64 additions of non-negative terms are
within n 2^-53 of the exact sum, relatively (MAE / MSE, n = the terms of the sum); the cosine sums three such accumulations per
pixel of values in [-1, 1], bounded absolutely by 3 n 2^-53 per pixel.  Counts are compared exactly."""
from importlib import import_module

import numpy as np
import pytest
import torch

import loss_ref as R
from helpers import synth, synth_raw_events
from gpu_support import DEV, _eim_model, _np, _t, pkg

pytestmark = pytest.mark.gpu

N = pkg.native
L = pkg.core.loss
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------ inputs
def _masks(B, H, W, seed):
    """name -> mask [B,1,H,W] on the device (None: no mask).  The float weights have 24 random bits, so their float64 sums are
    exact in any order and the counts compare exactly."""
    u8 = (synth.uniform01(seed, (B, 1, H, W)) > 0.4).astype(np.uint8)
    zero = u8.copy()
    zero[B - 1] = 0  # one image of the batch all zero: count 0, a NaN pair value
    return {"u8": _t(u8), "bool": _t(u8.astype(bool)), "f32": _t(synth.uniform01(seed + 1, (B, 1, H, W))),
            "ones": _t(np.ones((B, 1, H, W), np.uint8)), "none": None, "zero_image": _t(zero)}


def _weights(mask, B, H, W):
    if mask is None:
        return torch.ones((B, H, W), dtype=torch.float64, device=DEV)
    return (mask.reshape(B, H, W) != 0).double() if mask.dtype in (torch.bool, torch.uint8) else mask.reshape(B, H, W).double()


def _exact(a, b, w, mode):
    """float64 (sums [B], counts [B]) of the terms over the materialised maps a, b [B,D,H,W] (float32), on the device"""
    D = a.shape[1]
    if mode == "cos":
        ad, bd = a.double(), b.double()
        cos = (ad * bd).sum(1) / ((ad * ad).sum(1).sqrt().clamp_min(1e-8) * (bd * bd).sum(1).sqrt().clamp_min(1e-8))
        return (w * cos).sum((1, 2)), w.sum((1, 2))
    d = a - b
    t = (d * d).double() if mode == "mse" else d.abs().double()
    return (t * w[:, None]).sum((1, 2, 3)), D * w.sum((1, 2))


def _check(got, sums, counts, n_image, mode, hw, tag):
    """per image and pooled: counts exactly, sums under the a-priori bound"""
    got, sums, counts = _np(got), _np(sums), _np(counts)
    assert np.array_equal(got[:, 1], counts), f"{tag}: counts {got[:, 1]} != {counts}"
    B = got.shape[0]
    for g, e, n in list(zip(got[:, 0], sums, [n_image] * B)) + [(got[:, 0].sum(), sums.sum(), n_image * B)]:
        bound = 3 * n * U * hw if mode == "cos" else n * U * abs(e)
        print(f"{tag} {mode}: |got - exact| = {abs(g - e):.3e}, bound {bound:.3e}, exact {e:.17g}")
        assert abs(g - e) <= bound, tag


def _zero_image_contract(got, B):
    s, c = _np(got)[:, 0], _np(got)[:, 1]
    assert c[B - 1] == 0 and s[B - 1] == 0
    with np.errstate(invalid="ignore"):
        assert np.isnan(s[B - 1] / c[B - 1])  # the pair value
    if B > 1:
        assert np.isfinite(s.sum() / c.sum())  # the pooled value


CELL8 = {
    # name: B, D, hc, wc, H, W (padded = 8 hc x 8 wc), fused?
    "four_pads": (3, 256, 7, 9, 52, 70, True),          # all four pads nonzero
    "two_column_blocks": (2, 64, 3, 44, 20, 346, True),  # 346 columns = two blocks of 192
    "fallback": (1, 32, 2, 50, 13, 400, False),          # W > 384: the maps are materialised
}


@pytest.fixture(scope="module")
def cell8_maps():
    """per shape: raw maps, geometry, the two materialised maps (written once by einx_upsample_normalize, shared, left unchanged)"""
    out = {}
    for i, (name, (B, D, hc, wc, H, W, fused)) in enumerate(CELL8.items()):
        pads = N.padder_pads(H, W, 8)
        padded = (H + pads[2] + pads[3], W + pads[0] + pads[1])
        assert padded == (8 * hc, 8 * wc)
        ra, rb = _t(synth.normalish(900 + i, (B, D, hc, wc))), _t(synth.normalish(950 + i, (B, D, hc, wc)))
        sa, sb = 1.0, 1.25
        out[name] = dict(ra=ra, rb=rb, sa=sa, sb=sb, pads=pads, padded=padded, a=N.upsample_normalize(ra, padded, pads, sa),
                         b=N.upsample_normalize(rb, padded, pads, sb), masks=_masks(B, H, W, 40 + i))
    return out


@pytest.mark.parametrize("mode", ["mae", "mse", "cos"])
@pytest.mark.parametrize("shape", list(CELL8))
def test_desc_loss_cell8_against_float64_over_the_materialised_maps(cell8_maps, shape, mode):
    B, D, hc, wc, H, W, fused = CELL8[shape]
    m = cell8_maps[shape]
    if shape == "four_pads":
        assert all(p > 0 for p in m["pads"])
    nws = N.lib().einx_desc_loss_ws_bytes(B, D, hc, wc, m["padded"][0], m["padded"][1], m["pads"][2], m["pads"][0], H, W, 8)
    assert (nws < 2 * B * D * H * W * 4) == fused  # the path: the fused form never holds a map
    for name, mask in m["masks"].items():
        got = N.desc_loss(m["ra"], m["sa"], m["rb"], m["sb"], m["padded"], m["pads"], 8, mask, mode)
        sums, counts = _exact(m["a"], m["b"], _weights(mask, B, H, W), mode)
        _check(got, sums, counts, D * H * W, mode, H * W, f"{shape}/{name}")
        if name == "zero_image":
            _zero_image_contract(got, B)
        if name == "none":
            assert np.array_equal(_np(got)[:, 1], np.full(B, float(H * W if mode == "cos" else D * H * W)))


@pytest.mark.parametrize("mode", ["mae", "mse", "cos"])
def test_desc_loss_cell1_against_float64_over_the_materialised_maps(mode):
    B, D, Hp, Wp, H, W = 2, 128, 24, 40, 20, 37
    pads = N.padder_pads(H, W, 8)
    assert (H + pads[2] + pads[3], W + pads[0] + pads[1]) == (Hp, Wp)
    w0, w1, h0, h1 = pads
    ra, rb = _t(synth.normalish(970, (B, D, Hp, Wp))), _t(synth.normalish(971, (B, D, Hp, Wp)))
    a = N.normalize_map(ra, 1.0)[:, :, h0:Hp - h1, w0:Wp - w1].contiguous()
    b = N.normalize_map(rb, 1.41421)[:, :, h0:Hp - h1, w0:Wp - w1].contiguous()
    for name, mask in _masks(B, H, W, 60).items():
        got = N.desc_loss(ra, 1.0, rb, 1.41421, (Hp, Wp), pads, 1, mask, mode)
        sums, counts = _exact(a, b, _weights(mask, B, H, W), mode)
        _check(got, sums, counts, D * H * W, mode, H * W, f"cell1/{name}")
        if name == "zero_image":
            _zero_image_contract(got, B)


# ------------------------------------------------------------------------------------------ einx_map_loss / einx_logits_loss
def _check_np(got, sums, counts, n_image, tag):
    got = _np(got)
    assert np.array_equal(got[:, 1], counts), f"{tag}: counts {got[:, 1]} != {counts}"
    for g, e, n in list(zip(got[:, 0], sums, [n_image] * len(sums))) + [(got[:, 0].sum(), sums.sum(), n_image * len(sums))]:
        print(f"{tag}: |got - exact| = {abs(g - e):.3e}, bound {n * U * abs(e):.3e}, exact {e:.17g}")
        assert abs(g - e) <= n * U * abs(e), tag


@pytest.mark.parametrize("mode", ["sq", "abs"])
def test_map_loss_scores_and_features(mode):
    B, H, W = 3, 52, 70
    x, y = synth.uniform01(301, (B, 1, H, W)), synth.uniform01(302, (B, 1, H, W))
    for name, mask in _masks(B, H, W, 70).items():
        s, c = R.map_sums(x, y, None if mask is None else _np(mask), mode)
        _check_np(N.map_loss(_t(x), _t(y), mask, mode), s, c, H * W, f"scores/{name}")
    x, y = synth.normalish(303, (B, 128, 7, 9)), synth.normalish(304, (B, 128, 7, 9))  # C = 128, P = 63
    bcast, full = synth.uniform01(305, (B, 1, 7, 9)) > 0.5, synth.uniform01(306, (B, 128, 7, 9))
    for name, mask in (("none", None), ("broadcast", bcast), ("full", full)):
        s, c = R.map_sums(x, y, mask, mode)
        _check_np(N.map_loss(_t(x), _t(y), None if mask is None else _t(mask), mode), s, c, 128 * 63, f"features/{name}")


def test_map_loss_bce_clamps_the_logarithms_at_minus_100():
    B, H, W = 3, 52, 70
    p = synth.uniform(311, (B, 1, H, W), 0.001, 0.999)
    p[:, 0, 0, :6] = np.array([0.0, 0.0, 1.0, 1.0, 1e-45, 1e-45], np.float32)  # log 0 and log(1 - 1) on both sides of the target
    g = np.where(synth.uniform01(312, (B, 1, H, W)) > 0.8, np.float32(0.7), np.float32(0.0)).astype(np.float32)
    g[:, 0, 0, :6] = np.array([1.0, 0.0, 1.0, 0.0, 1.0, 0.0], np.float32)
    assert np.float32(1e-45) > 0
    s, c = R.map_sums(p, g, None, "bce")
    assert np.all(R.terms(p, g, "bce")[:, 0, 0, [0, 3, 4]] == 100.0) and np.all(R.terms(p, g, "bce")[:, 0, 0, [1, 2]] == 0.0)
    _check_np(N.map_loss(_t(p), _t(g), None, "bce"), s, c, H * W, "bce")


def test_map_loss_cosine_of_existing_maps():
    B, D, H, W = 2, 16, 20, 29
    x, y = R.unit_map(321, (B, D, H, W)), R.unit_map(322, (B, D, H, W), 1.3)
    for name, mask in _masks(B, H, W, 80).items():
        s, c = R.cos_sums(x, y, None if mask is None else _np(mask))
        got = _np(N.map_loss(_t(x), _t(y), mask, "cos"))
        assert np.array_equal(got[:, 1], c)
        assert np.all(np.abs(got[:, 0] - s) <= 3 * D * H * W * U * H * W), name


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("crop", [False, True])
def test_logits_loss_pixel_shuffle_crop_and_mask(masked, crop):
    B, hc, wc, H, W = 3, 7, 9, 52, 70
    x, y = synth.uniform(331, (B, 65, hc, wc), -4, 4), synth.uniform(332, (B, 65, hc, wc), -4, 4)
    pads = N.padder_pads(H, W, 8)
    Hm, Wm = (H, W) if crop else (8 * hc, 8 * wc)
    for name, mask in _masks(B, Hm, Wm, 90).items():
        if (mask is not None) != masked:
            continue
        s, c = R.logits_sums(x, y, 8, pads if crop else None, None if mask is None else _np(mask))
        assert np.all(c == Hm * Wm)  # every element of the window, masked or not
        got = N.logits_loss(_t(x), _t(y), 8, (pads[2], pads[0], H, W) if crop else None, mask)
        _check_np(got, s, c, Hm * Wm, f"logits/{name}")


# ------------------------------------------------------------------------------------------ modules on the extractors' dicts
H0, W0, B0 = 52, 70, 3


@pytest.fixture(scope="module")
def sp_forward():
    _, model, _ = _eim_model("SP_MNN", seed=11)
    ev, mask = synth.synth_events(31, B0, 5, H0, W0)
    img = synth.synth_image(31, B0, H0, W0)
    ef, imf, _ = model(_t(ev), _t(img), _t(mask))
    return ef, imf, _t(mask)


def _value(mod, sums_counts_f):
    s, c, f = sums_counts_f
    with np.errstate(invalid="ignore", divide="ignore"):
        return mod.weight * f(s.sum() / c.sum())


def test_descriptors_loss_on_feats_dicts_is_fused_and_lazy_entries_stay_lazy(sp_forward):
    ef, imf, mask = sp_forward
    assert "normalized_descriptors" in ef.lazy_keys() and "normalized_descriptors" in imf.lazy_keys()
    mods = {("mae", True): L.DescriptorsLoss(1.0, mode="mae"), ("mse", True): L.DescriptorsLoss(2.0, mode="mse"),
            ("cosine_similarity", False): L.DescriptorsLoss(0.5, mode="cosine_similarity"), ("mae", False): L.DescriptorsLoss(1.0, mode="mae", use_mask=False)}
    fused = {}
    for (mode, use), mod in mods.items():
        loss, info = mod(ef, imf, mask if use else None)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == "cuda" and list(info) == ["extractor_descriptor_loss"]
        assert info["extractor_descriptor_loss"] == loss.item()
        fused[(mode, use)] = (loss.item(), _np(mod._sums(ef, imf, mask if use else None)), _np(mod.pair_values(ef, imf, mask if use else None)))
    # the refusals of the table, before anything is resolved
    with pytest.raises(TypeError, match="missing 1 required positional argument: 'target'"):
        L.DescriptorsLoss(1.0, mode="mse")(ef, imf, None)
    with pytest.raises(IndexError, match="does not match the shape of the indexed tensor"):
        L.DescriptorsLoss(1.0, mode="cosine_similarity")(ef, imf, mask)
    with pytest.raises(NotImplementedError, match="triplet"):
        L.DescriptorsLoss(1.0, mode="triplet")(ef, imf, mask)
    assert "normalized_descriptors" in ef.lazy_keys() and "normalized_descriptors" in imf.lazy_keys()
    # the dict's tensors through the float64 restatement, and the same call after resolving the entry (einx_map_loss)
    a, b = ef["normalized_descriptors"], imf["normalized_descriptors"]
    assert "normalized_descriptors" not in ef.lazy_keys() and a.shape == (B0, 256, H0, W0)
    n = 256 * H0 * W0
    for (mode, use), mod in mods.items():
        value, sc, pairs = fused[(mode, use)]
        s, c, f = R.descriptors_loss(_np(a), _np(b), _np(mask) if use else None, mode)
        assert np.array_equal(sc[:, 1], c)
        bound = 3 * n * U * H0 * W0 if mode == "cosine_similarity" else n * U * np.abs(s)
        assert np.all(np.abs(sc[:, 0] - s) <= bound), (mode, sc[:, 0], s)
        exp = _value(mod, (s, c, f))
        assert abs(value - exp) <= np.spacing(np.float32(abs(exp))), (mode, value, exp)  # float32(float64 value)
        assert np.allclose(pairs, mod.weight * f(s / c), rtol=1e-12, atol=0)
        again = _np(mod._sums(ef, imf, mask if use else None))  # resolved now: the given tensors are reduced
        assert np.array_equal(again[:, 1], c) and np.all(np.abs(again[:, 0] - s) <= bound)
        loss2, _ = mod(ef, imf, mask if use else None)
        assert abs(loss2.item() - exp) <= np.spacing(np.float32(abs(exp)))
    # plain dicts of tensors, raw / coarse descriptors
    plain = L.DescriptorsLoss(1.0, mode="mae")({"normalized_descriptors": a}, {"normalized_descriptors": b}, mask)[0].item()
    assert abs(plain - _value(mods[("mae", True)], R.descriptors_loss(_np(a), _np(b), _np(mask), "mae"))) <= np.spacing(np.float32(plain))
    for desc_type, key in (("raw", "raw_descriptors"), ("coarse", "coarse_descriptors")):
        mod = L.DescriptorsLoss(1.0, desc_type=desc_type, mode="mae", use_mask=False)
        exp = _value(mod, R.descriptors_loss(_np(ef[key]), _np(imf[key]), None, "mae"))
        assert abs(mod(ef, imf, mask)[0].item() - exp) <= np.spacing(np.float32(exp))


@pytest.mark.parametrize("mode", ["mse", "mae", "mse-whole", "bce"])
def test_score_loss_on_feats_dicts(sp_forward, mode):
    ef, imf, mask = sp_forward
    pred, gt = {"score": ef["score"].clone()}, {"score": imf["score"].clone()}
    before = _np(gt["score"]).copy()
    mod = L.ScoreLoss(1.5, mode)
    loss, info = mod(pred, gt, mask)
    s, c, after = R.score_loss(_np(pred["score"]), before.copy(), _np(mask), mode)
    exp = R.value(s, c, 1.5)
    assert list(info) == ["extractor_keypoints_loss"] and info["extractor_keypoints_loss"] == loss.item()
    assert abs(loss.item() - exp) <= np.spacing(np.float32(abs(exp))), (mode, loss.item(), exp)
    assert np.array_equal(_np(gt["score"]), after)  # mse-whole edits the ground truth in place; the other modes leave it alone
    assert (mode == "mse-whole") == (not np.array_equal(after, before))
    if mode != "mse-whole":
        sc = _np(mod._sums(pred, gt, mask))
        assert np.array_equal(sc[:, 1], c) and np.all(np.abs(sc[:, 0] - s) <= H0 * W0 * U * np.abs(s))


def test_logits_and_feature_loss_on_feats_dicts(sp_forward):
    ef, imf, mask = sp_forward
    padder = import_module(pkg.__name__ + ".core.modules.utils.util").Padder((H0, W0), 8)
    s, c = R.logits_sums(_np(ef["logits"]), _np(imf["logits"]), 8, padder.padding_size, _np(mask))
    loss, info = L.LogitsLoss(2.0, "mse", 8)(ef, imf, mask, padder=padder)
    exp = R.value(s, c, 2.0)
    assert list(info) == ["extractor_keypoints_loss"] and abs(loss.item() - exp) <= np.spacing(np.float32(exp))
    s, c = R.map_sums(_np(ef["backbone_feats"]), _np(imf["backbone_feats"]), None, "sq")
    loss, info = L.FeatureLoss(1.0, "mse")(ef, imf)
    assert list(info) == ["feature_loss"] and abs(loss.item() - R.value(s, c)) <= np.spacing(np.float32(R.value(s, c)))


def test_descriptors_loss_fused_on_the_cell1_family():
    _, model, _ = _eim_model("SiLK_MNN", seed=12)
    B = 2
    ev, mask = synth.synth_events(32, B, 5, H0, W0)
    ef, imf, _ = model(_t(ev), _t(synth.synth_image(32, B, H0, W0)), _t(mask))
    mod = L.DescriptorsLoss(1.0, mode="mae")
    assert ef._batched.cell == 1
    fused = _np(mod._sums(ef, imf, _t(mask)))
    assert "normalized_descriptors" in ef.lazy_keys() and "normalized_descriptors" in imf.lazy_keys()
    a, b = ef["normalized_descriptors"], imf["normalized_descriptors"]
    s, c, _ = R.descriptors_loss(_np(a), _np(b), mask, "mae")
    assert np.array_equal(fused[:, 1], c) and np.all(np.abs(fused[:, 0] - s) <= a[0].numel() * U * np.abs(s))


# ------------------------------------------------------------------------------------------ determinism, graphs, workspaces
def _ops():
    """name -> a call of each op / path with fixed inputs, returning its [B,2] output"""
    ops = {}
    for i, (name, (B, D, hc, wc, H, W, fused)) in enumerate(CELL8.items()):
        pads = N.padder_pads(H, W, 8)
        padded = (8 * hc, 8 * wc)
        ra, rb = _t(synth.normalish(900 + i, (B, D, hc, wc))), _t(synth.normalish(950 + i, (B, D, hc, wc)))
        mask = _masks(B, H, W, 40 + i)["f32"]
        for mode in ("mae", "cos"):
            ops[f"desc8/{name}/{mode}"] = lambda ra=ra, rb=rb, padded=padded, pads=pads, mask=mask, mode=mode: N.desc_loss(ra, 1.0, rb, 1.25, padded, pads, 8, mask, mode)
    r1a, r1b = _t(synth.normalish(970, (2, 128, 24, 40))), _t(synth.normalish(971, (2, 128, 24, 40)))
    m1 = _masks(2, 20, 37, 60)["u8"]
    ops["desc1/mse"] = lambda: N.desc_loss(r1a, 1.0, r1b, 1.4, (24, 40), N.padder_pads(20, 37, 8), 1, m1, "mse")
    x, y = _t(synth.uniform(311, (3, 1, 52, 70), 0.001, 0.999)), _t(synth.uniform01(312, (3, 1, 52, 70)))
    mb, mf = _masks(3, 52, 70, 70)["bool"], _masks(3, 52, 70, 90)["f32"]
    ops["map/bce"] = lambda: N.map_loss(x, y, None, "bce")
    ops["map/sq"] = lambda: N.map_loss(x, y, mb, "sq")
    lx, ly = _t(synth.uniform(331, (3, 65, 7, 9), -4, 4)), _t(synth.uniform(332, (3, 65, 7, 9), -4, 4))
    ops["logits"] = lambda: N.logits_loss(lx, ly, 8, (2, 1, 52, 70), mf)
    return ops


def test_outputs_are_bit_equal_run_to_run_and_on_graph_replay():
    for name, op in _ops().items():
        first = op().clone()
        assert np.array_equal(_np(op()), _np(first), equal_nan=True), name
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = op()
        for _ in range(2):
            out.fill_(-1.0)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(_np(out), _np(first), equal_nan=True), f"{name}: graph replay differs"


GUARD, PATTERN = 4096, 0xA5


def test_nothing_writes_past_the_workspace_query_and_a_short_workspace_is_refused(monkeypatch):
    made = []

    def guarded(nbytes, device):
        nbytes = int(nbytes)
        buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=device)
        buf[nbytes:] = PATTERN
        made.append((nbytes, buf[nbytes:]))
        return buf[:nbytes]

    monkeypatch.setattr(N, "_workspace", guarded)
    ops = _ops()
    for op in ops.values():
        op()
    torch.cuda.synchronize()
    assert len(made) == len(ops)
    for nbytes, tail in made:
        assert nbytes > 0 and nbytes % 256 == 0
        assert int((tail != PATTERN).sum()) == 0, f"guard bytes behind a loss workspace of {nbytes} bytes were overwritten"
    # one region less than the query: refused on the host, nothing launched
    lib, P = N.lib(), N._ptr
    out = torch.full((2, 2), -1.0, dtype=torch.float64, device=DEV)
    B, D, hc, wc, H, W, _ = CELL8["two_column_blocks"]
    ra = _t(synth.normalish(901, (B, D, hc, wc)))
    nws = lib.einx_desc_loss_ws_bytes(B, D, hc, wc, 24, 352, 2, 3, H, W, 8)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    args = (P(ra), 1.0, P(ra), 1.0, B, D, hc, wc, 24, 352, 2, 3, H, W, 8, None, 0, 0, P(out), P(ws))
    assert lib.einx_desc_loss(*args, nws - 256, N._stream(ra)) != 0 and b"workspace smaller" in lib.einx_last_error()
    x = _t(synth.uniform01(1, (2, 1, 600)))
    nws = lib.einx_map_loss_ws_bytes(2, 600)
    assert lib.einx_map_loss(P(x), P(x), 2, 1, 600, None, 0, 0, 0, P(out), P(ws), nws - 256, N._stream(x)) != 0
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    nws = lib.einx_desc_loss_ws_bytes(B, D, hc, wc, 24, 352, 2, 3, H, W, 8)
    assert lib.einx_desc_loss(*args, nws, N._stream(ra)) == 0
    torch.cuda.synchronize()
    assert _np(out)[0, 0] == 0.0 and _np(out)[0, 1] == D * H * W  # a map against itself


# ------------------------------------------------------------------------------------------ the evaluation harness
@pytest.fixture(scope="module")
def loss_batches():
    """(model, the losses of train_stage1.yaml, two batches of raw events and images at B0 x H0 x W0)"""
    import json
    import os
    from helpers import GOLDEN
    with open(os.path.join(GOLDEN, "train_loss_configs.json")) as f:
        cfg = json.load(f)["train_stage1.yaml"]
    _, model, _ = _eim_model("SP_MNN", seed=11)
    losses = L.build_losses(pkg.configs.to_attr(cfg))
    batches = []
    for k in range(2):
        evs = [synth_raw_events(dict(seed=500 + 10 * k + b, n=300 if (k, b) == (1, 2) else 2500, H=H0, W=W0, bins=5, frac=False, pneg=False))
               for b in range(B0)]
        batches.append((evs, synth.synth_image(70 + k, B0, H0, W0)))
    return model, losses, batches


def test_same_time_evaluator_reports_the_validation_losses(loss_batches):
    model, losses, batches = loss_batches
    kp, ds = losses["keypoints_loss"], losses["descriptors_loss"]
    assert (kp.mode, ds.mode, ds.desc_type) == ("mse", "mae", "normalized")
    with_losses = pkg.SameTimeEvaluator(model, bins=5, resolution=(W0, H0), losses=losses)
    plain = pkg.SameTimeEvaluator(model, bins=5, resolution=(W0, H0))
    per = {n: [] for n in ("extractor_keypoints_loss", "extractor_descriptor_loss", "loss")}
    for evs, img in batches:
        rows1, (ef, imf, _) = with_losses.step(evs, _t(img.copy()))
        assert "normalized_descriptors" in ef.lazy_keys() and "normalized_descriptors" in imf.lazy_keys()  # the fused path
        mask = with_losses.last_inputs[1]
        assert mask.shape == (B0, 1, H0, W0)
        rows0, _ = plain.step(evs, _t(img.copy()))
        assert torch.equal(rows0, rows1)  # the rows `step` returns are unchanged
        a, b = ef["normalized_descriptors"], imf["normalized_descriptors"]
        for p in range(B0):  # the modules, one pair at a time, on the same float32 tensors
            one = slice(p, p + 1)
            v_kp = float(kp.pair_values({"score": ef["score"][one]}, {"score": imf["score"][one]}, mask[one]))
            v_ds = float(ds.pair_values({"normalized_descriptors": a[one].contiguous()}, {"normalized_descriptors": b[one].contiguous()}, mask[one]))
            per["extractor_keypoints_loss"].append(v_kp)
            per["extractor_descriptor_loss"].append(v_ds)
            per["loss"].append(v_kp + v_ds)
    res = with_losses.result()
    assert set(plain.result()) == set(plain.names)  # losses=None: exactly the parent's keys
    assert set(res) == set(plain.names) | set(per)
    for k in plain.names:
        assert res[k] == plain.result()[k] or (np.isnan(res[k]) and np.isnan(plain.result()[k]))
    for k, v in per.items():
        v = np.array(v, np.float64)
        assert len(v) == 2 * B0 and np.isfinite(v).sum() >= B0
        exp = np.mean(v[np.isfinite(v)])
        print(k, res[k], exp, v.tolist())
        assert abs(res[k] - exp) <= 1e-12 * abs(exp), k
    # run() enqueues the same two ops per batch
    runner = pkg.SameTimeEvaluator(model, bins=5, resolution=(W0, H0), losses=losses)
    assert len(list(runner.run([(evs, _t(img.copy())) for evs, img in batches]))) == 2
    r2 = runner.result()
    for k in per:
        assert r2[k] == res[k], k
    # an entry without a per-pair form (core.loss.Pass) is skipped by the means
    half = pkg.SameTimeEvaluator(model, bins=5, resolution=(W0, H0), losses={"keypoints_loss": L.Pass(), "descriptors_loss": ds})
    half.step(batches[0][0], _t(batches[0][1].copy()))
    r3 = half.result()
    assert np.isnan(r3["extractor_keypoints_loss"]) and np.isnan(r3["loss"]) and np.isfinite(r3["extractor_descriptor_loss"])
    with pytest.raises(ValueError, match="takes no losses"):
        pkg.DifferentTimeEvaluator(model, bins=5, resolution=(W0, H0), losses=losses)


def test_same_time_evaluator_with_homography_and_losses_step_equals_run(loss_batches):
    """he_thresh and losses together, a homography per batch: `step` and `run` give the same result() key for key, and the loss keys
    are those of an evaluator that accounts the losses alone"""
    model, losses, batches = loss_batches
    hom = _t(np.tile(np.array([[1.01, 0.01, -2.0], [-0.01, 0.99, 1.5], [1e-5, -1e-5, 1.0]], np.float32), (B0, 1, 1)))
    make = lambda **kw: pkg.SameTimeEvaluator(model, bins=5, resolution=(W0, H0), **kw)  # noqa: E731
    stepped, streamed, alone = make(he_thresh=(3, 5, 10), losses=losses), make(he_thresh=(3, 5, 10), losses=losses), make(losses=losses)
    for evs, img in batches:
        stepped.step(evs, _t(img.copy()), hom)
        alone.step(evs, _t(img.copy()))
    assert len(list(streamed.run([(evs, _t(img.copy()), hom) for evs, img in batches]))) == 2
    a, b, c = stepped.result(), streamed.result(), alone.result()
    loss_keys = ("extractor_keypoints_loss", "extractor_descriptor_loss", "loss")
    assert list(a) == list(b) and set(a) == set(stepped.names) | {k for k in a if k.startswith("HE")} | set(loss_keys) and len(a) == len(stepped.names) + 8 + 3
    for k in a:
        assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])
    for k in loss_keys:
        assert a[k] == c[k] or (a[k] != a[k] and c[k] != c[k]), (k, a[k], c[k])
    assert np.isfinite(a["loss"])
