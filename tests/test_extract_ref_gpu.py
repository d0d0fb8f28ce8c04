"""GPU tests (-m gpu), components: detect (K3, the score map) and desc.  The kernels between the convolution stack and the matcher
against tests/extract_ref.py -- the reference's steps as the torch calls it makes, on the CPU in float64 -- at the smallest shapes
that reach every path.  tests/test_extract_ref_cpu.py holds that statement against the reference's own outputs and runs the C
oracle and torch's float32 operations through every input and bound used here.

Index-only results compare exactly: zero patterns, pixel-shuffle placement, gathered pixels, counts.  Values compare under bounds
derived from the kernels' operation sequences in units of U = 2^-24 (the docstrings of extract_ref.prob_bound, normalized_bound,
sample_value_bound, upsample_value_bound); none is fitted to a run.  Every comparison prints error, bound and their ratio (-s)."""
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import extract_ref as er
from gpu_support import CONV, DEV, _build, _np, _t, pkg

pytestmark = pytest.mark.gpu

N = pkg.native
dd = import_module(pkg.__name__ + ".core.modules.utils.descriptor_util")
EX = import_module(pkg.__name__ + "._extract")


def _nz(t):
    return (t != 0).cpu().numpy()


# ------------------------------------------------------------------ score map: N.score_map
@pytest.mark.parametrize("dilate", [False, True])
@pytest.mark.parametrize("sid,C,hc,wc,pads", er.SCORE_SHAPES, ids=[s[0] for s in er.SCORE_SHAPES])
def test_score_map_vs_statement(sid, C, hc, wc, pads, dilate):
    """per mask dtype (bool, uint8 {0,1} and {0,255}, int64, float32 1.0 and 0.5, float64), pattern (one image each: empty, full,
    corners, edges, 2 % random) and border (0, 1, 4): the zero pattern of the whole padded map is the statement's (a bool mask
    zero-padded, every other dtype replicate-padded: Padder.pad), every kept pixel is the bit pattern of the pixel-shuffled
    probability of the same call, that probability is inside prob_bound of the float64 value, and an all-ones mask that is not
    bool gives the bits of mask=None."""
    Hp, Wp, H, W = er.score_geometry(C, hc, wc, pads)
    logits = er.score_logits(C, hc, wc)
    lt = _t(logits)
    p64 = er.probability(logits)
    base = er.pattern_batch(H, W)
    full = er.MASK_PATTERNS.index("full")
    none = {}
    for border in er.BORDERS:
        prob0, score0 = N.score_map(lt, None, pads, dilate=dilate, border=border)
        none[border] = score0.cpu()
        if border == 0:
            er.within(f"score_map.prob[{sid}]", prob0.cpu(), p64, er.prob_bound(logits, p64))
            shuf = (F.pixel_shuffle(prob0[:, :-1], 8) if C == 65 else prob0).cpu()
            assert torch.equal(shuf, none[0]), "pixel-shuffle placement"
            assert bool((shuf > 0).all())
            prob_none = prob0.cpu()
    for dname in er.MASK_DTYPES:
        mask = er.typed_mask(base, dname)
        for border in er.BORDERS:
            prob, score = N.score_map(lt, mask.to(DEV), pads, dilate=dilate, border=border)
            prob, score = prob.cpu(), score.cpu()
            _, s64, _ = er.score_map(logits, mask, pads, dilate, border)
            assert np.array_equal(_nz(score), _nz(s64)), (dname, border, "zero pattern")
            kept = score != 0
            assert torch.equal(score[kept], shuf[kept]), (dname, border, "kept pixels")
            assert torch.equal(prob, prob_none if C == 65 else score), (dname, border, "probability")
            if dname != "bool":
                assert torch.equal(score[full], none[border][full]), (dname, border, "an all-ones mask is no mask")


def test_signed_and_denormal_float_masks_read_as_non_zero():
    """the stated departure: a float mask's non-zero pixels are visible, where the reference's float32 box filter
    loses 1e-45 and cancels +1 against -1; 0.5 and 1.0 agree.  tests/test_extract_ref_cpu.py asserts the facts about this input."""
    sid, C, hc, wc, pads = er.SCORE_SHAPES[0]
    Hp, Wp, H, W = er.score_geometry(C, hc, wc, pads)
    m, _ = er.special_float_mask(H, W)
    logits = er.score_logits(C, hc, wc, B=1)
    _, score = N.score_map(_t(logits), m.to(DEV), pads, dilate=True, border=0)
    ours = er.visible(er.nonzero_mask(m), pads, True)
    ref = er.visible(m, pads, True)
    assert np.array_equal(_nz(score), ours.numpy()) and not np.array_equal(ours.numpy(), ref.numpy())


def test_score_map_c_abi_entries():
    """einx_score_map keeps the bool rule (zero padding) bit for bit; einx_score_map_pad with EINX_MASK_PAD_REPLICATE is the other
    rule on the same bytes; any other mask_pad is EINX_ERR_ARG before a launch"""
    sid, C, hc, wc, pads = er.SCORE_SHAPES[0]
    Hp, Wp, H, W = er.score_geometry(C, hc, wc, pads)
    w0, _, h0, _ = pads
    logits = _t(er.score_logits(C, hc, wc))
    B = logits.shape[0]
    base = torch.from_numpy(er.pattern_batch(H, W))
    m8 = base.to(DEV).view(torch.uint8)
    L, P = N.lib(), N._ptr
    out = {}
    for name, call in (("zero", lambda p, s: L.einx_score_map(P(logits), B, C, hc, wc, P(m8), H, W, h0, w0, 1, 0, P(p), P(s), N._stream(logits))),
                       ("replicate", lambda p, s: L.einx_score_map_pad(P(logits), B, C, hc, wc, P(m8), N.MASK_PAD_REPLICATE, H, W, h0, w0, 1, 0, P(p), P(s),
                                                                       N._stream(logits)))):
        prob, score = torch.empty_like(logits), torch.empty((B, 1, Hp, Wp), dtype=torch.float32, device=DEV)
        assert call(prob, score) == 0
        out[name] = score.cpu()
    assert torch.equal(out["zero"], N.score_map(logits, base.to(DEV), pads, dilate=True, border=0)[1].cpu())
    assert torch.equal(out["replicate"], N.score_map(logits, base.to(torch.uint8).to(DEV), pads, dilate=True, border=0)[1].cpu())
    assert not torch.equal(out["zero"], out["replicate"])
    prob, score = torch.empty_like(logits), torch.empty((B, 1, Hp, Wp), dtype=torch.float32, device=DEV)
    assert L.einx_score_map_pad(P(logits), B, C, hc, wc, P(m8), 2, H, W, h0, w0, 1, 0, P(prob), P(score), N._stream(logits)) == -1


# ------------------------------------------------------------------ score map: through ExtractorEngine (einx_extract and layer by layer)
@pytest.fixture(scope="module")
def small_model():
    model, sd = _build(CONV.cases["vgg5_small"], CONV)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    return model


@pytest.mark.parametrize("use_handle", [True, False], ids=["einx_extract", "op_level"])
@pytest.mark.parametrize("side", ["event", "image"])
def test_engine_score_map_vs_statement(small_model, monkeypatch, side, use_handle):
    """the same properties on ExtractorEngine's padded score map (37x45 images, pads (1,2,1,2)), one einx_extract call per network
    and layer by layer through the op-level entries: the pad rule has to arrive through both"""
    monkeypatch.setattr(EX.ExtractorEngine, "use_handle", use_handle)
    c, sd, kind, sec, x, m, pads = er.forward_case(CONV, side)
    ext = getattr(small_model, f"{side}_extractor").extractor
    dilate = kind == "vgg"
    assert ext.dilate_mask == dilate
    H, W = x.shape[-2:]
    B = len(er.MASK_PATTERNS)
    x5 = np.ascontiguousarray(np.repeat(x[:1], B, 0))
    base = er.pattern_batch(H, W)
    full = er.MASK_PATTERNS.index("full")
    old = ext.remove_borders
    try:
        for border in er.BORDERS:
            ext.remove_borders = border
            bf0 = ext.extract_batched(_t(x5.copy()), None)
            shuf = F.pixel_shuffle(bf0.prob[:, :-1], 8).cpu()
            if border == 0:
                p64 = er.probability(_np(bf0.logits))
                assert float((bf0.logits.double() - bf0.logits.double().amax(1, keepdim=True)).abs().max()) < 60
                er.within(f"engine.prob[{side},{use_handle}]", bf0.prob.cpu(), p64, er.prob_bound(_np(bf0.logits), p64))
            score_none = bf0.score.cpu()
            for dname in ("bool", "u8_1", "u8_255", "i64", "f32_half", "f64"):
                mask = er.typed_mask(base, dname)
                bf = ext.extract_batched(_t(x5.copy()), mask.to(DEV))
                assert tuple(bf.pads) == tuple(pads)
                score = bf.score.cpu()
                exp = er.apply_mask_border(torch.ones_like(score), mask, pads, dilate, border)
                assert np.array_equal(_nz(score), _nz(exp)), (dname, border, "zero pattern")
                kept = score != 0
                assert torch.equal(score[kept], shuf[kept]) and torch.equal(bf.prob.cpu(), bf0.prob.cpu()), (dname, border)
                if dname != "bool":
                    assert torch.equal(score[full], score_none[full]), (dname, border, "an all-ones mask is no mask")
    finally:
        ext.remove_borders = old


@pytest.mark.parametrize("side", ["event", "image"])
def test_forward_with_a_non_bool_mask_and_no_border(small_model, side):
    """one forward per extractor family that pads (VGGExtractor, SuperPointv1; the cell-1 families have no padding ring) with
    remove_borders = 0 and a uint8 mask: `score`, `nms` and `sparse_positions` are the statement's mask and border applied to the
    forward's own `probability`, then detect_ref.nms_torch, detect_ref.select_torch on the padded map, unpad_positions and the
    in-image filter.  The zero-pad reading (the same mask as bool) gives another keypoint set on this input."""
    c, sd, kind, sec, x, m, pads = er.forward_case(CONV, side)
    ext = getattr(small_model, f"{side}_extractor").extractor
    H, W = x.shape[-2:]
    assert min(pads) > 0
    old = ext.remove_borders
    try:
        ext.remove_borders = 0
        got = ext(_t(x.copy()), _t(m))
        zer = ext(_t(x.copy()), _t(m.astype(bool)))
    finally:
        ext.remove_borders = old
    exp = er.forward_chain(_np(got["probability"]), m, pads, kind, sec, (H, W))
    assert np.array_equal(_np(got["score"]), exp["score"])
    assert np.array_equal(_np(got["nms"]), exp["nms"])
    for b in range(x.shape[0]):
        assert np.array_equal(_np(got["sparse_positions"][b]), exp["sparse_positions"][b]), b
    assert sum(len(p) for p in exp["sparse_positions"]) > 0
    assert any(not np.array_equal(_np(a), _np(b)) for a, b in zip(got["sparse_positions"], zer["sparse_positions"])), \
        "the zero-pad reading must give a different keypoint set here, or the case tests nothing"


# ------------------------------------------------------------------ descriptors
@pytest.mark.parametrize("D", er.NORMALIZE_D)
def test_normalize_map_and_rows_vs_statement(D):
    """normalize_map_tile_kernel<32> (D <= 512) and normalize_map_kernel (513) at P = 1, 31, 32, 33 pixels, with a zero pixel and a
    pixel of 1e-20 values (the eps clamp acts: not a unit vector); its channels-last copy is the raw values; normalize_rows on the
    same widths"""
    for P in er.NORMALIZE_P:
        x, facts = er.normalize_input(D, P)
        exp = er.normalize(x, 1.3, dim=1)
        bound = er.normalized_bound(x, None, er.norm_terms_map(D), 1.3, 1)
        if D <= 512:
            out, cl = N.normalize_map(_t(x), 1.3, want_cl=True)
            assert np.array_equal(_np(cl), x.transpose(0, 2, 1))
        else:
            out = N.normalize_map(_t(x), 1.3)
        er.within(f"normalize_map[D{D},P{P}]", out.cpu(), exp, bound)
        assert not out[facts["zero"][0], :, facts["zero"][1]].any()
        rows = np.ascontiguousarray(x.transpose(0, 2, 1).reshape(-1, D))
        er.within(f"normalize_rows[D{D},P{P}]", N.normalize_rows(_t(rows), 1.3).cpu(), er.normalize(rows, 1.3, dim=1),
                  er.normalized_bound(rows, None, er.norm_terms_wave(D), 1.3, 1))


@pytest.mark.parametrize("D", er.SAMPLE_D)
def test_desc_sample_bilinear_vs_statement(D):
    """desc_sample_kernel<true> from both layouts (channel planes, the channels-last copy) on a 3x4 map under a 24x32 image:
    keypoints in the four corners, on every edge row and column (their outside taps carry weight: grid_sample's zero padding) and
    in the interior; counts (cap, 0) and (5, cap - 1) at a cap that is no multiple of 4"""
    hc, wc = er.SAMPLE_MAP
    Hp, Wp = er.SAMPLE_PADDED
    raw, launches, cap = er.sample_case(D)
    rt = _t(raw)
    _, cl = N.normalize_map(rt, 1.0, want_cl=True)
    for idx_list in launches:
        pos = [er.positions_of(i, Wp) for i in idx_list]
        exp = er.sample_low(raw, pos, (Hp, Wp), 0.9)
        ind = np.zeros((2, cap), np.int32)
        for b in range(2):
            ind[b, :len(idx_list[b])] = idx_list[b]
        cnt = torch.tensor([len(i) for i in idx_list], dtype=torch.int32, device=DEV)
        outs = {"planes": N.desc_sample(rt, _t(ind), cnt, (Hp, Wp), True, 0.9), "channels_last": N.desc_sample(rt, _t(ind), cnt, (Hp, Wp), True, 0.9, raw_cl=cl)}
        helper = dd.sparsify_low_resolution_descriptors(rt, [_t(p) for p in pos], (Hp, Wp), scale_factor=0.9)
        assert [tuple(h.shape) for h in helper] == [(len(i), D) for i in idx_list]
        for b in range(2):
            n = len(idx_list[b])
            if n == 0:
                assert tuple(exp[b].shape) == (0, D)
                continue
            v, a = er.sample_raw(raw[b], pos[b], (Hp, Wp))
            bound = er.normalized_bound(v, er.sample_value_bound(raw[b], a, hc, wc), er.norm_terms_wave(D), 0.9, 1)
            for layout, out in outs.items():
                er.within(f"desc_sample.{layout}[D{D}]", out[b, :n].cpu(), exp[b], bound)
            er.within(f"desc_sample.helper[D{D}]", helper[b].cpu(), exp[b], bound)


def test_gather_vs_statement():
    """desc_sample_kernel<false> through sparsify_full_resolution_descriptors: every pixel of a 5x7 map at fractional positions
    that floor() removes, D = 128, scale 1.41.  The gathered pixel is index-only: each row normalises exactly its own pixel."""
    D, H, W, scale = er.GATHER_CASE
    raw = er.desc_values(41, (1, D, H, W), -2.0, 2.0)
    pos = er.gather_positions(H, W)
    exp = er.gather_full(raw, [pos], scale)[0]
    got = dd.sparsify_full_resolution_descriptors(_t(raw), (_t(pos),), scale_factor=torch.tensor(scale))[0].cpu()
    picked = torch.from_numpy(raw).double()[0].reshape(D, -1).T
    er.within("gather", got, exp, er.normalized_bound(picked, None, er.norm_terms_wave(D), scale, 1))
    assert np.array_equal(np.sign(got.numpy()), np.sign(picked.numpy())), "each row carries the signs of its own pixel"


@pytest.mark.parametrize("case", er.UPSAMPLE_CASES, ids=lambda c: "x".join(map(str, c[:6])))
def test_upsample_normalize_vs_statement(case):
    """upsample_den_kernel + upsample_store_kernel (the two-kernel path, the LDS-limit case included) and upsample_band_kernel (one
    word past it) against F.interpolate in float64 + normalize + the Padder's crop"""
    B, D, hc, wc, Hp, Wp, (h0, w0, H, W) = case
    pads = er.upsample_pads(case)
    raw = er.desc_values(900 + D + hc, (B, D, hc, wc), -2.0, 2.0)
    up, a = er.upsample_raw(raw, (Hp, Wp))
    bound = er.unpad(er.normalized_bound(up, er.upsample_value_bound(raw, a, hc, wc), er.norm_terms_map(D), 1.25, 1), pads)
    got = N.upsample_normalize(_t(raw), (Hp, Wp), pads, 1.25)
    assert tuple(got.shape) == (B, D, H, W)
    er.within(f"upsample[{'x'.join(map(str, case[:6]))}]", got.cpu(), er.upsample(raw, (Hp, Wp), 1.25, pads), bound)


def test_range_edges_zero_inf_pattern():
    """one case per op at the float32 range edges, against torch's CPU float32 op on the zero / inf / NaN pattern only: a pixel of
    1e30 (the sum of squares overflows: denominator inf, output 0) and one of 1e-30 (the squares underflow: the clamp divides)"""
    for D in (7, 65):
        x = er.range_edge_input(D, 5)
        t32 = 1.3 * F.normalize(torch.from_numpy(x), p=2, dim=1)
        assert np.array_equal(er.zero_inf_pattern(N.normalize_map(_t(x), 1.3).cpu()), er.zero_inf_pattern(t32)), "normalize_map"
        rows = np.ascontiguousarray(x[0].T)
        assert np.array_equal(er.zero_inf_pattern(N.normalize_rows(_t(rows), 1.3).cpu()),
                              er.zero_inf_pattern(1.3 * F.normalize(torch.from_numpy(rows), dim=1))), "normalize_rows"
    # gather and bilinear sample of such pixels, dense upsample of such a map
    D, H, W = 65, 2, 3
    x = er.range_edge_input(D, H * W).reshape(1, D, H, W)
    pos = er.positions_of(np.arange(H * W), W)
    got = dd.sparsify_full_resolution_descriptors(_t(x), (_t(pos),), scale_factor=1.0)[0].cpu()
    exp = F.normalize(torch.from_numpy(x)[0].reshape(D, -1).T, dim=1)
    assert np.array_equal(er.zero_inf_pattern(got), er.zero_inf_pattern(exp)), "gather"
    size = (H * 8, W * 8)
    kp = er.positions_of(np.arange(size[0] * size[1]), size[1])
    got = dd.sparsify_low_resolution_descriptors(_t(x), [_t(kp)], size, scale_factor=1.0)[0].cpu()
    s32 = F.grid_sample(torch.from_numpy(x), er._grid(kp, size), mode="bilinear", align_corners=False).view(D, -1).T
    assert np.array_equal(er.zero_inf_pattern(got), er.zero_inf_pattern(F.normalize(s32, dim=1))), "desc_sample"
    up32 = F.normalize(F.interpolate(torch.from_numpy(x), size=size, mode="bilinear", align_corners=False, antialias=False), dim=1)
    got = N.upsample_normalize(_t(x), size, (0, 0, 0, 0), 1.0).cpu()
    assert np.array_equal(er.zero_inf_pattern(got), er.zero_inf_pattern(up32)), "upsample_normalize"
