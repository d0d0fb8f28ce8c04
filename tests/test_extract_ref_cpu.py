"""tests/extract_ref.py -- the reference's score-map and descriptor steps as torch calls -- held against what already exists, so that
a wrong statement cannot reach tests/test_extract_ref_gpu.py: the reference's own outputs in tests/golden (desc.npz, the small cases
of conv.npz), the C oracle on every input of the GPU file under the same bounds, and torch's float32 operation alone under those
bounds (a bound that torch's own float32 result misses is a wrong derivation).  Every constructed input asserts the fact it is
there for.  The positions contract of the drop-in descriptor helpers is tested here too, on CPU tensors: it raises before any
kernel is reached."""
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import extract_ref as er
from helpers import Golden, load_pkg, synth
from test_oracle_golden import _desc_positions

pkg = load_pkg()
DESC = Golden("desc")
CONV = Golden("conv")


def _pattern(x):
    return np.asarray(er._t(x) != 0)


# ------------------------------------------------------------------ the statement against the reference's own outputs
@pytest.mark.parametrize("name", ["low_d32", "low_d256"])
def test_statement_vs_golden_low_resolution(name):
    """sparsify_low_resolution_descriptors and normalize_descriptors as the reference computed them (torch float32 CPU): inside
    the bounds the kernels are held to, so the fixture checks statement and derivation at once"""
    c = DESC.cases[name]
    raw = synth.normalish(c["seed"], (2, c["D"], c["hc"], c["wc"]))
    Hp, Wp = c["hc"] * 8, c["wc"] * 8
    idx = _desc_positions(c, 0)
    pos = er.positions_of(idx, Wp)
    out = er.sample_low(raw, [pos, pos[:0]], (Hp, Wp), c["scale"])
    assert tuple(out[1].shape) == tuple(DESC[f"{name}.desc1_shape"]) and out[1].dtype == torch.float64
    v, a = er.sample_raw(raw[0], pos, (Hp, Wp))
    assert er.taps_outside(pos, (Hp, Wp), c["hc"], c["wc"])[:4].all(), "the four corner keypoints have taps in the zero ring"
    E = er.sample_value_bound(raw[0], a, c["hc"], c["wc"])
    er.within(f"golden.sample_low[{name}]", DESC[f"{name}.desc0"], out[0], er.normalized_bound(v, E, c["D"], c["scale"], 1))
    co = er.normalize(raw, 1.0, dim=1)
    er.within(f"golden.normalize[{name}]", DESC[f"{name}.coarse"], co, er.normalized_bound(raw, None, c["D"], 1.0, 1))


def test_statement_vs_golden_gather_and_upsample():
    c = DESC.cases["full_d128"]
    raw = synth.normalish(c["seed"], (1, c["D"], c["H"], c["W"]))
    idx = _desc_positions(c, 0)
    pos = er.positions_of(idx, c["W"])
    out = er.gather_full(raw, [pos], c["scale"])[0]
    picked = torch.from_numpy(raw).double()[0].reshape(c["D"], -1)[:, torch.from_numpy(idx.astype(np.int64))].T
    er.within("golden.gather", DESC["full_d128.desc0"], out, er.normalized_bound(picked, None, c["D"], c["scale"], 1))
    c = DESC.cases["dense_d16"]
    raw = synth.normalish(c["seed"], (1, c["D"], c["hc"], c["wc"]))
    size = (c["hc"] * 8, c["wc"] * 8)
    up, a = er.upsample_raw(raw, size)
    E = er.upsample_value_bound(raw, a, c["hc"], c["wc"])
    er.within("golden.upsample", DESC["dense_d16.up"], er.upsample(raw, size, 1.0), er.normalized_bound(up, E, c["D"], 1.0, 1))


_SMALL = [(n, side) for n in CONV.cases for side in ("ev", "im") if f"{n}.{side}.logits" in CONV and f"{n}.{side}.score" in CONV]


@pytest.mark.parametrize("name,side", _SMALL, ids=[f"{n}.{s}" for n, s in _SMALL])
def test_statement_vs_golden_logits_to_score(name, side):
    """the reference's own `score` of the small whole-network cases from its own `logits`: softmax / sigmoid, pixel shuffle, the
    (bool, zero-padded, dilated) events mask, the border frame and the crop"""
    c = CONV.cases[name]
    cfg = c["cfg"]
    kind = cfg[f"{'event' if side == 'ev' else 'image'}_extractor"]["type"]
    sec = cfg[f"{'event' if side == 'ev' else 'image'}_extractor"][kind]
    H, W = c.get("H", 260), c.get("W", 346)
    logits = CONV[f"{name}.{side}.logits"]
    cell = 8 if logits.shape[1] == 65 else 1
    pads = pkg.native.padder_pads(H, W, cell)
    mask = synth.synth_events(c["iseed"], c["B"], c["ce"], H, W)[1] if side == "ev" else None
    assert mask is None or mask.dtype == np.bool_
    prob, score, _ = er.score_map(logits, mask, pads, dilate=True, border=sec["remove_borders"])
    exp = CONV[f"{name}.{side}.score"]
    got = er.unpad(score, pads)
    assert np.array_equal(_pattern(got), _pattern(exp)), "zero pattern"
    p = prob if cell == 1 else F.pixel_shuffle(prob[:, :-1], 8)
    b = er.prob_bound(logits, er.probability(logits))
    b = b if cell == 1 else F.pixel_shuffle(b[:, :-1], 8)
    er.within(f"golden.score[{name}.{side}]", exp, got, er.unpad(b, pads))
    assert p.shape == score.shape


# ------------------------------------------------------------------ score map: the C oracle and torch float32 on the GPU file's inputs
@pytest.mark.parametrize("dilate", [False, True])
@pytest.mark.parametrize("sid,C,hc,wc,pads", er.SCORE_SHAPES, ids=[s[0] for s in er.SCORE_SHAPES])
def test_score_map_oracle_vs_statement(oracle, sid, C, hc, wc, pads, dilate):
    """every (mask dtype, pattern, border) of the GPU file: the oracle's zero pattern is exactly the statement's, its kept pixels are
    its own pixel-shuffled probability, and that probability is inside the bound.  With zero padding for every dtype (the parent
    of this test) the rows of a dtype other than bool fail wherever a pad exceeds the border: finding 1."""
    Hp, Wp, H, W = er.score_geometry(C, hc, wc, pads)
    logits = er.score_logits(C, hc, wc)
    p64 = er.probability(logits)
    assert float((torch.from_numpy(logits).double() - torch.from_numpy(logits).double().amax(1, keepdim=True)).abs().max()) < 60
    bound = er.prob_bound(logits, p64)
    eprob, eshuf = oracle.logits_to_score(logits)
    er.within(f"oracle.prob[{sid}]", eprob, p64, bound)
    t32 = torch.softmax(torch.from_numpy(logits), 1) if C == 65 else 1 / (1 + torch.exp(-torch.from_numpy(logits)))
    er.within(f"torch32.prob[{sid}]", t32, p64, bound)
    base = er.pattern_batch(H, W)
    ring = er.ring(pads, Hp, Wp)
    told_apart = 0
    for dname in er.MASK_DTYPES:
        mask = er.typed_mask(base, dname)
        vis = er.visible(mask, pads, dilate)
        if dname != "bool" and ring.any():
            zero = er.visible(torch.from_numpy(base), pads, dilate)
            corners = er.MASK_PATTERNS.index("corners")
            assert bool((vis[corners, 0] & ring & ~zero[corners, 0]).any()), "a ring pixel is visible under replicate and not under zero padding"
            told_apart += 1
        for border in er.BORDERS:
            _, s64, _ = er.score_map(logits, mask, pads, dilate, border)
            got = eshuf.copy()
            oracle.mask_border(got, mask.numpy(), pads, dilate, border)
            assert np.array_equal(_pattern(got), _pattern(s64)), (dname, border)
            kept = got != 0
            assert np.array_equal(got[kept], eshuf[kept])
    assert told_apart == (len(er.MASK_DTYPES) - 1 if ring.any() else 0)
    full = er.MASK_PATTERNS.index("full")
    assert bool(er.visible(er.typed_mask(base, "f32_1"), pads, True)[full].all()), "an all-ones mask that is not bool hides nothing, ring included"
    assert not bool(er.visible(torch.from_numpy(base), pads, True)[full].all()) or not ring.any()


def test_signed_and_denormal_float_masks_are_a_stated_departure(oracle):
    """the reference decides visibility as `conv(mask.float(), ones / 9) > 0` in float32: 1e-45 alone underflows (not visible), +1
    next to -1 cancel.  The package reads a mask that is not bool as its non-zero pixels (stated departures): this
    test pins both facts, and that the two readings agree on the ordinary values 0.5 and 1.0."""
    sid, C, hc, wc, pads = er.SCORE_SHAPES[0]
    Hp, Wp, H, W = er.score_geometry(C, hc, wc, pads)
    m, facts = er.special_float_mask(H, W)
    w0, _, h0, _ = pads
    ref = er.visible(m, pads, True)[0, 0]
    ours = er.visible(er.nonzero_mask(m), pads, True)[0, 0]
    at = lambda yx: (yx[0] + h0, yx[1] + w0)  # noqa: E731
    assert not ref[at(facts["denormal"])] and ours[at(facts["denormal"])]
    a, b = facts["pair"]
    assert not ref[at(a)] and not ref[at(b)] and ours[at(a)] and ours[at(b)], "both pixels of the pair see +1 and -1"
    assert ref[at(facts["half"])] and ref[at(facts["one"])] and ours[at(facts["half"])] and ours[at(facts["one"])]
    assert bool((ours | ~ref).all()), "non-zero reading only ever keeps more"
    logits = er.score_logits(C, hc, wc, B=1)
    _, shuf = oracle.logits_to_score(logits)
    oracle.mask_border(shuf, m.numpy(), pads, True, 0)
    assert np.array_equal(shuf[0, 0] != 0, ours.numpy()) and not np.array_equal(shuf[0, 0] != 0, ref.numpy())


# ------------------------------------------------------------------ descriptors: the C oracle and torch float32 on the GPU file's inputs
@pytest.mark.parametrize("D", er.NORMALIZE_D)
def test_normalize_oracle_vs_statement(oracle, D):
    for P in er.NORMALIZE_P:
        x, facts = er.normalize_input(D, P)
        n = facts["norms"]
        assert n[facts["zero"]] == 0.0
        assert P == 1 or 0.0 < n[facts["tiny"]] < 1e-12, "this pixel's norm is below 1e-12 and not zero"
        exp = er.normalize(x, 1.3, dim=1)
        if P > 1:
            unit = torch.linalg.vector_norm(exp, dim=1)
            assert float(unit[facts["tiny"]]) < 1.3 * 1e-6 and abs(float(unit[0, 1]) - 1.3) < 1e-9, "the clamp acts: not a unit vector"
        bound = er.normalized_bound(x, None, er.norm_terms_map(D), 1.3, 1)
        er.within(f"oracle.normalize_map[D{D},P{P}]", oracle.normalize_map(x[..., None], 1.3)[..., 0], exp, bound)
        er.within(f"torch32.normalize[D{D},P{P}]", 1.3 * F.normalize(torch.from_numpy(x), p=2, dim=1), exp, bound)
        rows = np.ascontiguousarray(x.transpose(0, 2, 1).reshape(-1, D))
        er.within(f"oracle.normalize_rows[D{D},P{P}]", oracle.normalize_rows(rows, 1.3), er.normalize(rows, 1.3, dim=1),
                  er.normalized_bound(rows, None, er.norm_terms_wave(D), 1.3, 1))


def _sample_expected(raw, idx_list, scale):
    hc, wc = er.SAMPLE_MAP
    Hp, Wp = er.SAMPLE_PADDED
    pos = [er.positions_of(i, Wp) for i in idx_list]
    exp = er.sample_low(raw, pos, (Hp, Wp), scale)
    bounds = []
    for b, p in enumerate(pos):
        if len(p) == 0:
            bounds.append(torch.zeros((0, raw.shape[1]), dtype=torch.float64))
            continue
        v, a = er.sample_raw(raw[b], p, (Hp, Wp))
        bounds.append(er.normalized_bound(v, er.sample_value_bound(raw[b], a, hc, wc), er.norm_terms_wave(raw.shape[1]), scale, 1))
    return pos, exp, bounds


@pytest.mark.parametrize("D", er.SAMPLE_D)
def test_sample_low_oracle_vs_statement(oracle, D):
    hc, wc = er.SAMPLE_MAP
    Hp, Wp = er.SAMPLE_PADDED
    raw, launches, cap = er.sample_case(D)
    assert cap % 4 != 0
    for idx_list in launches:
        pos, exp, bounds = _sample_expected(raw, idx_list, 0.9)
        got = oracle.desc_sample_bilinear(raw, idx_list, (Hp, Wp), 0.9)
        for b in range(2):
            assert got[b].shape == tuple(exp[b].shape)
            if len(pos[b]) == 0:
                continue
            out = er.taps_outside(pos[b], (Hp, Wp), hc, wc)
            assert out.any() and (len(out) == 5 or not out.all()), "some keypoints have a weighted tap outside the map; of a whole set, others have none"
            er.within(f"oracle.sample_low[D{D}]", got[b], exp[b], bounds[b])
            t32 = F.grid_sample(torch.from_numpy(raw[b:b + 1]), er._grid(pos[b], (Hp, Wp)), mode="bilinear", align_corners=False)
            t32 = 0.9 * F.normalize(t32.view(-1, len(pos[b])).T, p=2, dim=1)
            er.within(f"torch32.sample_low[D{D}]", t32, exp[b], bounds[b])


def test_gather_oracle_vs_statement(oracle):
    D, H, W, scale = er.GATHER_CASE
    raw = er.desc_values(41, (1, D, H, W), -2.0, 2.0)
    pos = er.gather_positions(H, W)
    assert np.array_equal(np.floor(pos[:, 0]) * W + np.floor(pos[:, 1]), np.arange(H * W)) and (pos[:, :2] % 1 != 0.5).any()
    exp = er.gather_full(raw, [pos], scale)[0]
    picked = torch.from_numpy(raw).double()[0].reshape(D, -1).T
    got = oracle.desc_gather(raw, [np.arange(H * W, dtype=np.int32)], scale)[0]
    er.within("oracle.gather", got, exp, er.normalized_bound(picked, None, er.norm_terms_wave(D), scale, 1))


@pytest.mark.parametrize("case", er.UPSAMPLE_CASES, ids=lambda c: "x".join(map(str, c[:6])))
def test_upsample_oracle_vs_statement(oracle, case):
    B, D, hc, wc, Hp, Wp, (h0, w0, H, W) = case
    pads = er.upsample_pads(case)
    raw = er.desc_values(900 + D + hc, (B, D, hc, wc), -2.0, 2.0)
    up, a = er.upsample_raw(raw, (Hp, Wp))
    bound = er.unpad(er.normalized_bound(up, er.upsample_value_bound(raw, a, hc, wc), er.norm_terms_map(D), 1.25, 1), pads)
    exp = er.upsample(raw, (Hp, Wp), 1.25, pads)
    assert tuple(exp.shape) == (B, D, H, W)
    tag = "x".join(map(str, case[:6]))
    er.within(f"oracle.upsample[{tag}]", er.unpad(torch.from_numpy(oracle.upsample_normalize(raw, (Hp, Wp), 1.25)), pads), exp, bound)
    t32 = F.interpolate(torch.from_numpy(raw), size=(Hp, Wp), mode="bilinear", align_corners=False, antialias=False)
    er.within(f"torch32.upsample[{tag}]", er.unpad(1.25 * F.normalize(t32, p=2, dim=1), pads), exp, bound)


def test_range_edges_zero_inf_pattern(oracle):
    """at the float32 range edges the sum of squares overflows (denominator inf, output 0) or underflows (the clamp divides): the
    oracle gives torch's float32 zero / inf / NaN pattern -- values are not compared there"""
    for D in (7, 65):
        x = er.range_edge_input(D, 5)
        t32 = 1.3 * F.normalize(torch.from_numpy(x), p=2, dim=1)
        assert bool((t32[0, :, 0] == 0).all()) and bool((t32[0, :, 1] != 0).all()), "overflow gives zeros, underflow the clamp's quotient"
        assert np.array_equal(er.zero_inf_pattern(oracle.normalize_map(x[..., None], 1.3)[..., 0]), er.zero_inf_pattern(t32))
        rows = np.ascontiguousarray(x[0].T)
        assert np.array_equal(er.zero_inf_pattern(oracle.normalize_rows(rows, 1.3)), er.zero_inf_pattern(1.3 * F.normalize(torch.from_numpy(rows), dim=1)))
    D, H, W = 65, 2, 3
    x = er.range_edge_input(D, H * W).reshape(1, D, H, W)
    exp = F.normalize(torch.from_numpy(x)[0].reshape(D, -1).T, dim=1)
    assert np.array_equal(er.zero_inf_pattern(oracle.desc_gather(x, [np.arange(H * W, dtype=np.int32)], 1.0)[0]), er.zero_inf_pattern(exp))
    size = (H * 8, W * 8)
    idx = np.arange(size[0] * size[1], dtype=np.int32)
    kp = er.positions_of(idx, size[1])
    s32 = F.grid_sample(torch.from_numpy(x), er._grid(kp, size), mode="bilinear", align_corners=False).view(D, -1).T
    assert np.array_equal(er.zero_inf_pattern(oracle.desc_sample_bilinear(x, [idx], size, 1.0)[0]), er.zero_inf_pattern(F.normalize(s32, dim=1)))
    up32 = F.normalize(F.interpolate(torch.from_numpy(x), size=size, mode="bilinear", align_corners=False, antialias=False), dim=1)
    assert np.array_equal(er.zero_inf_pattern(oracle.upsample_normalize(x, size, 1.0)), er.zero_inf_pattern(up32))


# ------------------------------------------------------------------ finding 1 through a whole extractor (documents the GPU rows)
@pytest.mark.parametrize("side", ["event", "image"])
def test_zero_pad_reading_changes_the_keypoints(oracle, side):
    """the oracle's whole forward with remove_borders = 0 under both readings of one mask: as uint8 (ring replicated) and as bool (ring
    zero) the keypoint sets differ, because a ring maximum suppresses in-image neighbours within the NMS radius; and the uint8
    forward is the statement's chain on its own probability"""
    c, sd, kind, sec, x, m, pads = er.forward_case(CONV, side)
    H, W = x.shape[-2:]
    assert min(pads) > 0 and m.dtype == np.uint8 and set(np.unique(m)) == {0, 1}
    kw = dict(top_k=sec["detection_top_k"], radius=sec["nms_radius"], border=0, det_thr=sec["detection_threshold"])
    rep = oracle.extractor_forward(kind, sd, x.copy(), m, **kw)
    zer = oracle.extractor_forward(kind, sd, x.copy(), m.astype(bool), **kw)
    assert any(not np.array_equal(a, b) for a, b in zip(rep["sparse_positions"], zer["sparse_positions"]))
    exp = er.forward_chain(rep["probability"], m, pads, kind, sec, (H, W))
    for b in range(x.shape[0]):
        assert np.array_equal(rep["sparse_positions"][b], exp["sparse_positions"][b]), b
    assert np.array_equal(rep["score"], exp["score"]) and np.array_equal(rep["nms"], exp["nms"])


# ------------------------------------------------------------------ finding 2: the positions contract of the drop-in helpers
dd = import_module(pkg.__name__ + ".core.modules.utils.descriptor_util")


def test_pack_positions_valid_inputs_pack_as_before():
    Hp, Wp = er.SAMPLE_PADDED
    idx = er.sample_keypoints()
    pos = torch.from_numpy(er.positions_of(idx, Wp))
    packed, cnt = dd._pack_positions([pos, pos[:0], pos[:7]], (Hp, Wp), bilinear=True)
    assert cnt.tolist() == [len(idx), 0, 7] and packed.dtype == torch.int32 and tuple(packed.shape) == (3, len(idx))
    assert np.array_equal(packed[0].numpy(), idx) and np.array_equal(packed[2, :7].numpy(), idx[:7]) and not packed[1].any()
    D, H, W, _ = er.GATHER_CASE
    gp = torch.from_numpy(er.gather_positions(H, W))
    packed, cnt = dd._pack_positions([gp], (H, W), bilinear=False)
    assert np.array_equal(packed[0].numpy(), np.arange(H * W)) and cnt.tolist() == [H * W]
    packed, cnt = dd._pack_positions([gp[:0]], (H, W), bilinear=False)
    assert cnt.tolist() == [0] and tuple(packed.shape) == (1, 1)


@pytest.mark.parametrize("yx", [(5.0, 0.5), (0.5, 7.0), (-0.5, 0.5), (0.5, -0.25), (float("nan"), 0.5), (4.5, float("inf"))], ids=str)
def test_gather_refuses_positions_outside_the_map(yx):
    """the reference raises IndexError for an index >= size; the kernel would read at c * plane + y * W + x unchecked"""
    D, H, W, _ = er.GATHER_CASE
    raw = torch.zeros((2, D, H, W))
    good = torch.tensor([[0.5, 0.5, 0.0], [4.9, 6.9, 0.0]])
    bad = torch.cat([good, torch.tensor([[yx[0], yx[1], 0.0]])])
    with pytest.raises(IndexError, match="out of bounds"):
        dd.sparsify_full_resolution_descriptors(raw, [good, bad])
    dd._pack_positions([good, good], (H, W), bilinear=False)  # the good rows alone pass


@pytest.mark.parametrize("yx", [(10.2, 20.9), (10.0, 20.5), (24.5, 0.5), (0.5, 32.5), (-0.5, 0.5), (float("nan"), 0.5)], ids=str)
def test_bilinear_refuses_positions_it_cannot_sample(yx):
    """a fractional part other than 0.5 (the reference interpolates at the float position: its raw samples at (10.2, 20.9) and
    (10.5, 20.5) differ, asserted here on the statement) and positions outside the padded image"""
    Hp, Wp = er.SAMPLE_PADDED
    raw = er.desc_values(5, (1, 8, 5, 6), -1.0, 1.0)
    a = er.sample_raw(raw[0], np.array([[10.2, 20.9, 0]], np.float32), (40, 48))[0]
    b = er.sample_raw(raw[0], np.array([[10.5, 20.5, 0]], np.float32), (40, 48))[0]
    assert float((a - b).abs().max()) > 1e-3
    good = torch.tensor([[0.5, 0.5, 0.0], [23.5, 31.5, 0.0]])
    bad = torch.cat([good, torch.tensor([[yx[0], yx[1], 0.0]])])
    with pytest.raises(NotImplementedError, match="einx: "):
        dd.sparsify_low_resolution_descriptors(torch.zeros((1, 8, 3, 4)), [bad], (Hp, Wp))
    dd._pack_positions([good], (Hp, Wp), bilinear=True)


def test_new_symbols_resolve_and_the_abi_version_stays():
    L = pkg.native.lib()
    assert hasattr(L, "einx_score_map_pad") and hasattr(L, "einx_extract_pad")
    assert L.einx_abi_version() == 6  # additive symbols only
    m8, pad = pkg.native.mask_bytes(torch.tensor([[0.0, 0.5, -1.0, 1e-45]]))
    assert m8.tolist() == [[0, 1, 1, 1]] and pad == pkg.native.MASK_PAD_REPLICATE
    m8, pad = pkg.native.mask_bytes(torch.tensor([[False, True]]))
    assert m8.tolist() == [[0, 1]] and pad == pkg.native.MASK_PAD_ZERO
