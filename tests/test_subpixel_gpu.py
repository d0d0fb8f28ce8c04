"""GPU tests (-m gpu), component: sub-pixel keypoints -- csrc/subpixel.hip's float-position descriptor sampler
against einx_desc_sample (bit-equal at pixel centres) and against the reference's torch calls in float64 under the a-priori bound
of tests/subpixel_ref.py; the refinement against its float32 restatement (exact); the `subpixel` switch through the whole
extractors, EIM.forward / forward_graph and an evaluator; the blob scene."""
from importlib import import_module

import numpy as np
import pytest
import torch

import extract_ref as er
import subpixel_ref as S
from gpu_support import DEV, _np, _t, pkg
from helpers import close_and_record, sub_dict, synth, synth_raw_events

pytestmark = pytest.mark.gpu

N = pkg.native
dd = import_module(pkg.__name__ + ".core.modules.utils.descriptor_util")
I32 = torch.int32


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def _cl(raw):
    return N.normalize_map(raw, 1.0, want_cl=True)[1]


# ------------------------------------------------------------------ 1. pixel centres: the existing sampler, bit for bit
@pytest.mark.parametrize("cl", [False, True], ids=["planar", "channels_last"])
@pytest.mark.parametrize("D", S.SAMPLE_D)
def test_desc_sample_pos_at_pixel_centres_is_desc_sample(D, cl):
    Hp, Wp = S.SAMPLE_PADDED
    raw = _t(S.sample_raw_map(D))
    raw_cl = _cl(raw) if cl else None
    for cap in S.SAMPLE_CAPS:
        idx = S.centre_indices(cap)
        for counts in ((cap, 0), (0, cap), (min(cap, 3), cap)):
            indices, cnt = _i32(np.stack([idx, idx[::-1]])), _i32(counts)
            exp = N.desc_sample(raw, indices, cnt, (Hp, Wp), True, 1.41, raw_cl=raw_cl)
            pos = np.stack([er.positions_of(idx, Wp), er.positions_of(idx[::-1], Wp)])
            for ordering in ("yx", "xy"):
                p = pos if ordering == "yx" else pos[:, :, [1, 0, 2]]
                for stride in (3, 2):
                    got = N.desc_sample_pos(raw, _t(p[:, :, :stride]), cnt, (Hp, Wp), 1.41, ordering=ordering, raw_cl=raw_cl)
                    for b in range(2):
                        n = counts[b]
                        assert n == 0 or float(got[b, :n].abs().max()) > 0
                        assert torch.equal(got[b, :n], exp[b, :n]), (cap, counts, ordering, stride, b)


# ------------------------------------------------------------------ 2. any float position: the reference's grid_sample in float64
@pytest.mark.parametrize("cl", [False, True], ids=["planar", "channels_last"])
@pytest.mark.parametrize("D", S.SAMPLE_D)
def test_desc_sample_pos_at_float_positions_vs_statement(D, cl):
    """positions inside, on tap boundaries, at the exact corners, in a 3 px band outside the image (which still reaches the map:
    the reference samples there) and far outside (zero rows), two launches with counts (n, 0) and (5, n)"""
    Hp, Wp = S.SAMPLE_PADDED
    scale = 1.41
    raw = S.sample_raw_map(D)
    rt = _t(raw)
    raw_cl = _cl(rt) if cl else None
    p, facts = S.float_positions()
    n = len(p)
    assert n % 4 != 0
    expected = [S.sample_bound(raw[b], p, (Hp, Wp), scale) for b in range(2)]
    pos = _t(np.stack([p, p]))
    for counts in ((n, 0), (5, n)):
        got = N.desc_sample_pos(rt, pos, _i32(counts), (Hp, Wp), scale, raw_cl=raw_cl)
        for b in range(2):
            k = counts[b]
            if k == 0:
                continue
            exp, bound = expected[b]
            tag = f"desc_sample_pos[{'cl' if cl else 'planar'}]"
            near = [i for i in range(k) if i not in facts["far"]]  # (a far row's bound scales with its coordinate; its value is 0)
            close_and_record(tag, _np(got[b, near]), exp[near].numpy(), atol=float(bound[near].max()))
            er.within(f"{tag}[D{D},b{b}]", got[b, :k].cpu(), exp[:k], bound[:k])
            if k == n:
                far = got[b, facts["far"]]
                assert bool((far == 0).all()), "a position whose four taps lie outside the map must give an exactly zero row"
                assert bool((exp[facts["far"]] == 0).all())
    # through the public helper: per-image lists, both orderings
    lists = [_t(p[:7]), _t(p[:0]).reshape(0, 3)]
    out = dd.sample_descriptors_at(rt, lists, (Hp, Wp), scale)
    assert out[1].shape == (0, D) and torch.equal(out[0], N.desc_sample_pos(rt, pos, _i32((7, 0)), (Hp, Wp), scale)[0, :7])
    out_xy = dd.sample_descriptors_at(rt, [t[:, [1, 0, 2]].contiguous() for t in lists], (Hp, Wp), scale, ordering="xy")
    assert torch.equal(out_xy[0], out[0])


def test_desc_sample_pos_gives_zero_rows_for_wild_coordinates():
    """coordinates from which no index may be formed: huge, infinite, NaN -- compared as floats first, zero rows"""
    Hp, Wp = S.SAMPLE_PADDED
    raw = _t(np.abs(S.sample_raw_map(68)[:1]) + 1.0)
    inf, nan = float("inf"), float("nan")
    rows = [(1e30, 3.0), (3.0, -1e30), (inf, 2.0), (2.0, -inf), (nan, 2.0), (2.0, nan), (nan, nan), (3e9, 3e9), (-3e9, 5.0), (20.25, 24.75)]
    p = torch.tensor([rows], dtype=torch.float32, device=DEV)
    for raw_cl in (None, _cl(raw)):
        got = N.desc_sample_pos(raw, p, _i32([len(rows)]), (Hp, Wp), 1.0, raw_cl=raw_cl)
        assert bool((got[0, :-1] == 0).all())
        assert abs(float(got[0, -1].norm()) - 1.0) < 1e-5
    with pytest.raises(ValueError, match="finite"):
        dd.sample_descriptors_at(raw, [p[0]], (Hp, Wp))


# ------------------------------------------------------------------ 3. the refinement rule, exactly
@pytest.fixture(scope="module")
def refine_case():
    return S.refine_case()


@pytest.mark.parametrize("ordering", ["yx", "xy"])
def test_refine_keypoints_equals_the_float32_restatement(refine_case, ordering):
    s, idx, counts, facts = refine_case
    pads = S.REFINE_PADS
    B, cap = idx.shape
    before = S.detector_positions(idx, s, pads, ordering)
    before[2] = 7.0  # an image without keypoints: nothing of it may be written
    pos = _t(before.copy())
    out = N.refine_keypoints(_t(s), _i32(idx), _i32(counts), pos, pads, ordering)
    assert out is pos
    got = _np(pos)
    cols = [1, 0] if ordering == "xy" else [0, 1]
    diff = 0
    for b in range(2):
        exp, _, off = S.refine(s[b], idx[b], pads, np.float32)
        diff += int((got[b][:, cols] != exp).sum())
        assert np.array_equal(got[b][:, cols], exp), (b, got[b][:, cols] - exp)
        assert np.array_equal(got[b, :, 2], before[b, :, 2])  # the score column is not touched
        w0, _, h0, _ = pads
        assert np.array_equal(np.floor(got[b][:, cols] + np.float32([h0, w0])), np.stack([idx[b] // s.shape[2], idx[b] % s.shape[2]], 1))
    assert diff == 0
    assert np.array_equal(got[2], before[2])
    k = facts["dyadic"]
    y, x = idx[0, k] // s.shape[2], idx[0, k] % s.shape[2]
    assert got[0, k, cols[0]] == np.float32(y + 0.5 + 0.25 - pads[2])
    # a count above the capacity is clamped; a count below it leaves the rows past it alone
    pos = _t(before.copy())
    N.refine_keypoints(_t(s), _i32(idx), _i32([cap + 5, 3, 0]), pos, pads, ordering)
    got2 = _np(pos)
    assert np.array_equal(got2[0], got[0]) and np.array_equal(got2[1, :3], got[1, :3]) and np.array_equal(got2[1, 3:], before[1, 3:])


@pytest.mark.parametrize("cl", [False, True], ids=["planar", "channels_last"])
@pytest.mark.parametrize("D", S.SAMPLE_D)
def test_refine_keypoints_resamples_the_rows_at_the_refined_positions(refine_case, D, cl):
    """cell-8 mode on the constructed map (24 x 32 over a 3 x 4 descriptor map): every row equals desc_sample_pos at the refined
    padded-frame position bit for bit, rows with offset (0, 0) equal desc_sample's, rows past the counts are not written"""
    s, idx, counts, facts = refine_case
    pads = S.REFINE_PADS
    Hp, Wp = S.REFINE_MAP
    B, cap = idx.shape
    raw = _t(er.desc_values(31 + D, (B, D, 3, 4), -2.0, 2.0))
    raw_cl = _cl(raw) if cl else None
    cnt = _i32([cap, 5, 0])
    rows = N.desc_sample(raw, _i32(idx), cnt, (Hp, Wp), True, 1.41, raw_cl=raw_cl)
    rows[1, 5:] = 3.0
    rows[2] = 3.0
    pixel = rows.clone()
    pos = _t(S.detector_positions(idx, s, pads))
    N.refine_keypoints(_t(s), _i32(idx), cnt, pos, pads, "yx", raw=raw, raw_cl=raw_cl, sparse_desc=rows, scale=1.41)
    padded = pos.clone()
    padded[:, :, 0] += pads[2]
    padded[:, :, 1] += pads[0]
    exp = N.desc_sample_pos(raw, padded, cnt, (Hp, Wp), 1.41, raw_cl=raw_cl)
    assert torch.equal(rows[0], exp[0]) and torch.equal(rows[1, :5], exp[1, :5])
    assert bool((rows[1, 5:] == 3.0).all()) and bool((rows[2] == 3.0).all())
    for name in ("tie", "corner", "corner0", "no_max", "valley"):
        assert torch.equal(rows[0, facts[name]], pixel[0, facts[name]]), name
    assert not torch.equal(rows[0, facts["dyadic"]], pixel[0, facts["dyadic"]])
    e, bound = S.sample_bound(_np(raw[0]), _np(padded[0]), (Hp, Wp), 1.41)
    er.within(f"refine_describe[D{D}]", rows[0].cpu(), e, bound)


def test_refine_keypoints_refuses_by_name():
    s = torch.zeros((1, 1, 8, 8200), device=DEV)
    idx, cnt, pos = torch.zeros((1, 4), dtype=I32, device=DEV), torch.zeros((1,), dtype=I32, device=DEV), torch.zeros((1, 4, 3), device=DEV)
    with pytest.raises(RuntimeError, match="einx_refine_keypoints.*8192"):
        N.refine_keypoints(s, idx, cnt, pos)
    with pytest.raises(TypeError):
        N.refine_keypoints(s[..., :32].contiguous(), idx.long(), cnt, pos)
    with pytest.raises(ValueError, match="positions"):
        N.refine_keypoints(s[..., :32].contiguous(), idx, cnt, pos[:, :, :2].contiguous())


# ------------------------------------------------------------------ 4. the whole extractors
H, W = 40, 48


def _eim(cfg_name, top_k, seed=21, radius=None):
    cfg = pkg.default_config(cfg_name, event_channels=5)
    et, it = cfg.event_extractor.type, cfg.image_extractor.type
    for sec in (cfg.event_extractor[et], cfg.image_extractor[it]):
        sec.detection_top_k = top_k
        if not top_k:
            sec.detection_threshold = 0.0  # no top-k: every NMS survivor above 0 is a keypoint
        if radius is not None:
            sec.nms_radius = radius
    model = pkg.EIM(cfg, device=DEV).eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return cfg, model, sd


def _side(model, side, B, seed=61):
    """-> (wrapper, call(x) -> feats, numpy input, numpy mask or None)"""
    if side == "event":
        ev, mask = synth.synth_events(seed, B, 5, H, W)
        return model.event_extractor, lambda: model.event_extractor(_t(ev), _t(mask)), ev, mask
    img = synth.synth_image(seed, B, H, W)
    return model.image_extractor, lambda: model.image_extractor(_t(img.copy())), img, None


DENSE_KEYS = ("backbone_feats", "logits", "raw_descriptors", "probability", "score", "nms", "normalized_descriptors")


def _check_refined_against_pixel(on, off, ext):
    """`on` (subpixel) against `off` (pixel) of the same extractor and input -> number of coordinates that moved"""
    for k in DENSE_KEYS + (("coarse_descriptors",) if ext.cell_size == 8 else ()):
        assert torch.equal(on[k], off[k]), k
    bo, bf = on._batched, off._batched
    assert bo.subpixel and not bf.subpixel
    assert torch.equal(bo.det.counts, bf.det.counts) and torch.equal(bo.det.thr, bf.det.thr)
    Hp, Wp = bo.padded
    w0, _, h0, _ = bo.pads
    moved = 0
    yx = [1, 0] if ext.ordering == "xy" else [0, 1]
    for b in range(len(off["sparse_positions"])):
        p1, p0 = on["sparse_positions"][b], off["sparse_positions"][b]
        n = p0.shape[0]
        assert p1.shape == p0.shape
        assert torch.equal(bo.det.indices[b, :n], bf.det.indices[b, :n])
        assert torch.equal(p1[:, 2], p0[:, 2])  # scores: the integer peak's
        if n == 0:
            continue
        assert float((p1[:, :2] - p0[:, :2]).abs().max()) <= S.DMAX
        assert torch.equal(p1[:, :2].floor(), p0[:, :2].floor())
        moved += int((p1[:, :2] != p0[:, :2]).sum())
        # and exactly the restatement on the score map the detection ran on
        exp, _, _ = S.refine(_np(bo.score[b, 0]), _np(bo.det.indices[b, :n]), bo.pads, np.float32)
        assert np.array_equal(_np(p1)[:, yx], exp + np.float32(bo.shift))
    if ext.cell_size == 8:
        padded = bo.det.positions.clone()
        padded[:, :, yx[0]] += h0
        padded[:, :, yx[1]] += w0
        exp = N.desc_sample_pos(bo.raw, padded, bo.det.counts, (Hp, Wp), bo.scale, ordering=ext.ordering, raw_cl=bo.raw_cl)
        for b, d in enumerate(on["sparse_descriptors"]):
            assert torch.equal(d, exp[b, :d.shape[0]])
    else:
        for d1, d0 in zip(on["sparse_descriptors"], off["sparse_descriptors"]):
            assert torch.equal(d1, d0)  # the gather at the integer peak
    return moved


@pytest.mark.parametrize("top_k", [16, 0])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("side", ["event", "image"])
@pytest.mark.parametrize("cfg_name", ["SP_MNN", "SiLK_MNN"])
def test_extractor_with_the_switch_on_and_off(oracle, cfg_name, side, B, top_k):
    cfg, model, sd = _eim(cfg_name, top_k)
    wrapper, call, x, mask = _side(model, side, B)
    ext = wrapper.extractor
    ext.dense_outputs = True
    kind = wrapper.config.type
    sec = wrapper.config[kind]
    assert ext.keypoint_mode == "pixel"
    off = call()
    exp = oracle.extractor_forward(kind, sub_dict(sd, f"{side}_extractor.extractor."), x.copy(), mask, top_k=top_k,
                                   det_thr=sec.detection_threshold, scale=sec.descriptor_scale_factor)
    for k in ("score", "nms", "raw_descriptors"):
        assert np.array_equal(_np(off[k]), exp[k]), k
    for b in range(B):  # the switch off: the parent's outputs, bit for bit
        assert np.array_equal(_np(off["sparse_positions"][b]), exp["sparse_positions"][b])
        assert np.array_equal(_np(off["sparse_descriptors"][b]), exp["sparse_descriptors"][b])
    assert sum(int(p.shape[0]) for p in off["sparse_positions"]) >= (B if top_k else 4 * B)
    ext.subpixel = True
    assert ext.keypoint_mode == "subpixel" and ext.conv_mode == "fp32"
    on = call()
    assert _check_refined_against_pixel(on, off, ext) > 0
    ext.subpixel = False
    again = call()
    for b in range(B):
        assert torch.equal(again["sparse_positions"][b], off["sparse_positions"][b])
        assert torch.equal(again["sparse_descriptors"][b], off["sparse_descriptors"][b])
    ext.train()
    ext.subpixel = True
    assert ext.keypoint_mode == "pixel"


def test_padding0_network_refines_before_the_positions_are_mapped_back():
    cfg = pkg.default_config("SiLK_MNN", event_channels=5)
    cfg.image_extractor.silk.padding = 0
    cfg.image_extractor.silk.detection_top_k = 16
    model = pkg.EIM(cfg, device=DEV).eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=23)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    ext = model.image_extractor.extractor
    ext.dense_outputs = False
    img = synth.synth_image(62, 2, H, W)
    off = model.image_extractor(_t(img.copy()))
    ext.subpixel = True
    on = model.image_extractor(_t(img.copy()))
    bo = on._batched
    assert bo.shift == 9.0 and bo.subpixel
    moved = 0
    for b in range(2):
        p1, p0 = on["sparse_positions"][b], off["sparse_positions"][b]
        assert p0.shape[0] > 0 and torch.equal(p1[:, :2].floor(), p0[:, :2].floor()) and torch.equal(p1[:, 2], p0[:, 2])
        exp, _, _ = S.refine(_np(bo.score[b, 0]), _np(bo.det.indices[b, :p0.shape[0]]), bo.pads, np.float32)
        assert np.array_equal(_np(p1)[:, :2], exp + np.float32(9.0))
        assert torch.equal(on["sparse_descriptors"][b], off["sparse_descriptors"][b])
        moved += int((p1 != p0).sum())
    assert moved > 0


@pytest.mark.parametrize("side", ["event", "image"])
def test_a_re_detection_refines_again(side):
    """nms_radius 3 (the generic pass kernel; radius 4 finishes on the device) with a budget of ONE pass: the forward re-detects
    with a larger budget, and the refinement runs again on the new keypoints"""
    results = []
    for budget in (1, None):
        _, model, _ = _eim("SP_MNN", 16, radius=3)
        wrapper, call, _, _ = _side(model, side, 2)
        ext = wrapper.extractor
        ext.dense_outputs = False
        ext.subpixel = True
        eng = ext.engine()
        if budget:
            eng.nms_base = eng.nms_iters = budget
        results.append(call())
        if budget:
            assert eng.nms_iters > budget, "the forward did not need a re-detection"
    a, b = results
    ext.subpixel = False
    off = call()
    for i in range(2):
        assert torch.equal(a["sparse_positions"][i], b["sparse_positions"][i])
        assert torch.equal(a["sparse_descriptors"][i], b["sparse_descriptors"][i])
        assert torch.equal(a["sparse_positions"][i].floor(), off["sparse_positions"][i].floor())
    assert any(not torch.equal(a["sparse_positions"][i], off["sparse_positions"][i]) for i in range(2))
    assert any(not torch.equal(a["sparse_descriptors"][i], off["sparse_descriptors"][i]) for i in range(2))


# ------------------------------------------------------------------ 5. EIM.forward, forward_graph, an evaluator
def _rows_of(matched, positions):
    """every matched keypoint (first two columns) is a row of the side's sparse positions"""
    have = {tuple(r) for r in _np(positions)[:, :2].tolist()}
    return all(tuple(r) in have for r in _np(matched)[:, :2].tolist())


def _off_centre(p):
    return int(((p[:, :2] - p[:, :2].floor()) != 0.5).sum())


def test_eim_forward_graph_and_evaluator_carry_refined_positions():
    B = 2
    _, model, _ = _eim("SP_MNN", 64, seed=27)
    exts = (model.event_extractor.extractor, model.image_extractor.extractor)
    for e in exts:
        e.dense_outputs = False
        e.subpixel = True
    ev, mask = synth.synth_events(63, B, 5, H, W)
    img = synth.synth_image(63, B, H, W)
    ef, imf, m = model(_t(ev), _t(img.copy()), _t(mask))
    n_matched = 0
    for b in range(B):
        assert _off_centre(ef["sparse_positions"][b]) > 0 and _off_centre(imf["sparse_positions"][b]) > 0
        assert _rows_of(m["matched_kpts0"][b], ef["sparse_positions"][b]) and _rows_of(m["matched_kpts1"][b], imf["sparse_positions"][b])
        n_matched += int(m["matched_kpts0"][b].shape[0])
        if m["matched_kpts0"][b].shape[0]:
            assert _off_centre(m["matched_kpts0"][b]) + _off_centre(m["matched_kpts1"][b]) > 0
    assert n_matched > 0
    # the captured graph holds the extra launches: replay == eager
    for _ in range(2):
        gf, gi, gm = model.forward_graph(_t(ev), _t(img.copy()), _t(mask))
        for b in range(B):
            assert torch.equal(gf["sparse_positions"][b], ef["sparse_positions"][b]) and torch.equal(gi["sparse_positions"][b], imf["sparse_positions"][b])
            assert torch.equal(gf["sparse_descriptors"][b], ef["sparse_descriptors"][b]) and torch.equal(gi["sparse_descriptors"][b], imf["sparse_descriptors"][b])
            assert torch.equal(gm["matches0"][b], m["matches0"][b]) and torch.equal(gm["matched_kpts1"][b], m["matched_kpts1"][b])
    assert len(model._graphs) == 1
    # toggling one side re-captures, and that side is back on pixel centres while the other stays refined
    exts[1].subpixel = False
    gf, gi, gm = model.forward_graph(_t(ev), _t(img.copy()), _t(mask))
    assert len(model._graphs) == 2
    for b in range(B):
        assert _off_centre(gi["sparse_positions"][b]) == 0 and torch.equal(gf["sparse_positions"][b], ef["sparse_positions"][b])
    exts[1].subpixel = True
    model.forward_graph(_t(ev), _t(img.copy()), _t(mask))
    assert len(model._graphs) == 2  # the first capture is found again
    # one evaluator step on raw events: the matches it scores are the refined keypoints
    evs = [synth_raw_events(dict(seed=700 + b, n=3000, H=H, W=W, bins=5, frac=False, pneg=False)) for b in range(B)]
    runner = pkg.DifferentTimeEvaluator(model, bins=5, resolution=(W, H))
    rows, (ef2, imf2, m2) = runner.step(evs, _t(img.copy()))
    for b in range(B):
        assert _off_centre(ef2["sparse_positions"][b]) > 0 and _off_centre(imf2["sparse_positions"][b]) > 0
        assert _rows_of(m2["matched_kpts0"][b], ef2["sparse_positions"][b]) and _rows_of(m2["matched_kpts1"][b], imf2["sparse_positions"][b])
    for e in exts:
        e.subpixel = False
    rows_off, (ef3, _, _) = pkg.DifferentTimeEvaluator(model, bins=5, resolution=(W, H)).step(evs, _t(img.copy()))
    assert all(_off_centre(p) == 0 for p in ef3["sparse_positions"])


# ------------------------------------------------------------------ 6. the blob scene on the device
def test_blob_scene_through_detect_and_refine():
    """condition A: every refined keypoint within 0.05 px of its blob's centre; condition B: the pixel centres einx_detect emits are
    off by at least 0.3 px on average (tests/test_subpixel_cpu.py asserts both on the restatement: 0.030 / 0.388)"""
    score, centres = S.blob_scene()
    Hm, Wm = S.BLOB_MAP
    st = _t(score[:, None])
    det = N.detect(st, top_k=0, radius=4, det_thr=0.5, cap=64, nms_iters=8)
    counts = _np(det.counts)
    assert counts.tolist() == [centres.shape[1]] * S.BLOB_IMAGES and not bool(det.not_converged.any())
    pixel = _np(det.positions).copy()
    N.refine_keypoints(st, det.indices, det.counts, det.positions)
    got, idx = _np(det.positions), _np(det.indices)
    errs, pix = [], []
    for b in range(S.BLOB_IMAGES):
        n = counts[b]
        exp, _, _ = S.refine(score[b], idx[b, :n], dtype=np.float32)
        assert np.array_equal(got[b, :n, :2], exp)
        e, _ = S.blob_errors(got[b, :n], idx[b, :n], centres[b], Wm)
        p, _ = S.blob_errors(pixel[b, :n], idx[b, :n], centres[b], Wm)
        errs.append(e)
        pix.append(p)
    errs, pix = np.concatenate(errs), np.concatenate(pix)
    print(f"blob scene on the device: {errs.size} blobs, refined max {errs.max():.4f} px, pixel centres mean {pix.mean():.4f} px")
    assert errs.size == 560
    assert errs.max() <= S.BLOB_A
    assert pix.mean() >= S.BLOB_B
