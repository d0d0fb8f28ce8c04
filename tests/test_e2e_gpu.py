"""GPU tests (-m gpu), component: e2e.
SURVEY 8a rows A4-A6, A18, A22 end to end: whole extractors and whole EIM / ImageImageMatcher forwards against the oracle and the reference's fixtures, at the fixture sizes and at BASELINE.json's batch sizes.
(Round 6 regrouped the per-round files test_gpu_parity / test_r2..r5_gpu by component; shared helpers live in gpu_support.py.)"""
import numpy as np
import pytest
import torch
import json
import os
import sys
import statistics
import subprocess
import time
from importlib import import_module

from helpers import (check_matches_vs_reference, close_and_record, la_bound, la_bound_e2e, lg_noise, record_flips, record_only,
                     split, state_dict_for, sub_dict, synth, twin_inputs, twin_state_dict_for, upstream_deviation)
from test_lightglue_f64_gpu import SHIPPED, _check_pair
from gpu_support import (CONV, DEV, E2E, FTOL, LGCAL, MNN, PAD0, _Z, _assert_feats_equal_oracle, _bench_like_model, _build,
                         _calibrate, _calibrate_lightglue, _inputs, _np, _oracle_feats, _oracle_pair, _t, pkg)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CONV.cases))
def test_extractors_small_vs_oracle_and_golden(oracle, name):
    from test_oracle_golden import _check_feats
    c = CONV.cases[name]
    model, sd = _build(c, CONV)
    ev, mask, img = _inputs(c)
    img_t = _t(img)
    ef, imf, m = model(_t(ev), img_t, _t(mask))
    oef, oimf = _oracle_feats(oracle, c, sd, ev, mask, img, dense=True)
    _assert_feats_equal_oracle(ef, oef, dense=True)
    _assert_feats_equal_oracle(imf, oimf, dense=True)
    if c["cfg"]["image_extractor"]["type"] == "superpointv1":
        assert np.array_equal(_np(img_t), img / np.float32(255.0))  # in-place `image /= 255` quirk
    else:
        assert np.array_equal(_np(img_t), img)
    # and against the reference's own outputs
    as_np = lambda f: {k: (_np(v) if torch.is_tensor(v) else [_np(t) for t in v]) for k, v in f.items()}  # noqa: E731
    _check_feats(f"{name}.ev", as_np(ef), CONV)
    _check_feats(f"{name}.im", as_np(imf), CONV)
    # key set of the output dict (reference: 13 keys for cell-8 nets, 12 for cell-1 nets)
    import json
    assert sorted(ef.keys()) == json.loads(bytes(CONV[f"{name}.ev.keys"]).decode())
    assert sorted(imf.keys()) == json.loads(bytes(CONV[f"{name}.im.keys"]).decode())


@pytest.mark.parametrize("name", ["sp_mnn", "sp_mnn16", "silk_mnn"])
def test_e2e_full_size(oracle, name):
    from test_oracle_golden import _check_feats
    c = E2E.cases[name]
    model, sd = _build(c, E2E)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    ev, mask, img = _inputs(c)
    ef, imf, m = model(_t(ev), _t(img), _t(mask))
    oef, oimf = _oracle_feats(oracle, c, sd, ev, mask, img)
    _assert_feats_equal_oracle(ef, oef)
    _assert_feats_equal_oracle(imf, oimf)
    as_np = lambda f: {k: (_np(v) if torch.is_tensor(v) else [_np(t) for t in v]) for k, v in f.items()}  # noqa: E731
    _check_feats(f"{name}.ev", as_np(ef), E2E)
    _check_feats(f"{name}.im", as_np(imf), E2E)
    # matcher: bit-exact against the oracle on the same descriptors; against the reference up to
    # arg-max near-ties (checked with margins in test_oracle_golden.py::test_e2e_full_size)
    for b in range(c["B"]):
        exp = oracle.mnn(oef["sparse_descriptors"][b], oimf["sparse_descriptors"][b])
        assert np.array_equal(_np(m["matches0"][b])[0], exp["matches0"])
        assert np.array_equal(_np(m["matches1"][b])[0], exp["matches1"])
        assert np.array_equal(_np(m["matching_scores0"][b])[0], exp["matching_scores0"])
        mk0, mk1 = oracle.matched_kpts(oef["sparse_positions"][b], oimf["sparse_positions"][b], exp["matches0"], 3)
        assert np.array_equal(_np(m["matched_kpts0"][b]), mk0)
        assert np.array_equal(_np(m["matched_kpts1"][b]), mk1)
        np.testing.assert_allclose(_np(m["log_assignment"][b])[0], exp["log_assignment"], atol=1e-5, rtol=0)
    # against the reference: equal, except at rows where the reference differs from ITSELF (recorded from the reference,
    # tests/golden/mnnstab.npz), and there the value must be one its own alternative evaluations gave.  No tolerance, no budget.
    for key in ("matches0", "matches1"):
        got = np.concatenate([_np(m[key][b])[0] for b in range(c["B"])])
        check_matches_vs_reference(f"e2e.{name}.{key} vs reference", name, key, got, E2E[f"{name}.m.{key}"])


# ------------------------------------------------------------------ size-independent properties at bench size
def test_properties_at_bench_batch():
    c = dict(E2E.cases["sp_mnn"])
    model, _ = _build(c, E2E)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    B = 32
    ev, mask = synth.synth_events(500, B, 5)
    img = synth.synth_image(500, B)
    ef, imf, m = model(_t(ev), _t(img), _t(mask))
    from importlib import import_module
    du = import_module(pkg.__name__ + ".core.modules.utils.detector_util")
    for feats in (ef, imf):
        nms = feats["nms"]
        again = du.fast_nms(nms[:, None].contiguous(), 4)
        assert torch.equal(again[:, 0], nms)  # NMS is idempotent on its own output
        for b in range(B):
            p = _np(feats["sparse_positions"][b])
            assert 0 < p.shape[0] <= 1024
            flat = (p[:, 0] - 0.5) * 346 + (p[:, 1] - 0.5)
            assert np.all(np.diff(flat) > 0)  # raster order
            assert p[:, 0].min() >= 2 and p[:, 0].max() <= 258 and p[:, 1].min() >= 1 and p[:, 1].max() <= 345  # border 4 - pad
            yy, xx = p[:, 0], p[:, 1]
            dy = np.abs(yy[:, None] - yy[None]); dx = np.abs(xx[:, None] - xx[None])
            close = (np.maximum(dy, dx) <= 4) & ~np.eye(len(p), dtype=bool)
            assert not close.any()  # no two survivors within the NMS window
            d = _np(feats["sparse_descriptors"][b])
            np.testing.assert_allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-5)
    for b in range(B):
        m0, m1 = _np(m["matches0"][b])[0], _np(m["matches1"][b])[0]
        sel = np.nonzero(m0 > -1)[0]
        assert np.array_equal(m1[m0[sel]], sel)  # mutual consistency
        assert (m0 > -1).sum() == (m1 > -1).sum() == m["matched_kpts0"][b].shape[0]
    # batch invariance: pair 7 alone gives the same bits as pair 7 inside the batch
    ef1, imf1, m1_ = model(_t(ev[7:8]), _t(img[7:8]), _t(mask[7:8]))
    assert torch.equal(ef1["sparse_positions"][0], ef["sparse_positions"][7])
    assert torch.equal(imf1["sparse_descriptors"][0], imf["sparse_descriptors"][7])
    assert torch.equal(m1_["matches0"][0], m["matches0"][7])


@pytest.mark.parametrize("name", ["sp_lg", "silk_lg"])
def test_e2e_lightglue(oracle, name):
    """EIM.forward with the LightGlue matcher at 346x260: SuperPoint-shaped 256-d descriptors, and the SiLK family's 128-d
    descriptors through LightGlue's input_proj (configs/model/test/EI_SiLK_LG.yaml, lightglue.py:451-454)."""
    c = E2E.cases[name]
    model, sd = _build(c, E2E)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    ev, mask, img = _inputs(c)
    ef, imf, m = model(_t(ev), _t(img), _t(mask))
    oef, oimf = _oracle_feats(oracle, c, sd, ev, mask, img)
    _assert_feats_equal_oracle(ef, oef)
    _assert_feats_equal_oracle(imf, oimf)
    for key in ("matches0", "matches1"):
        exp = split(E2E[f"{name}.m.{key}"], E2E[f"{name}.m.{key}.lens"])
        for b in range(c["B"]):
            assert record_flips(f"e2e.{name}.{key} vs reference", _np(m[key][b])[0], exp[b]) == 0, key
    for key in ("matched_kpts0", "matched_kpts1"):
        exp = split(E2E[f"{name}.m.{key}"], E2E[f"{name}.m.{key}.lens"])
        for b in range(c["B"]):
            assert tuple(m[key][b].shape) == exp[b].shape  # [M,2] for LightGlue
            np.testing.assert_allclose(_np(m[key][b]), exp[b], atol=FTOL)
    for key in ("matching_scores0", "matching_scores1"):
        exp = split(E2E[f"{name}.m.{key}"], E2E[f"{name}.m.{key}.lens"])
        for b in range(c["B"]):
            close_and_record(f"e2e.{name}.{key} vs reference", _np(m[key][b])[0], exp[b], atol=FTOL)
    for b in range(c["B"]):
        la = _np(m["log_assignment"][b])
        assert list(la.shape) == E2E[f"{name}.m.la_shapes"][b].tolist()
        # the gate: identical inputs (the GPU extractors are bit-equal to the oracle's) -> 2 x the reference's own noise floor
        o = oracle.lightglue(sub_dict(sd, "matcher.matcher."), oef["sparse_positions"][b], oef["sparse_descriptors"][b],
                             oimf["sparse_positions"][b], oimf["sparse_descriptors"][b])
        close_and_record(f"e2e.{name}.log_assignment vs oracle", la[0], o["log_assignment"], atol=la_bound(f"e2e.{name}"))
        # recorded, not gated: end to end against the reference (its extractors' floats differ upstream by ~1e-6)
        up = upstream_deviation([(f"{name}.ev", oef), (f"{name}.im", oimf)], E2E)
        record_only(f"e2e.{name}.log_assignment vs reference (recorded)", la[0, ::97, ::89][:8, :8], E2E[f"{name}.m.la_probe"][b],
                    la_bound_e2e(f"e2e.{name}", up))


@pytest.mark.parametrize("name", list(LGCAL.cases))
def test_e2e_lightglue_same_scene(oracle, name):
    """Round 4: EIM.forward + LightGlue in a NON-degenerate regime ("same scene" pairs, calibrated assignment head; fixtures
    generated from the reference, tests/golden/lgcal.npz): 750-790 matches per pair, matching_scores spread over 0.003 .. 0.95.
    Extractors bit-equal to the oracle; assignments equal to the reference AND to the oracle (flip counts recorded);
    matching_scores to 1e-4; log_assignment to the noise-floor-derived bounds, also against the reference in float64."""
    c = LGCAL.cases[name]
    cfg = pkg.configs.to_attr(c["cfg"])
    model = pkg.EIM(cfg, device=DEV)
    sd = twin_state_dict_for(c, LGCAL)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("descriptor_scale_factor") for k in missing), (missing, unexpected)
    model.eval()
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    ev, mask, img = twin_inputs(c)
    ef, imf, m = model(_t(ev), _t(img), _t(mask))
    oef, oimf = _oracle_feats(oracle, c, sd, ev, mask, img)
    _assert_feats_equal_oracle(ef, oef)
    _assert_feats_equal_oracle(imf, oimf)
    for b in range(c["B"]):
        nf = lg_noise(f"{name}.{b}")
        o = oracle.lightglue(sub_dict(sd, "matcher.matcher."), oef["sparse_positions"][b], oef["sparse_descriptors"][b],
                             oimf["sparse_positions"][b], oimf["sparse_descriptors"][b])
        for key in ("matches0", "matches1"):
            exp = split(LGCAL[f"{name}.m.{key}"], LGCAL[f"{name}.m.{key}.lens"])[b]
            got = _np(m[key][b])[0]
            assert record_flips(f"lgcal.{name}.{key} vs reference", got, exp) == 0, f"pair {b}: {key}"
            la_o = o["log_assignment"] if key == "matches0" else o["log_assignment"].T
            assert record_flips(f"lgcal.{name}.{key} vs oracle", got, np.asarray(o[key]).reshape(-1), la_o) == 0, f"pair {b}: {key}"
        assert int((_np(m["matches0"][b]) > -1).sum()) == nf["matches"] >= 100
        for key in ("matching_scores0", "matching_scores1"):
            exp = split(LGCAL[f"{name}.m.{key}"], LGCAL[f"{name}.m.{key}.lens"])[b]
            close_and_record(f"lgcal.{name}.{key} vs reference", _np(m[key][b])[0], exp, atol=FTOL)
            close_and_record(f"lgcal.{name}.{key} vs oracle", _np(m[key][b])[0], np.asarray(o[key]).reshape(-1), atol=FTOL)
        close_and_record(f"lgcal.{name}.matching_scores0 vs reference in float64", _np(m["matching_scores0"][b])[0],
                         LGCAL[f"{name}.m.matching_scores0_f64.{b}"], atol=FTOL)
        for key in ("matched_kpts0", "matched_kpts1"):
            exp = split(LGCAL[f"{name}.m.{key}"], LGCAL[f"{name}.m.{key}.lens"])[b]
            assert tuple(m[key][b].shape) == exp.shape
            np.testing.assert_allclose(_np(m[key][b]), exp, atol=FTOL)
        la = _np(m["log_assignment"][b])
        assert list(la.shape) == LGCAL[f"{name}.m.la_shapes"][b].tolist()
        # identical inputs (the GPU extractors are bit-equal to the oracle's): 2 x the reference's own noise floor
        close_and_record(f"lgcal.{name}.log_assignment vs oracle", la[0], o["log_assignment"], atol=la_bound(f"{name}.{b}"))
        # recorded, not gated: end to end against the reference (extractor floats differ by ~1e-6 upstream)
        up = upstream_deviation([(f"{name}.ev", oef), (f"{name}.im", oimf)], LGCAL)
        record_only(f"lgcal.{name}.log_assignment vs reference (recorded)", la[0, ::31, ::29], LGCAL[f"{name}.m.la_probe2"][b],
                    la_bound_e2e(f"{name}.{b}", up))
        record_only(f"lgcal.{name}.log_assignment vs reference in float64 (recorded)", la[0, ::31, ::29], LGCAL[f"{name}.m.la_probe2_f64.{b}"],
                    la_bound_e2e(f"{name}.{b}", up))


# ------------------------------------------------------------------ other front doors and edge cases
def test_image_image_matcher_and_build_model(oracle):
    """ImageImageMatcher (core/modules/ImageImageMatcher.py) through build_model; both sides use the
    image extractor; first image takes a mask."""
    c = E2E.cases["sp_mnn"]
    cfg = pkg.configs.to_attr(c["cfg"])
    cfg.name = "ImageImageMatcher"
    model = pkg.build_model(cfg, DEV, None)
    sd = {k: v for k, v in state_dict_for(c, E2E).items() if not k.startswith("event_extractor")}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    model.eval()
    for ext in (model.image_extractor.extractor,):
        ext.dense_outputs = False
    img0 = synth.synth_image(31, 2, 100, 124)
    img1 = synth.synth_image(32, 2, 100, 124)
    mask0 = synth.uniform01(33, (2, 1, 100, 124)) < np.float32(0.7)
    f0, f1, m = model(_t(img0), _t(img1), mask=_t(mask0))
    sub = sub_dict(sd, "image_extractor.extractor.")
    o0 = oracle.extractor_forward("superpointv1", sub, img0.copy(), mask0, top_k=1024)
    o1 = oracle.extractor_forward("superpointv1", sub, img1.copy(), None, top_k=1024)
    _assert_feats_equal_oracle(f0, o0)
    _assert_feats_equal_oracle(f1, o1)
    for b in range(2):
        exp = oracle.mnn(o0["sparse_descriptors"][b], o1["sparse_descriptors"][b], want_la=False)
        assert np.array_equal(_np(m["matches0"][b])[0], exp["matches0"])


def test_small_helper_functions(oracle):
    """logits_to_prob / depth_to_space / remove_border_points / get_dense_* with the reference's
    signatures (silk magicpoint_test.py:60-101 properties: softmax sums to one, score shape)."""
    from importlib import import_module
    du = import_module(pkg.__name__ + ".core.modules.utils.detector_util")
    dd = import_module(pkg.__name__ + ".core.modules.utils.descriptor_util")
    logits = synth.normalish(5, (3, 65, 16, 16))
    prob = du.logits_to_prob(_t(logits))
    eprob, escore = oracle.logits_to_score(logits)
    assert np.array_equal(_np(prob), eprob)
    np.testing.assert_allclose(_np(prob).sum(1), 1.0, atol=1e-6)
    score = du.depth_to_space(prob, cell_size=8)
    assert tuple(score.shape) == (3, 1, 128, 128)
    assert np.array_equal(_np(score), escore)
    l1 = synth.normalish(6, (2, 1, 20, 24))
    p1 = du.logits_to_prob(_t(l1))
    assert np.array_equal(_np(p1), oracle.logits_to_score(l1)[0])
    assert du.depth_to_space(p1, cell_size=1) is p1  # cell-1: the same tensor (reference aliasing)
    m = _t(synth.uniform01(7, (1, 1, 8, 8)))
    assert not _np(du.remove_border_points(m, 4)).any()  # silk utils_test.py:17-29
    dpos = du.get_dense_positions(score, ordering="yx")
    assert tuple(dpos.shape) == (3, 128 * 128, 3)
    assert _np(dpos[0, 129]).tolist()[:2] == [1.5, 1.5] and float(dpos[1, 5, 2]) == float(score[1, 0, 0, 5])
    nd = dd.normalize_descriptors(_t(synth.normalish(8, (2, 16, 4, 5))), 1.0)
    assert tuple(dd.get_dense_descriptors(nd).shape) == (2, 20, 16)


def _every_pair_equals_its_own_forward(model, ev_t, img_t, mask_t, ef, imf, m):
    """pair b of the batched forward, for EVERY b, is bit-identical to the forward of pair b alone (keypoints, descriptors,
    matches, matched keypoints, matching scores, log_assignment): the XCD remap, the persistent tile walk and the stacked 2B layout
    may not depend on a pair's place in the batch"""
    for b in range(ev_t.shape[0]):
        ef1, imf1, m1 = model(ev_t[b:b + 1], img_t[b:b + 1].clone(), mask_t[b:b + 1])
        for got, one in ((ef, ef1), (imf, imf1)):
            assert torch.equal(got["sparse_positions"][b], one["sparse_positions"][0]), f"pair {b}: keypoints"
            assert torch.equal(got["sparse_descriptors"][b], one["sparse_descriptors"][0]), f"pair {b}: descriptors"
        for k in ("matches0", "matches1", "matched_kpts0", "matched_kpts1", "matching_scores0", "matching_scores1", "log_assignment"):
            a, o = m[k][b], m1[k][0]
            assert (a is None) == (o is None), f"pair {b}: {k}"
            assert a is None or torch.equal(a, o), f"pair {b}: {k}"


@pytest.mark.parametrize("cfg_name,B", [("SP_MNN", 32), ("SiLK_MNN", 32)])
def test_baseline_batch_sampled_pairs_vs_oracle_mnn(oracle, cfg_name, B):
    """configs[1] / configs[2] at their real batch size: pairs 0, B/2, B-1 bit-equal to per-pair oracle runs
    (keypoints + scores, descriptors, match indices, matched keypoints)."""
    cfg, model, sd = _bench_like_model(cfg_name)
    ev, mask = synth.synth_events(10_000, B, 5)
    img = synth.synth_image(10_000, B)
    ev_t, mask_t, img_t = _t(ev), _t(mask), _t(img)
    _calibrate(model, sd, ev_t, img_t, mask_t)
    ef, imf, m = model(ev_t, img_t.clone(), mask_t)
    nmatch = []
    for b in (0, B // 2, B - 1):
        oe, oi = _oracle_pair(oracle, cfg, sd, ev, mask, img, b)
        for got, exp in ((ef, oe), (imf, oi)):
            assert np.array_equal(_np(got["sparse_positions"][b]), exp["sparse_positions"][0]), f"pair {b}: keypoints"
            assert np.array_equal(_np(got["sparse_descriptors"][b]), exp["sparse_descriptors"][0]), f"pair {b}: descriptors"
        r = oracle.mnn(oe["sparse_descriptors"][0], oi["sparse_descriptors"][0], want_la=False)
        assert np.array_equal(_np(m["matches0"][b])[0], r["matches0"]), f"pair {b}: matches0"
        assert np.array_equal(_np(m["matches1"][b])[0], r["matches1"]), f"pair {b}: matches1"
        mk0, mk1 = oracle.matched_kpts(oe["sparse_positions"][0], oi["sparse_positions"][0], r["matches0"], 3)
        assert np.array_equal(_np(m["matched_kpts0"][b]), mk0) and np.array_equal(_np(m["matched_kpts1"][b]), mk1)
        nmatch.append(int((r["matches0"] > -1).sum()))
    assert min(nmatch) >= 5, f"calibrated descriptors should give real matches, got {nmatch}"
    _every_pair_equals_its_own_forward(model, ev_t, img_t, mask_t, ef, imf, m)


@pytest.mark.parametrize("cfg_name", ["SP_MNN", "SP_LG"])
def test_pair_without_events_gives_the_reference_empty_dict_and_leaves_the_batch_alone(cfg_name):
    """A pair whose events mask is empty has no event keypoints (score[~mask] = 0, EventExtractors.py:561-562): the matcher
    returns the reference's empty-input dict for THAT pair (MNN.py:63-86 / lightglue.py:572-591: matches of length 0 / m, no
    matched keypoints, zero log_assignment [1,1,m+1]) and the other pairs of the batch are exactly what they are alone."""
    cfg, model, sd = _bench_like_model(cfg_name)
    B = 3
    ev, mask = synth.synth_events(777, B, 5)
    img = synth.synth_image(777, B)
    ev[1] = 0.0
    mask[1] = False
    ef, imf, m = model(_t(ev), _t(img), _t(mask))
    assert ef["sparse_positions"][1].shape == (0, 3) and ef["sparse_descriptors"][1].shape == (0, 256)
    mi = imf["sparse_positions"][1].shape[0]
    assert mi > 0
    assert tuple(m["matches0"][1].shape) == (1, 0) and tuple(m["matches1"][1].shape) == (1, mi)
    assert bool((m["matches1"][1] == -1).all()) and float(m["matching_scores1"][1].abs().max()) == 0.0
    assert tuple(m["matched_kpts0"][1].shape) == (0, 3) and tuple(m["matched_kpts1"][1].shape) == (0, 3)
    la = m["log_assignment"][1]
    assert tuple(la.shape) == (1, 1, mi + 1) and float(la.abs().max()) == 0.0
    for b in (0, 2):
        ef1, imf1, m1 = model(_t(ev[b:b + 1]), _t(img[b:b + 1]), _t(mask[b:b + 1]))
        assert torch.equal(ef1["sparse_positions"][0], ef["sparse_positions"][b])
        assert torch.equal(imf1["sparse_descriptors"][0], imf["sparse_descriptors"][b])
        assert torch.equal(m1["matches0"][0], m["matches0"][b])
        assert torch.equal(m1["matched_kpts0"][0], m["matched_kpts0"][b])


def test_other_geometry_vga_16_bins_vs_oracle(oracle):
    """Nothing is specialised to 346x260 / 5 bins: one 640x480 pair with the reference's shipped 16 event bins (N = 307,200 score
    pixels: the generic selection path, 60x80 heads, other conv tile choices) bit-equal to the oracle end to end."""
    cfg = pkg.default_config("SP_MNN", event_channels=16)
    model = pkg.EIM(cfg, device=DEV).eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=17)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    H, W = 480, 640
    ev, mask = synth.synth_events(4321, 1, 16, H, W)
    img = synth.synth_image(4321, 1, H, W)
    ef, imf, m = model(_t(ev), _t(img), _t(mask))
    oe = oracle.extractor_forward("vgg", sub_dict(sd, "event_extractor.extractor."), ev.copy(), mask, top_k=1024)
    oi = oracle.extractor_forward("superpointv1", sub_dict(sd, "image_extractor.extractor."), img.copy(), None, top_k=1024)
    for got, exp in ((ef, oe), (imf, oi)):
        assert np.array_equal(_np(got["sparse_positions"][0]), exp["sparse_positions"][0])
        assert np.array_equal(_np(got["sparse_descriptors"][0]), exp["sparse_descriptors"][0])
        assert np.array_equal(_np(got["score"]), exp["score"])
    r = oracle.mnn(oe["sparse_descriptors"][0], oi["sparse_descriptors"][0], want_la=False)
    assert np.array_equal(_np(m["matches0"][0])[0], r["matches0"])
    assert 0 < ef["sparse_positions"][0].shape[0] <= 1024 and tuple(ef["score"].shape) == (1, 1, H, W)


def test_shipped_16_bin_config_at_bench_batch_vs_per_pair_oracle(oracle):
    """The reference's model YAMLs ship `in_channels: 16` (configs/model/SP_MNN.yaml:12,24; BASELINE.json's bench shape uses 5):
    B = 32 pairs of 346x260 with 16 event bins, pairs 0 / 16 / 31 bit-equal to per-pair oracle runs (keypoints + scores,
    descriptors, match indices) -- the first event layer then stages 16 channels in two chunks instead of one thin one."""
    B = 32
    cfg, model, sd = _bench_like_model("SP_MNN", seed=19, event_channels=16)
    ev, mask = synth.synth_events(16_000, B, 16)
    img = synth.synth_image(16_000, B)
    ev_t, mask_t, img_t = _t(ev), _t(mask), _t(img)
    _calibrate(model, sd, ev_t, img_t, mask_t)
    ef, imf, m = model(ev_t, img_t.clone(), mask_t)
    assert tuple(ef["backbone_feats"].shape) == (B, 128, 33, 44)
    for b in (0, B // 2, B - 1):
        oe, oi = _oracle_pair(oracle, cfg, sd, ev, mask, img, b)
        for got, exp in ((ef, oe), (imf, oi)):
            assert np.array_equal(_np(got["sparse_positions"][b]), exp["sparse_positions"][0]), f"pair {b}: keypoints"
            assert np.array_equal(_np(got["sparse_descriptors"][b]), exp["sparse_descriptors"][0]), f"pair {b}: descriptors"
        r = oracle.mnn(oe["sparse_descriptors"][0], oi["sparse_descriptors"][0], want_la=False)
        assert np.array_equal(_np(m["matches0"][b])[0], r["matches0"]), f"pair {b}: matches0"
        assert np.array_equal(_np(m["matches1"][b])[0], r["matches1"]), f"pair {b}: matches1"
    _every_pair_equals_its_own_forward(model, ev_t, img_t, mask_t, ef, imf, m)


@pytest.mark.parametrize("cfg_name,bins", [("SP_MNN", 5), ("SP_LG", 16), ("SiLK_MNN", 5)])
def test_ec_sensor_geometry_240x180_vs_oracle(oracle, cfg_name, bins):
    """The reference's second sensor: ECDataset.RESOLUTION = (240, 180) (datasets/EC.py:125; MVSEC is 346x260).  180 is not a
    multiple of 8: the Padder adds 4 rows (2 + 2), 240 columns need none -- 184x240 padded maps, 23x30 heads, N = 43,200 score
    pixels.  Two pairs per forward, every extractor output and the MNN matches bit-equal to the oracle; LightGlue: assignments
    equal, scores within 1e-4."""
    H, W, B = 180, 240, 2
    cfg, model, sd = _bench_like_model(cfg_name, seed=23, event_channels=bins)
    ev, mask = synth.synth_events(2400 + bins, B, bins, H, W)
    img = synth.synth_image(2400 + bins, B, H, W)
    ev_t, mask_t, img_t = _t(ev), _t(mask), _t(img)
    _calibrate(model, sd, ev_t, img_t, mask_t)
    ef, imf, m = model(ev_t, img_t.clone(), mask_t)
    assert tuple(ef["score"].shape) == (B, 1, H, W) and tuple(ef["nms"].shape) == (B, H, W)
    et, it = cfg.event_extractor.type, cfg.image_extractor.type
    for b in range(B):
        oe, oi = _oracle_pair(oracle, cfg, sd, ev, mask, img, b)
        for got, exp in ((ef, oe), (imf, oi)):
            assert np.array_equal(_np(got["score"][b:b + 1]), exp["score"]), f"pair {b}: score map"
            assert np.array_equal(_np(got["nms"][b:b + 1]), exp["nms"]), f"pair {b}: nms map"
            assert np.array_equal(_np(got["sparse_positions"][b]), exp["sparse_positions"][0]), f"pair {b}: keypoints"
            assert np.array_equal(_np(got["sparse_descriptors"][b]), exp["sparse_descriptors"][0]), f"pair {b}: descriptors"
        if cfg.matcher.type == "MNN":
            r = oracle.mnn(oe["sparse_descriptors"][0], oi["sparse_descriptors"][0], want_la=False)
            assert np.array_equal(_np(m["matches0"][b])[0], r["matches0"]) and np.array_equal(_np(m["matches1"][b])[0], r["matches1"])
        else:
            r = oracle.lightglue(sub_dict(sd, "matcher.matcher."), oe["sparse_positions"][0], oe["sparse_descriptors"][0],
                                 oi["sparse_positions"][0], oi["sparse_descriptors"][0], size0=(H, W), size1=(H, W))
            assert np.array_equal(_np(m["matches0"][b])[0], np.asarray(r["matches0"]).reshape(-1))
            close_and_record("EC 240x180 sp_lg matching_scores0 vs oracle", _np(m["matching_scores0"][b])[0], np.asarray(r["matching_scores0"]).reshape(-1), atol=1e-4)


def test_baseline_batch_sampled_pairs_vs_oracle_lightglue(oracle):
    """configs[3]: B=64 SP+LightGlue on "same scene" pairs with a calibrated assignment head (hundreds of confident matches per
    pair, synth.twin_overrides / lightglue_calibration): extractor outputs bit-equal, match assignments equal (flips are counted
    and reported; target 0), matching scores to 1e-4, log_assignment to a multiple of the reference's own noise floor."""
    B = 64
    cfg, model, sd = _bench_like_model("SP_LG")
    tw = synth.twin_overrides(sd)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in tw.items()}, strict=False)
    sd.update(tw)
    ev, mask = synth.synth_events(10_000, B, 5)
    img = synth.synth_image(10_000, B)
    ev = synth.twin_events(ev, img)
    ev_t, mask_t, img_t = _t(ev), _t(mask), _t(img)
    _calibrate(model, sd, ev_t, img_t, mask_t)
    ef, imf, _ = model(ev_t, img_t.clone(), mask_t)
    _calibrate_lightglue(model, sd, ef, imf)
    ef, imf, m = model(ev_t, img_t.clone(), mask_t)
    bound = la_bound("sp_lg_twin.0")
    for b in (0, B // 2, B - 1):
        oe, oi = _oracle_pair(oracle, cfg, sd, ev, mask, img, b)
        for got, exp in ((ef, oe), (imf, oi)):
            assert np.array_equal(_np(got["sparse_positions"][b]), exp["sparse_positions"][0]), f"pair {b}: keypoints"
            assert np.array_equal(_np(got["sparse_descriptors"][b]), exp["sparse_descriptors"][0]), f"pair {b}: descriptors"
        r = oracle.lightglue(sub_dict(sd, "matcher.matcher."), oe["sparse_positions"][0], oe["sparse_descriptors"][0],
                             oi["sparse_positions"][0], oi["sparse_descriptors"][0])
        g0, e0 = _np(m["matches0"][b])[0], np.asarray(r["matches0"]).reshape(-1)
        assert int((e0 > -1).sum()) >= 100, f"pair {b}: the calibrated workload should match hundreds of keypoints, got {int((e0 > -1).sum())}"
        record_flips("B64 sp_lg (same scene) matches0 vs oracle", g0, e0, r["log_assignment"])
        # flash-style attention sums in a different order than the oracle: an assignment may differ ONLY at rows of the
        # allow-list built from the oracle's own decision margins (best minus second best of the row, or of the chosen column,
        # inside the same-input log_assignment bound); no count budget
        la = np.asarray(r["log_assignment"])[:-1, :-1]
        top2r = np.sort(la, axis=1)[:, -2:]
        top2c = np.sort(la, axis=0)[-2:, :]
        row_gap = top2r[:, 1] - top2r[:, 0]
        col_gap = top2c[1] - top2c[0]
        allow = {int(i) for i in np.nonzero((row_gap < bound) | (col_gap[np.argmax(la, axis=1)] < bound))[0]}
        bad = np.nonzero(g0 != e0)[0]
        assert {int(i) for i in bad} <= allow, f"pair {b}: rows {sorted({int(i) for i in bad} - allow)} differ outside the oracle's near-tie rows"
        gla = _np(m["log_assignment"][b])[0] if m["log_assignment"][b] is not None else None
        if gla is not None:
            close_and_record("B64 sp_lg (same scene) log_assignment vs oracle", gla[::53, ::47], r["log_assignment"][::53, ::47], atol=bound)
        es = np.asarray(r["matching_scores0"]).reshape(-1)
        assert es.max() > 0.9 and ((es > 0.1) & (es < 0.9)).sum() >= 100
        close_and_record("B64 sp_lg (same scene) matching_scores0 vs oracle", _np(m["matching_scores0"][b])[0], es, atol=1e-4)
        # the float64 forward on the GPU's own features (equal to the oracle's): GPU vs exact and oracle vs exact side by side
        pair = (oe["sparse_positions"][0], oe["sparse_descriptors"][0], oi["sparse_positions"][0], oi["sparse_descriptors"][0],
                (260, 346), (260, 346))
        got = {"la": gla, "layers": None, "m0": g0, "m1": _np(m["matches1"][b])[0], "s0": _np(m["matching_scores0"][b])[0],
               "s1": _np(m["matching_scores1"][b])[0]}
        _check_pair("lgf64.b64_sp_lg", sub_dict(sd, "matcher.matcher."), SHIPPED, pair, got, orc=r, fixture="sp_lg_twin.0")
    _every_pair_equals_its_own_forward(model, ev_t, img_t, mask_t, ef, imf, m)


@pytest.mark.parametrize("name", list(PAD0))
def test_padding0_networks_vs_oracle_and_reference(oracle, name):
    """SiLKModel(padding=0) / VGGExtractorNP(padding=0): un-padded convolutions + `mapping_positions` (+9)
    (silk_extractor.py:142-152, EventExtractors.py:319-329): bit-equal to the oracle, 1e-4 to the reference's arithmetic."""
    from helpers import state_dict_for
    from test_oracle_golden import _check_feats
    from test_r2_golden_cpu import _G
    c = PAD0[name]
    cfg = pkg.configs.to_attr(c["cfg"])
    model = pkg.EIM(cfg, device=DEV).eval()
    sd = state_dict_for(c)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    ev, mask = synth.synth_events(c["iseed"], c["B"], c["ce"], c["H"], c["W"])
    img = synth.synth_image(c["iseed"], c["B"], c["H"], c["W"])
    ef = model.event_extractor(_t(ev), None)
    img_t = _t(img)
    imf = model.image_extractor(img_t)
    assert np.array_equal(_np(img_t), img)  # SiLK leaves the caller's image untouched
    oe = oracle.extractor_forward("vgg_np", sub_dict(sd, "event_extractor.extractor."), ev.copy(), None, top_k=c["k"], scale=1.41,
                                  padding=0, dense=True)
    oi = oracle.extractor_forward("silk", sub_dict(sd, "image_extractor.extractor."), img.copy(), None, top_k=c["k"], scale=1.41,
                                  padding=0, dense=True)
    for got, exp in ((ef, oe), (imf, oi)):
        for k in ("backbone_feats", "logits", "raw_descriptors", "probability", "score", "nms", "normalized_descriptors"):
            assert np.array_equal(_np(got[k]), exp[k]), k
        for b in range(c["B"]):
            assert np.array_equal(_np(got["sparse_positions"][b]), exp["sparse_positions"][b])
            assert np.array_equal(_np(got["sparse_descriptors"][b]), exp["sparse_descriptors"][b])
        assert tuple(got["score"].shape) == (c["B"], 1, c["H"] - 18, c["W"] - 18)
        assert [tuple(_np(s)) for s in got["image_size"]] == [(c["H"], c["W"])] * c["B"]
    as_np = lambda f: {k: (_np(v) if torch.is_tensor(v) else [_np(t) for t in v]) for k, v in f.items()}  # noqa: E731
    _check_feats(f"{name}.ev", as_np(ef), _G())
    _check_feats(f"{name}.im", as_np(imf), _G())
    np.testing.assert_allclose(_np(ef["dense_positions"][0])[::97], _Z[f"{name}.ev.dense_positions_probe"], atol=1e-6)
    np.testing.assert_allclose(_np(imf["dense_positions"][0])[::97], _Z[f"{name}.im.dense_positions_probe"], atol=1e-6)
    assert float(ef["sparse_positions"][0][:, :2].min()) >= 9.0 + 4.0  # +9 mapping on top of the 4-pixel border
    with pytest.raises(RuntimeError, match="shape of the mask"):
        model.event_extractor(_t(ev), _t(mask))
    # the matcher consumes the mapped keypoints like any others
    m = model.matcher(ef, imf)
    exp = oracle.mnn(oe["sparse_descriptors"][0], oi["sparse_descriptors"][0], want_la=False)
    assert np.array_equal(_np(m["matches0"][0])[0], exp["matches0"])


# ------------------------------------------------------------------ EIM.forward's optional masks (EIM.py:44: events_mask=None, image_mask=None)
def test_eim_forward_without_masks_and_with_an_image_mask_vs_oracle(oracle):
    from helpers import sub_dict
    cfg = pkg.default_config("SP_MNN", event_channels=5)
    for sec in (cfg.event_extractor.vgg, cfg.image_extractor.superpointv1):
        sec.detection_top_k = 150
    model = pkg.EIM(cfg, device=DEV).eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=17)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    H, W, B = 84, 108, 2
    ev, emask = synth.synth_events(91, B, 5, H, W)
    img = synth.synth_image(91, B, H, W)
    imask = synth.uniform01(92, (B, 1, H, W)) < np.float32(0.6)
    esub, isub = sub_dict(sd, "event_extractor.extractor."), sub_dict(sd, "image_extractor.extractor.")
    for em, im in ((None, None), (emask, imask), (None, imask)):
        ef, imf, m = model(_t(ev), _t(img), None if em is None else _t(em), None if im is None else _t(im))
        oe = oracle.extractor_forward("vgg", esub, ev.copy(), em, top_k=150)
        oi = oracle.extractor_forward("superpointv1", isub, img.copy(), im, top_k=150)
        for got, exp in ((ef, oe), (imf, oi)):
            assert np.array_equal(got["score"].cpu().numpy(), exp["score"])
            assert np.array_equal(got["nms"].cpu().numpy(), exp["nms"])
            for b in range(B):
                assert np.array_equal(got["sparse_positions"][b].cpu().numpy(), exp["sparse_positions"][b])
                assert np.array_equal(got["sparse_descriptors"][b].cpu().numpy(), exp["sparse_descriptors"][b])
        for b in range(B):
            r = oracle.mnn(oe["sparse_descriptors"][b], oi["sparse_descriptors"][b], want_la=False)
            assert np.array_equal(m["matches0"][b].cpu().numpy()[0], r["matches0"])
        if im is not None:  # the image-side mask zeroes scores exactly where it is False (no dilation on the image side)
            assert float(imf["score"][~_t(im)].abs().max()) == 0.0


# ------------------------------------------------------------------ whole forwards at odd geometries (small-grid kernels, forked heads, ragged tiles)
@pytest.mark.parametrize("cfg_name,B,H,W,bins,k", [
    ("SP_MNN", 1, 41, 67, 5, 64), ("SP_MNN", 2, 97, 53, 3, 200), ("SP_MNN", 3, 64, 136, 16, 128), ("SP_MNN", 1, 135, 181, 5, 500),
    ("SiLK_MNN", 1, 37, 45, 5, 80), ("SiLK_MNN", 2, 58, 83, 2, 150),
], ids=lambda v: str(v))
def test_whole_forward_at_odd_geometries_vs_oracle(oracle, cfg_name, B, H, W, bins, k):
    """Single pairs and tiny batches at sizes that are not multiples of the cell / tile sizes: every launch takes a small-grid
    path (conv16_kernel, conv16_1x1_kernel, forked head branches) with ragged tiles; keypoints, descriptors and matches must
    equal per-pair oracle runs bit for bit."""
    from helpers import sub_dict
    cfg = pkg.default_config(cfg_name, event_channels=bins)
    et, it = cfg.event_extractor.type, cfg.image_extractor.type
    cfg.event_extractor[et].detection_top_k = k
    cfg.image_extractor[it].detection_top_k = k
    model = pkg.EIM(cfg, device=DEV).eval()
    sd = synth.synth_state_dict([(kk, tuple(v.shape)) for kk, v in model.state_dict().items()], seed=H * 7 + W)
    model.load_state_dict({kk: torch.from_numpy(v) for kk, v in sd.items()}, strict=False)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    ev, mask = synth.synth_events(H + W, B, bins, H, W)
    img = synth.synth_image(H + W, B, H, W)
    ef, imf, m = model(_t(ev), _t(img), _t(mask))
    oe = oracle.extractor_forward(et, sub_dict(sd, "event_extractor.extractor."), ev.copy(), mask, top_k=k,
                                  scale=cfg.event_extractor[et].descriptor_scale_factor)
    oi = oracle.extractor_forward(it, sub_dict(sd, "image_extractor.extractor."), img.copy(), None, top_k=k,
                                  scale=cfg.image_extractor[it].descriptor_scale_factor)
    for got, exp in ((ef, oe), (imf, oi)):
        for key in ("backbone_feats", "logits", "raw_descriptors", "score", "nms"):
            assert np.array_equal(got[key].cpu().numpy(), exp[key]), key
        for b in range(B):
            assert np.array_equal(got["sparse_positions"][b].cpu().numpy(), exp["sparse_positions"][b])
            assert np.array_equal(got["sparse_descriptors"][b].cpu().numpy(), exp["sparse_descriptors"][b])
    for b in range(B):
        if len(oe["sparse_descriptors"][b]) == 0 or len(oi["sparse_descriptors"][b]) == 0:
            continue
        r = oracle.mnn(oe["sparse_descriptors"][b], oi["sparse_descriptors"][b], want_la=False)
        assert np.array_equal(m["matches0"][b].cpu().numpy()[0], r["matches0"])
