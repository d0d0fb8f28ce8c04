"""CPU-only: sub-pixel keypoints where no device is needed -- the refinement rule's restatement in float32 and
float64, the clamp and the floor invariant, the blob scene on the restatement, the restated sampler against the pixel-centre
statement, the new symbols and the Python switch."""
from importlib import import_module

import numpy as np
import pytest
import torch

import extract_ref as er
import subpixel_ref as S
from helpers import load_pkg, synth

pkg = load_pkg()
N = pkg.native
EX = import_module(pkg.__name__ + "._extract")
BASE = import_module(pkg.__name__ + ".core.modules._base")
dd = import_module(pkg.__name__ + ".core.modules.utils.descriptor_util")


def test_exact_quadratics_agree_between_float32_and_float64():
    """dyadic coefficients: every intermediate but the quotient is exact in both formats; 1/6 differs by its rounding only"""
    d32, d64 = S.offset(0.5, 1.0, 0.75, np.float32), S.offset(0.5, 1.0, 0.75, np.float64)
    assert d64 == 0.5 * (0.5 - 0.75) / ((0.5 - 1.0) + (0.75 - 1.0)) == 1.0 / 6.0
    assert abs(float(d32) - float(d64)) <= float(np.spacing(np.float32(1.0 / 6.0)))
    for l, r, exp in ((0.25, 0.75, 0.25), (0.75, 0.25, -0.25), (0.5, 0.5, 0.0), (0.875, 0.625, -0.25)):  # dyadic quotients: exact
        a, b = S.offset(l, 1.0, r, np.float32), S.offset(l, 1.0, r, np.float64)
        assert float(a) == float(b) == exp, (l, r)
    a, b = S.offset(0.0, 1.0, 0.5, np.float32), S.offset(0.0, 1.0, 0.5, np.float64)  # 0.5 * (-0.5) / (-1.5)
    assert float(b) == 1.0 / 6.0 and abs(float(a) - float(b)) <= float(np.spacing(np.float32(1.0 / 6.0)))


def test_rule_gives_zero_without_a_strict_maximum_and_clamps():
    nan = np.nan
    for l, c, r in ((1.0, 1.0, 0.5), (0.5, 1.0, 1.0), (1.0, 1.0, 1.0), (0.75, 0.5, 0.25), (nan, 1.0, 0.5), (0.5, 1.0, nan), (0.5, nan, 0.5),
                    (0.5, 0.25, 0.5)):
        for dt in (np.float32, np.float64):
            assert float(S.offset(l, c, r, dt)) == 0.0, (l, c, r)
    big = 1.0 - 2.0 ** -12
    for dt in (np.float32, np.float64):
        assert float(S.offset(big, 1.0, 0.0, dt)) == -S.DMAX and float(S.offset(0.0, 1.0, big, dt)) == S.DMAX
        assert abs(0.5 * big / (1 + 2.0 ** -12)) > S.DMAX  # the unclamped vertex lies beyond the clamp


def test_clamp_constant_and_floor_invariant():
    assert S.DMAX == 0.5 - 2.0 ** -10 and float(np.float32(S.DMAX)) == S.DMAX
    assert N.SUBPIXEL_DMAX == S.DMAX
    for y in (0, 1, 255, 4095, 8191):
        for d in (S.DMAX, -S.DMAX):
            p = (np.float32(y) + np.float32(0.5)) + np.float32(d)
            assert p.dtype == np.float32 and float(np.floor(p)) == float(y), (y, d, p)
    # why a clamp below 0.5 at all: an offset of 0.5 - 2^-13 already rounds up to the next pixel in the last row of the largest map
    near = np.float32(0.5 - 2.0 ** -13)
    assert float(np.floor((np.float32(S.MAX_SIDE - 1) + np.float32(0.5)) + near)) == float(S.MAX_SIDE)


def test_refine_restatement_on_the_constructed_case():
    s, idx, counts, facts = S.refine_case()
    pos, padded, off = S.refine(s[0], idx[0], S.REFINE_PADS, np.float32)
    pos64, _, off64 = S.refine(s[0], idx[0], S.REFINE_PADS, np.float64)
    Hp, Wp = S.REFINE_MAP
    y, x = idx[0] // Wp, idx[0] % Wp
    k = facts["dyadic"]
    assert float(off[k, 0]) == 0.25 and abs(float(off[k, 1]) - 1.0 / 6.0) < 1e-7
    for name in ("tie", "corner", "corner0", "no_max", "valley"):
        assert np.all(off[facts[name]] == 0.0), name
    assert float(off[facts["row0"], 0]) == 0.0 and float(off[facts["row0"], 1]) != 0.0
    assert float(off[facts["col0"], 1]) == 0.0 and float(off[facts["col0"], 0]) != 0.0
    assert float(off[facts["last_row"], 0]) == 0.0 and float(off[facts["last_row"], 1]) != 0.0
    assert float(off[facts["last_col"], 1]) == 0.0 and float(off[facts["last_col"], 0]) != 0.0
    assert float(off[facts["nan"], 1]) == 0.0 and float(off[facts["nan"], 0]) != 0.0
    assert float(off[facts["clamp_neg"], 1]) == -S.DMAX and np.all(off[facts["clamp_pos"]] == np.float32(S.DMAX))
    assert np.all(np.abs(off) <= S.DMAX) and np.array_equal(np.floor(padded[:, 0]), y) and np.array_equal(np.floor(padded[:, 1]), x)
    assert np.abs(off.astype(np.float64) - off64).max() <= 2.0 ** -24  # one rounding of a quotient below 0.5
    assert np.abs(pos.astype(np.float64) - pos64).max() <= 2.0 ** -18  # + the roundings of y + 0.5 + d at |y| < 32
    # image 1: random neighbours, every selected pixel a strict maximum
    _, _, off1 = S.refine(s[1], idx[1], S.REFINE_PADS, np.float32)
    assert np.all(off1 != 0.0)


def test_blob_scene_on_the_restatement():
    """condition A (every refined keypoint within 0.05 px of its blob's centre) and condition B (the pixel centres are off by at
    least 0.3 px on average) on the float32 restatement, before any device sees the scene.  Measured: 0.030 max / 0.378 mean."""
    score, centres = S.blob_scene()
    H, W = S.BLOB_MAP
    errs, pix = [], []
    for b in range(S.BLOB_IMAGES):
        idx = S.blob_peaks(score[b])
        assert len(idx) == centres.shape[1] == 40
        pos, _, _ = S.refine(score[b], idx, dtype=np.float32)
        e, p = S.blob_errors(pos, idx, centres[b], W)
        errs.append(e)
        pix.append(p)
    errs, pix = np.concatenate(errs), np.concatenate(pix)
    print(f"blob scene: {errs.size} blobs, refined max {errs.max():.4f} px mean {errs.mean():.4f} px; pixel centres mean {pix.mean():.4f} px")
    assert errs.size == 560
    assert errs.max() <= S.BLOB_A
    assert pix.mean() >= S.BLOB_B


def test_restated_sampler_at_pixel_centres_is_the_pixel_centre_statement():
    Hp, Wp = S.SAMPLE_PADDED
    raw = S.sample_raw_map(8)
    idx = S.centre_indices(9)
    pos = er.positions_of(idx, Wp)
    a = S.sample(raw, [pos, pos[:0]], (Hp, Wp), 1.41)
    b = er.sample_low(raw, [pos, pos[:0]], (Hp, Wp), 1.41)
    assert torch.equal(a[0], b[0]) and a[1].shape == (0, 8)
    v, bound = S.sample_value_bound(raw[0], pos, (Hp, Wp))
    v0, a0 = er.sample_raw(raw[0], pos, (Hp, Wp))
    assert torch.equal(v, v0)
    # inside the image the extended bound is the pixel-centre one plus half a unit of coordinate shift per axis
    assert bool((bound >= er.sample_value_bound(raw[0], a0, *S.SAMPLE_MAP)).all())


def test_float_positions_cover_what_they_claim():
    Hp, Wp = S.SAMPLE_PADDED
    hc, wc = S.SAMPLE_MAP
    p, facts = S.float_positions()
    assert p[0].tolist() == [0.0, 0.0, 0.0] and p[1].tolist() == [float(Hp), float(Wp), 0.0]
    outside = (p[:, 0] < 0) | (p[:, 0] > Hp) | (p[:, 1] < 0) | (p[:, 1] > Wp)
    band = outside & (p[:, 0] >= -3) & (p[:, 0] <= Hp + 3) & (p[:, 1] >= -3) & (p[:, 1] <= Wp + 3)
    assert band.sum() >= 16
    raw = S.sample_raw_map(8)
    v, _ = er.sample_raw(np.abs(raw[0]) + 1.0, p, (Hp, Wp))
    far = np.zeros(len(p), bool)
    far[facts["far"]] = True
    assert bool((v[torch.from_numpy(far)] == 0).all())        # all four taps in the zero ring
    assert bool((v[torch.from_numpy(band)].abs().sum(1) > 0).all())  # the band still reaches the map: the reference samples it
    g = er._grid(p[4:4 + 2 * hc], (Hp, Wp)).double()[0, 0]
    iy = ((g[:, 1] + 1) * hc - 1) / 2
    assert float((iy - iy.round()).abs().max()) < 1e-5       # tap boundaries (up to the float32 grid's rounding)


def test_new_symbols_resolve_and_the_abi_version_stays():
    L = N.lib()
    assert hasattr(L, "einx_refine_keypoints") and hasattr(L, "einx_desc_sample_pos")
    assert L.einx_abi_version() == 6  # additive symbols only
    assert callable(N.refine_keypoints) and callable(N.desc_sample_pos)


def test_entries_refuse_bad_arguments_by_name():
    L = N.lib()
    p = 256  # never dereferenced: the checks come first
    args = lambda Hp, Wp: (p, 1, Hp, Wp, Hp, Wp, 0, 0, 0, p, p, 4, p, None, 0, 0, 0, 0, 0, 1.0, None, None)  # noqa: E731
    assert L.einx_refine_keypoints(*args(8193, 32)) != 0
    assert b"einx_refine_keypoints" in L.einx_last_error() and b"8192" in L.einx_last_error()
    assert L.einx_refine_keypoints(*args(32, 8193)) != 0
    assert L.einx_refine_keypoints(None, *args(24, 32)[1:]) != 0 and b"null pointer" in L.einx_last_error()
    bil = list(args(24, 32))
    bil[17] = 1  # bilinear without a raw map / descriptor rows
    assert L.einx_refine_keypoints(*bil) != 0 and b"null pointer" in L.einx_last_error()
    bil[13], bil[20], bil[14], bil[15], bil[16] = p, p, 513, 3, 4
    assert L.einx_refine_keypoints(*bil) != 0 and b"D must be <= 512" in L.einx_last_error()
    cl = list(args(24, 32))
    cl[18] = 1  # channels-last without bilinear
    assert L.einx_refine_keypoints(*cl) != 0 and b"channels-last" in L.einx_last_error()
    pos = lambda D, stride: (p, 1, D, 3, 4, 24, 32, 0, p, stride, 0, p, 4, 1.0, p, None)  # noqa: E731
    assert L.einx_desc_sample_pos(*pos(513, 3)) != 0 and b"einx_desc_sample_pos" in L.einx_last_error()
    assert L.einx_desc_sample_pos(*pos(8, 1)) != 0 and b"two coordinates" in L.einx_last_error()
    assert L.einx_desc_sample_pos(None, *pos(8, 3)[1:]) != 0 and b"null pointer" in L.einx_last_error()


@pytest.fixture(scope="module")
def extractors():
    out = {}
    for name in ("SP_MNN", "SiLK_MNN"):
        cfg = pkg.default_config(name, event_channels=5)
        model = pkg.EIM(cfg, device="cpu").eval()
        sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=3)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        out[name] = model
    return out


def test_switch_defaults_off_and_reads_pixel_on_the_cpu_and_in_training(extractors):
    assert BASE.NativeExtractor.subpixel is False
    for model in extractors.values():
        for wrapper in (model.event_extractor, model.image_extractor):
            ext = wrapper.extractor
            assert ext.subpixel is False and ext.keypoint_mode == "pixel"
            ext.subpixel = True
            try:
                assert ext.keypoint_mode == "pixel"  # parameters on the CPU
                assert ext.half_precision is False and ext.conv_mode == "fp32"  # independent switches
            finally:
                del ext.subpixel
            assert ext.subpixel is False
    # per side, and part of the graph key
    m = extractors["SP_MNN"]
    before = m._graph_config()
    m.event_extractor.extractor.subpixel = True
    try:
        assert m.image_extractor.extractor.subpixel is False
        assert len(m._graph_config()[0]) == len(before[0])  # on the CPU the mode still reads "pixel"
    finally:
        del m.event_extractor.extractor.subpixel


def test_training_mode_reads_pixel(monkeypatch):
    """with parameters that claim to be on a GPU the mode follows the switch in eval mode and reads "pixel" in training mode"""
    class FakeParam:
        device = torch.device("cuda", 0)

    ext = BASE.NativeExtractor.__new__(BASE.NativeExtractor)
    torch.nn.Module.__init__(ext)
    monkeypatch.setattr(BASE.NativeExtractor, "parameters", lambda self, recurse=True: iter([FakeParam()]))
    ext.eval()
    assert ext.keypoint_mode == "pixel"
    ext.subpixel = True
    assert ext.keypoint_mode == "subpixel"
    ext.train()
    assert ext.keypoint_mode == "pixel"


class _Det:
    cap = 4
    positions = indices = counts = None


@pytest.mark.parametrize("cell", [8, 1])
def test_engine_refines_only_when_asked(monkeypatch, cell):
    """a spy on _native.refine_keypoints: no call from a re-detection with the switch off, exactly one with it on -- after the
    descriptors are sampled for cell 8 (whose rows it rewrites), positions only for cell 1"""
    calls = []
    monkeypatch.setattr(N, "detect", lambda *a, **k: calls.append("detect") or _Det())
    monkeypatch.setattr(N, "desc_sample", lambda *a, **k: calls.append("desc_sample") or "rows")
    monkeypatch.setattr(N, "refine_keypoints", lambda *a, **k: calls.append(("refine", sorted(k))))
    eng = EX.ExtractorEngine("x", top_k=16, radius=4, border=4, det_thr=1.0, ordering="yx", cell=cell)
    bf = EX.BatchedFeats()
    bf.pads, bf.padded = (0, 0, 0, 0), (40, 48)
    assert bf.subpixel is False
    eng.redetect(bf)
    assert calls == ["detect", "desc_sample"]
    del calls[:]
    bf.subpixel = True
    eng.redetect(bf)
    if cell == 8:
        assert calls == ["detect", "desc_sample", ("refine", ["raw", "raw_cl", "scale", "sparse_desc"])]
    else:
        assert calls == ["detect", ("refine", []), "desc_sample"]


def test_extract_batched_hands_the_mode_to_the_engine(monkeypatch, extractors):
    seen = {}

    class Eng:
        def run(self, x, mask, **kw):
            seen.update(kw)
            return "bf"

    ext = extractors["SP_MNN"].image_extractor.extractor
    monkeypatch.setattr(type(ext), "engine", lambda self: Eng())
    monkeypatch.setattr(ext, "_scale_host", 1.0, raising=False)
    ext.subpixel = True
    try:
        assert ext.extract_batched(torch.zeros((1, 1, 40, 48))) == "bf"
    finally:
        del ext.subpixel
    assert seen["subpixel"] is False  # on the CPU the mode reads "pixel"


def test_sample_descriptors_at_refuses_non_finite_positions():
    raw = torch.zeros((1, 8, 5, 6))
    good = torch.tensor([[0.25, 0.75, 0.0], [41.0, -2.5, 0.0]])
    for bad in (float("nan"), float("inf"), float("-inf")):
        for col in (0, 1):
            p = good.clone()
            p[1, col] = bad
            with pytest.raises(ValueError, match="finite"):
                dd.sample_descriptors_at(raw, [p], S.SAMPLE_PADDED)
    with pytest.raises(ValueError, match="ordering"):
        dd.sample_descriptors_at(raw, [good], S.SAMPLE_PADDED, ordering="zz")
    with pytest.raises(ValueError, match="position lists"):
        dd.sample_descriptors_at(raw, [good, good], S.SAMPLE_PADDED)
    # finite positions pass the checks and reach the device call, which has no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.sample_descriptors_at(raw, [good], S.SAMPLE_PADDED)
    # the pixel-centre sampler keeps refusing, and points at the new function
    with pytest.raises(NotImplementedError, match="sample_descriptors_at"):
        dd.sparsify_low_resolution_descriptors(raw, [good], S.SAMPLE_PADDED)
