"""Homographic pairs (core/geometry/homography.py, datasets/warp.py, csrc/warp.hip), the part that needs no GPU: the
sampler against what the reference's own sampler returned for the same seeds (tests/golden/warp.npz, gen_warp.py), the state it
leaves the generator in, the drop-in point warps, every refusal of the Python layer and of the C ABI (all raised before a device
call), and the preconditions of the GPU module's cases (tests/warp_ref.py)."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import warp_ref as ref
from helpers import Golden, load_pkg

pkg = load_pkg()
L = pkg.native.lib()
hom = import_module(pkg.__name__ + ".core.geometry.homography")
warp = import_module(pkg.__name__ + ".datasets.warp")
harness = import_module(pkg.__name__ + ".harness")
WARP = Golden("warp")
EINX_ERR_ARG = -1


def _normalised(H):
    return H / H[2, 2]


@pytest.mark.parametrize("name", list(WARP.cases))
def test_sampler_reproduces_the_reference(name):
    """the same H (relative 1e-10: np.linalg.solve may differ between BLAS builds, the draws may not), the same corners, and the
    generator left in the same state: its next draw is the one recorded after the reference's call"""
    c = WARP.cases[name]
    rng = np.random.RandomState(c["seed"])
    H, full, warped, patch = hom.sample_homography_corners(tuple(c["shape"]), tuple(c["patch_shape"]), rng=rng, **c["kw"])
    assert rng.uniform() == WARP[f"{name}.next"][0]
    assert H.shape == (3, 3) and H.dtype == np.float64 and tuple(patch) == tuple(c["patch_shape"])
    exp = _normalised(WARP[f"{name}.H"])
    err = np.abs(_normalised(H) - exp).max() / np.abs(exp).max()
    print(f"{name}: tries {c['tries']}, H differs by {err:.3e} (relative)")
    assert err <= 1e-10
    assert np.array_equal(full, WARP[f"{name}.full"])
    assert np.allclose(warped, WARP[f"{name}.warped"], rtol=0, atol=1e-9 * max(c["shape"]))


def test_fixture_covers_what_it_should():
    cases = list(WARP.cases.values())
    assert len(cases) >= 12 and max(c["tries"] for c in cases) >= 2
    assert {tuple(c["shape"]) for c in cases} == {(346, 260), (240, 180)}
    assert any(c["shape"] != c["patch_shape"] for c in cases) and any(c["kw"].get("n_angles") == 0 for c in cases)
    assert {c["kw"]["difficulty"] for c in cases} >= {0.0, 0.3, 0.7, 1.0}


def test_sample_homographies_is_successive_calls_on_one_rng():
    a = hom.sample_homographies(3, (346, 260), rng=np.random.RandomState(5), difficulty=0.6)
    rng = np.random.RandomState(5)
    b = np.stack([hom.sample_homography_corners((346, 260), (346, 260), difficulty=0.6, rng=rng)[0] for _ in range(3)])
    assert a.shape == (3, 3, 3) and a.dtype == np.float64 and np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1])
    assert hom.sample_homographies(0, (346, 260), rng=rng).shape == (0, 3, 3)
    with pytest.raises(ValueError, match="negative"):
        hom.sample_homographies(-1, (346, 260), rng=rng)
    with pytest.raises(TypeError):
        hom.sample_homographies(1, (346, 260))  # rng is required: a run is reproducible from its seed


def test_point_warps_are_drop_in():
    p = WARP.meta["points"]
    pts = np.random.RandomState(p["seed"]).uniform(0, p["hi"], size=(p["n"], 2))
    Hs = np.stack([WARP[f"{n}.H"] for n in p["H"]])
    tp = torch.from_numpy(np.stack([pts, pts[::-1].copy(), pts * 0.5]))
    for inverse, tag in ((True, "inv"), (False, "fwd")):
        one, many = hom.warp_points(pts, Hs[0], inverse=inverse), hom.warp_points(pts, Hs, inverse=inverse)
        assert one.shape == (p["n"], 2) and many.shape == (3, p["n"], 2)
        assert np.allclose(one, WARP[f"points.single.{tag}"], rtol=1e-10, atol=0)
        assert np.allclose(many, WARP[f"points.batched.{tag}"], rtol=1e-10, atol=0)
        t3 = hom.warp_points_torch(tp, torch.from_numpy(Hs), inverse=inverse)
        t1 = hom.warp_points_torch(tp, torch.from_numpy(Hs[1]), inverse=inverse)
        assert t3.dtype == torch.float64 and tuple(t3.shape) == (3, p["n"], 2)
        assert np.allclose(t3.numpy(), WARP[f"points.torch.{tag}"], rtol=1e-10, atol=0)
        assert np.allclose(t1.numpy(), WARP[f"points.torch1.{tag}"], rtol=1e-10, atol=0)
    assert np.array_equal(hom.flat2mat(np.arange(8.0)[None]), WARP["points.flat2mat"])
    got = hom.compute_homography(np.array([[0.0, 0], [0, 2], [3, 2], [3, 0]]), np.array([[1.0, 1], [0, 3], [4, 4], [5, 0]]), [1.0, 1.0])
    assert np.allclose(got, WARP["points.compute"], rtol=1e-10, atol=1e-12)
    # the sampler's H takes the image's corners where it says
    c = WARP.cases["mvsec_patch"]
    H, full, warped, _ = hom.sample_homography_corners(tuple(c["shape"]), tuple(c["patch_shape"]), rng=np.random.RandomState(c["seed"]), **c["kw"])
    assert np.allclose(hom.warp_points(warped, H, inverse=True), full, atol=1e-8)


def test_invert_homography_is_the_adjugate_and_exact_where_it_can_be():
    eye = warp.invert_homography(torch.eye(3)[None])
    assert eye.dtype == torch.float64 and torch.equal(eye[0], torch.eye(3, dtype=torch.float64))
    t = warp.invert_homography(torch.from_numpy(ref.translation(3, -2))[None])[0].numpy()
    assert np.array_equal(t, ref.translation(-3, 2))
    r = ref.rot180(13, 19)
    assert np.array_equal(warp.invert_homography(torch.from_numpy(r)[None])[0].numpy(), r)  # its own inverse
    H = torch.from_numpy(hom.sample_homographies(4, (346, 260), rng=np.random.RandomState(3), difficulty=0.8))
    inv = warp.invert_homography(H)
    assert (inv @ H - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-9
    assert torch.equal(warp.invert_homography(H.float()), warp.invert_homography(H.float().double()))  # formed in float64, whatever comes in
    assert not torch.isfinite(warp.invert_homography(torch.zeros(1, 3, 3))).any()  # singular: nothing raises, nothing is read back


def test_symbol_and_abi_version():
    sig = import_module(pkg.__name__ + "._lib").SIGNATURES
    assert "einx_warp_perspective" in sig and hasattr(L, "einx_warp_perspective")
    assert L.einx_abi_version() == 6  # an additive symbol
    assert pkg.HomographicEvaluator is harness.HomographicEvaluator
    assert import_module(pkg.__name__ + ".datasets").warp_perspective is warp.warp_perspective


def test_c_abi_refusals_and_empty_shapes():
    """EINX_ERR_ARG with a message in the house style, from host code that runs before any launch; empty shapes succeed without one"""
    one = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    call = L.einx_warp_perspective
    ok_args = dict(src=one, src_type=1, B=2, C=1, Hs=4, Ws=5, Hinv=one, Hd=4, Wd=5, mode=0, dst=one, valid=one, stream=None)

    def status(**kw):
        a = dict(ok_args, **kw)
        return call(*[a[k] for k in ok_args])

    for kw, word in ((dict(src_type=2), b"src_type"), (dict(src_type=-1), b"src_type"), (dict(mode=2), b"mode"), (dict(B=-1), b"negative"),
                     (dict(C=-1), b"negative"), (dict(Hs=-1), b"negative"), (dict(Ws=-2), b"negative"), (dict(Hd=-1), b"negative"),
                     (dict(Wd=-1), b"negative"), (dict(src=None), b"null"), (dict(Hinv=None), b"null"), (dict(dst=None), b"null")):
        assert status(**kw) == EINX_ERR_ARG, kw
        msg = L.einx_last_error()
        assert msg.startswith(b"einx_warp_perspective: ") and word in msg, (kw, msg)
    for kw in (dict(B=0), dict(Hd=0), dict(Wd=0), dict(C=0, valid=None), dict(B=0, src=None, Hinv=None, dst=None, valid=None)):
        assert status(**kw) == 0, kw


def test_python_refusals():
    x = torch.zeros(2, 1, 5, 7)
    eye = torch.eye(3)
    with pytest.raises(ValueError, match="must be a tensor"):
        warp.warp_perspective(np.zeros((2, 1, 5, 7), np.float32), eye)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        warp.warp_perspective(torch.zeros(5, 7), eye)
    with pytest.raises(ValueError, match="uint8, float32 or bool"):
        warp.warp_perspective(x.double(), eye)
    with pytest.raises(ValueError, match="mode must be"):
        warp.warp_perspective(x, eye, mode="bicubic")
    with pytest.raises(ValueError, match="out_shape must be"):
        warp.warp_perspective(x, eye, out_shape=5)
    with pytest.raises(ValueError, match="out_shape must not be negative"):
        warp.warp_perspective(x, eye, out_shape=(5, -1))
    with pytest.raises(ValueError, match=r"H must be \[2, 3, 3\]"):
        warp.warp_perspective(x, torch.eye(3)[None].repeat(3, 1, 1))
    with pytest.raises(ValueError, match=r"H must be \[2, 3, 3\]"):
        warp.warp_perspective(x, torch.eye(4))
    with pytest.raises(ValueError, match="float tensor"):
        warp.warp_perspective(x, torch.eye(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP device"):  # every argument is fine: there is no CPU path
        warp.warp_perspective(x, eye)


def test_evaluator_refusals_and_unchanged_parents():
    import types
    lg = pkg.LightGlue({"width_confidence": 0.9}).eval()
    with_lg = types.SimpleNamespace(matcher=types.SimpleNamespace(matcher=lg))
    with_mnn = types.SimpleNamespace(matcher=types.SimpleNamespace(matcher=pkg.NearestNeighborMatcher()))
    ident = lambda B, shape: np.tile(np.eye(3), (B, 1, 1))  # noqa: E731
    with pytest.raises(TypeError):
        pkg.HomographicEvaluator(with_lg, 5)  # no sampler
    with pytest.raises(ValueError, match="sampler must be a callable"):
        pkg.HomographicEvaluator(with_lg, 5, sampler=np.eye(3))
    with pytest.raises(ValueError, match="takes no losses"):
        pkg.HomographicEvaluator(with_lg, 5, sampler=ident, losses={})
    with pytest.raises(ValueError, match="needs a LightGlue matcher"):
        pkg.HomographicEvaluator(with_mnn, 5, sampler=ident, matcher_loss=True)
    ev = pkg.HomographicEvaluator(with_lg, 5, sampler=ident, matcher_loss=True)
    assert (ev.gt_pos_th, ev.gt_neg_th) == (3, 6)  # gt_matches_from_homography's defaults
    ev._validate(harness._Batch([], None))
    lg.point_pruning = True
    with pytest.raises(ValueError, match="point pruning"):
        ev._validate(harness._Batch([], None))
    with pytest.raises(ValueError, match="takes no depth maps"):
        pkg.HomographicEvaluator(with_mnn, 5, sampler=ident)._validate(harness._Batch([], None, depth=(0, 0)))
    for extra in (dict(homography=torch.eye(3)), dict(pose=(0, 0, 0)), dict(image_mask=torch.ones(1))):
        with pytest.raises(ValueError, match="samples the pair's homography itself"):
            ev._warped(harness._Batch([], torch.zeros(1, 1, 4, 4), **extra))
    bad = pkg.HomographicEvaluator(with_mnn, 5, sampler=lambda B, shape: np.eye(3))
    with pytest.raises(ValueError, match="sampler must return"):
        bad._warped(harness._Batch([], torch.zeros(2, 1, 4, 4)))
    # the field the parents never set comes last and defaults to None: their batches are what they were
    assert harness._Batch._fields == ("events_list", "images", "homography", "pose", "depth", "image_mask")
    assert harness._Batch([], None, None, None, None).image_mask is None


def test_preconditions_of_the_gpu_cases():
    """no pixel of an inexact case lies within 1e-9 of the validity boundary (the GPU module compares `valid` exactly and
    everywhere); every sample has valid pixels, and those of the sign-changing and mixed cases invalid ones too; no nearest-mode
    tie in the sampled cases; the exact homographies take pixel centres to pixel centres"""
    for name, (H, (Hs, Ws), dst) in ref.inexact_cases(hom.sample_homographies).items():
        Hinv = warp.invert_homography(torch.from_numpy(H)).numpy()
        qx, qy, w = ref.source_points(Hinv, *dst)
        near = int(ref.near_boundary(qx, qy, w, Hs, Ws).sum())
        valid = ref.valid_rule(qx, qy, w, Hs, Ws)
        share = valid.reshape(ref.B, -1).mean(1)
        q = np.stack([qx, qy])[:, valid]
        frac = q - np.floor(q)  # nearest mode rounds q - 0.5: a tie is a q at an integer
        gap = float(np.minimum(frac, 1 - frac).min())
        print(f"{name}: {near} pixels near the boundary, valid share {np.round(share, 3).tolist()}, nearest tie gap {gap:.2e}")
        assert near == 0, name
        assert (share > 0.02).all(), name
        if name.startswith("wsign"):
            assert (w > 0).any() and (w < 0).any() and (share < 1).all()
        if name.startswith("mixed"):
            assert (share[:2] < 1).all(), name
        if name.startswith("sampled"):
            assert gap > 1e-9, name
    for (Hs, Ws), dst in ref.SIZES:
        for H in (np.eye(3), ref.translation(3, -2), ref.rot180(Hs, Ws)):
            Hinv = warp.invert_homography(torch.from_numpy(H)[None]).numpy()
            ref.gather_exact(torch.zeros(1, 1, Hs, Ws), Hinv, dst)  # asserts the exactness
