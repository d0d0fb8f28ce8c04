"""GPU tests (-m gpu), component: the perspective warp (datasets/warp.py, csrc/warp.hip) against the yardstick of
tests/warp_ref.py: source points in numpy float64 in the documented order, values by F.grid_sample in float64 on the CPU.

Gates, and where each comes from:
  valid            exact, on every pixel: test_warp_cpu.py checks that no pixel of these cases lies within 1e-9 of the validity
                   boundary (the exact homographies put pixels ON it, where float64 decides without rounding).
  float32 values   |gpu - f64| <= 8 * 2^-24 * max|tap|, derived in warp_ref.py from the kernel's roundings; the observed error is
                   printed beside it.  Invalid pixels are 0.
  exact H          the identity, an integer translation and the half turn are permutations: bit-equal to integer indexing.
  uint8            bit-equal to the half-even rounding of the float32 path on the same input.
  nearest          bit-equal to grid_sample's nearest on the CPU (no source point of these cases lies within 1e-9 of a tie)."""
from importlib import import_module

import numpy as np
import pytest
import torch

import warp_ref as ref
from gpu_support import DEV, pkg

pytestmark = pytest.mark.gpu

warp = import_module(pkg.__name__ + ".datasets.warp")
hom = import_module(pkg.__name__ + ".core.geometry.homography")
INEXACT = ref.inexact_cases(hom.sample_homographies)


def _hinv(H):
    return warp.invert_homography(torch.from_numpy(np.asarray(H, np.float64)).reshape(-1, 3, 3)).numpy()


def _check_f32(tag, src, H, dst, got, valid):
    exp, exp_valid = ref.yardstick(src, _hinv(H), dst)
    got, valid = got.cpu(), valid.cpu()
    assert valid.dtype == torch.bool and tuple(valid.shape) == (src.shape[0], 1, *dst)
    assert torch.equal(valid[:, 0], exp_valid), f"{tag}: {int((valid[:, 0] != exp_valid).sum())} validity flags differ"
    v = exp_valid[:, None].expand_as(got)
    assert bool((got[~v] == 0).all()), f"{tag}: an invalid pixel is not 0"
    assert torch.equal(torch.isnan(got[v]), torch.isnan(exp[v])), f"{tag}: NaN pattern differs"
    fin = v & ~torch.isnan(exp)
    err, b = float((got.double() - exp)[fin].abs().max()) if bool(fin.any()) else 0.0, ref.bound(src)
    print(f"{tag}: max |gpu - f64| {err:.3e}, bound {b:.3e}, {int(exp_valid.sum())} of {exp_valid.numel()} pixels valid")
    assert err <= b, tag


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("name", list(INEXACT))
def test_float32_against_the_float64_yardstick(name, C):
    H, (Hs, Ws), dst = INEXACT[name]
    src = ref.image(7, ref.B, C, Hs, Ws)
    got, valid = warp.warp_perspective(src.to(DEV), H, out_shape=dst)
    assert got.dtype == torch.float32 and tuple(got.shape) == (ref.B, C, *dst)
    _check_f32(f"{name} C={C}", src, H, dst, got, valid)
    again, valid2 = warp.warp_perspective(src.to(DEV), H, out_shape=dst)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(valid, valid2)  # two runs: equal bits


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("sizes", ref.SIZES)
def test_exact_homographies_are_permutations(sizes, C):
    (Hs, Ws), dst = sizes
    src = ref.image(8, ref.B, C, Hs, Ws)
    for tag, H in (("identity", np.eye(3)), ("translation", ref.translation(3, -2)), ("half turn", ref.rot180(Hs, Ws))):
        exp, exp_valid = ref.gather_exact(src, _hinv(H), dst)
        for dtype in (torch.float32, torch.uint8):
            s = src.to(dtype)
            got, valid = warp.warp_perspective(s.to(DEV), torch.from_numpy(H).float() if dtype == torch.uint8 else H, out_shape=dst)
            assert got.dtype == dtype
            assert torch.equal(valid.cpu()[:, 0], exp_valid), (tag, dtype)
            assert torch.equal(got.cpu(), exp.to(dtype)), (tag, dtype)  # (the cast commutes with a permutation)
        if tag == "identity" and dst == (Hs, Ws):
            assert bool(exp_valid.all()) and torch.equal(exp, src)
        if tag == "translation" and dst == (Hs, Ws):
            assert int(exp_valid[0].sum()) == (Hs - 2) * (Ws - 3)


@pytest.mark.parametrize("name", [n for n in INEXACT if not n.startswith("wsign")])
def test_uint8_is_the_half_even_rounding_of_the_float32_path(name):
    H, (Hs, Ws), dst = INEXACT[name]
    src = ref.image(9, ref.B, 2, Hs, Ws).to(torch.uint8).to(DEV)
    got, valid = warp.warp_perspective(src, H, out_shape=dst)
    f32, valid_f = warp.warp_perspective(src.float(), H, out_shape=dst)
    assert got.dtype == torch.uint8 and torch.equal(valid, valid_f)
    assert torch.equal(got, torch.round(f32).to(torch.uint8))  # torch.round: half to even
    assert int(((f32 - torch.floor(f32)) != 0).sum()) > f32.numel() // 4  # the rounding had something to do


@pytest.mark.parametrize("name", [n for n in INEXACT if n.startswith("sampled")])
def test_nearest_mode_on_a_bool_mask(name):
    H, (Hs, Ws), dst = INEXACT[name]
    mask = ref.image(10, ref.B, 1, Hs, Ws) > 128
    got, valid = warp.warp_perspective(mask.to(DEV), H, out_shape=dst, mode="bilinear")  # a bool input is warped nearest whatever is asked
    assert got.dtype == torch.bool and tuple(got.shape) == (ref.B, 1, *dst)
    exp, exp_valid = ref.yardstick(mask, _hinv(H), dst, mode="nearest")
    assert torch.equal(valid.cpu()[:, 0], exp_valid)
    assert torch.equal(got.cpu(), (exp != 0) & exp_valid[:, None])
    assert 0.2 < float(got.float().mean()) < 0.8
    # a [B,H,W] uint8 label image in nearest mode: the same pixels, values copied
    lab = (ref.image(11, ref.B, 1, Hs, Ws)[:, 0]).to(torch.uint8)
    got3, _ = warp.warp_perspective(lab.to(DEV), H, out_shape=dst, mode="nearest")
    exp3, _ = ref.yardstick(lab[:, None], _hinv(H), dst, mode="nearest")
    assert tuple(got3.shape) == (ref.B, *dst) and torch.equal(got3.cpu(), (exp3[:, 0] * exp_valid).to(torch.uint8))


def test_non_contiguous_source_and_the_callers_tensor():
    H, (Hs, Ws), dst = INEXACT["mixed 13x19->11x23"]
    base = ref.image(12, ref.B, 5, 2 * Hs, Ws + 3).to(DEV)
    keep = base.clone()
    view = base[:, :, ::2, 2:-1]
    assert not view.is_contiguous() and tuple(view.shape[-2:]) == (Hs, Ws)
    got, valid = warp.warp_perspective(view, H, out_shape=dst)
    exp, exp_valid = warp.warp_perspective(view.contiguous(), H, out_shape=dst)
    assert torch.equal(got, exp) and torch.equal(valid, exp_valid) and torch.equal(base, keep)
    # one [3,3] matrix for all, in float32 on the device: the same as its float64 copies on the host
    one = torch.from_numpy(H[2]).float()
    a, va = warp.warp_perspective(view, one.to(DEV), out_shape=dst)
    b, vb = warp.warp_perspective(view, one.double()[None].repeat(ref.B, 1, 1), out_shape=dst)
    assert torch.equal(a, b) and torch.equal(va, vb)


def test_nan_taps_propagate():
    H, (Hs, Ws), dst = INEXACT["sampled 13x19->13x19"]
    src = ref.image(13, ref.B, 1, Hs, Ws)
    src[0, 0, 6, 9] = float("nan")
    src[2, 0, 0, 0] = float("nan")
    got, valid = warp.warp_perspective(src.to(DEV), H, out_shape=dst)
    assert 0 < int(torch.isnan(got).sum()) < got.numel() // 2
    _check_f32("NaN taps", src, H, dst, got, valid)


def test_the_call_can_be_captured_and_replayed():
    """no workspace, no allocation of its own, no synchronisation: a captured call replays on new contents of the same buffers"""
    H, (Hs, Ws), dst = INEXACT["mixed 65x346->65x346"]
    nat = pkg.native
    Hinv = warp.invert_homography(torch.from_numpy(H)).reshape(ref.B, 9).to(DEV).contiguous()
    src = ref.image(14, ref.B, 2, Hs, Ws).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nat.warp_perspective(src, Hinv, *dst)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, valid = nat.warp_perspective(src, Hinv, *dst)
    src.copy_(ref.image(15, ref.B, 2, Hs, Ws))
    Hinv.copy_(Hinv.roll(1, 0))
    g.replay()
    torch.cuda.synchronize()
    exp, exp_valid = nat.warp_perspective(src, Hinv, *dst)
    assert torch.equal(out, exp) and torch.equal(valid, exp_valid) and 0 < int(valid.sum()) < valid.numel()


def test_empty_shapes():
    H = torch.eye(3)
    for shape, dst in (((0, 2, 5, 7), None), ((2, 0, 5, 7), None), ((2, 1, 5, 7), (0, 4)), ((2, 1, 5, 7), (4, 0))):
        x = torch.zeros(shape, device=DEV)
        got, valid = warp.warp_perspective(x, H, out_shape=dst)
        hd, wd = shape[-2:] if dst is None else dst
        assert tuple(got.shape) == (shape[0], shape[1], hd, wd) and tuple(valid.shape) == (shape[0], 1, hd, wd)
        if shape[1] == 0:
            assert bool(valid.all())  # no channel to write, the flags are still the identity's
    got, valid = warp.warp_perspective(torch.zeros((2, 1, 0, 7), device=DEV), H, out_shape=(3, 4))  # no source pixel: nothing is valid
    assert tuple(got.shape) == (2, 1, 3, 4) and not bool(valid.any()) and not bool(got.any())


def test_the_pixel_centre_convention():
    """a single set pixel under an affine H that takes pixel centres to pixel centres: the set pixel of the output is the one whose
    centre is H (c + 0.5, r + 0.5).  With the centres at integers instead, the quarter turn lands one column off."""
    Hs, Ws, r, c = 13, 19, 4, 11
    src = torch.zeros(1, 1, Hs, Ws)
    src[0, 0, r, c] = 7.0
    for H, dst in ((ref.rot90(Hs), (Ws, Hs)), (np.array([[1.0, 0, 2], [0, 1.0, 5], [0, 0, 1.0]]), (Hs + 6, Ws + 3))):
        x, y, w = H @ np.array([c + 0.5, r + 0.5, 1.0])
        col, row = int(np.floor(x / w)), int(np.floor(y / w))
        assert (x / w - col, y / w - row) == (0.5, 0.5)
        got, valid = warp.warp_perspective(src.to(DEV), H, out_shape=dst)
        hit = torch.nonzero(got.cpu()[0, 0])
        assert hit.tolist() == [[row, col]] and float(got[0, 0, row, col]) == 7.0, (hit.tolist(), (row, col))
        assert int(valid.sum()) == Hs * Ws  # the whole source is in the destination
