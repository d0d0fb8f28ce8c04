"""CPU tests of core.geometry.depth / .epipolar / .utils and core.metrics.util: the float64 restatement
tests/geometry_f64.py against itself in float32 -- the condition under which tests/test_geometry_gpu.py may compare with
array_equal -- and against the reference's fixture tests/golden/geometry.npz; the module surface; the refusals; the host-side
parts of the new entry points."""
import ctypes
import inspect
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import geometry_f64 as F
from helpers import GOLDEN, load_pkg

pkg = load_pkg()
_lib = import_module(pkg.__name__ + "._lib")
NM = import_module(pkg.__name__ + ".core.metrics._native_metrics")
depth = import_module(pkg.__name__ + ".core.geometry.depth")
epipolar = import_module(pkg.__name__ + ".core.geometry.epipolar")
utils = import_module(pkg.__name__ + ".core.geometry.utils")
mutil = import_module(pkg.__name__ + ".core.metrics.util")
wrappers = import_module(pkg.__name__ + ".core.geometry.wrappers")
pairs = import_module(pkg.__name__ + ".datasets.pairs")
GOLD = np.load(os.path.join(GOLDEN, "geometry.npz"))
META = json.loads(bytes(GOLD["meta"]).decode())
BOUNDS = {"none": None, "eq": F.BOUND_EQ, "above": F.BOUND_ABOVE}


def _same(a, b, what):
    assert np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True), what


# ------------------------------------------------------------------------------------------------ the restatement is exact in fp32
@pytest.mark.parametrize("n", F.PROJECT_N)
def test_fp32_evaluation_is_exact_sparse(n):
    """every projection, depth and flag of the occlusion scenes is the same in float32 and float64, for every form the GPU test
    runs: no cycle check, the bound on a distance and one lattice step above it, T_1to0 given and inverted, maps and given depths"""
    for ccth in BOUNDS.values():
        for given in (True, False):
            for pre in (False, True):
                e64, e32 = F.occlusion_expected(n, ccth, given, pre, np.float64), F.occlusion_expected(n, ccth, given, pre, np.float32)
                for b, (a, q) in enumerate(zip(e64, e32)):
                    assert q["proj_0to1"].dtype == np.float32 and a["proj_0to1"].dtype == np.float64
                    for k in F.G.STAGE_A_KEYS:
                        _same(a[k], q[k], (n, ccth, given, pre, b, k))


def test_sparse_cases_hold_what_the_gpu_test_needs():
    """per side, over the pairs of the scenes: a consistent point; one hidden behind a nearer surface (invisible at the bound, its
    squared cycle distance EQUAL to it; visible without the check and with the bound one lattice step above); a hole, a NaN and a
    negative value under a projection; a projection outside the other camera and a point behind it; a way back that ends outside"""
    for n in F.PROJECT_N[1:]:
        c = F.occlusion_scene(n)
        none, eq, above = (F.occlusion_expected(n, t, True, False) for t in BOUNDS.values())
        pre = F.occlusion_expected(n, F.BOUND_EQ, True, True)
        for side in (0, 1):
            vis, info = f"visible{side}", f"side{side}"
            got = {k: 0 for k in ("consistent", "hidden_eq", "below", "hole", "outside", "behind", "back_out")}
            for b in range(c.B):
                fwd, i = none[b][vis], eq[b][info]
                got["consistent"] += int((fwd & eq[b][vis] & (i["dist"] == 0)).sum())
                at = fwd & i["validj"] & i["back_ok"] & (i["dist"] == F.BOUND_EQ)
                assert not eq[b][vis][at].any() and above[b][vis][at].all(), (n, side, b, "strict comparison")
                got["hidden_eq"] += int(at.sum())
                got["below"] += int((at & above[b][vis]).sum())
                got["hole"] += int((fwd & ~i["validj"]).sum())
                got["outside"] += int((none[b][f"valid{side}"] & i["front"] & ~i["inside"]).sum())
                got["behind"] += int((pre[b][f"valid{side}"] & ~pre[b][info]["front"]).sum())
                got["back_out"] += int((fwd & i["validj"] & above[b][info]["consistent"] & ~i["back_ok"]).sum())
            assert all(v > 0 for v in got.values()), (n, side, got)
        # the three kinds of hole under a projection, in pair 0
        d = [c.depth0[0], c.depth1[0]]
        for side in (0, 1):
            i = eq[0][f"side{side}"]
            uv = none[0]["proj_0to1" if side == 0 else "proj_1to0"][none[0][f"visible{side}"] & ~i["validj"]]
            under = d[1 - side][np.floor(uv[:, 1]).astype(int), np.floor(uv[:, 0]).astype(int)]
            assert (under == 0).any() and np.isnan(under).any() and (under < 0).any(), (n, side)


@pytest.mark.parametrize("name", list(F.DENSE_SHAPES))
def test_fp32_evaluation_is_exact_dense(name):
    c = F.dense_case(name)
    changed = 0
    for b in range(c.B):
        runs = {}
        for tag, ccth in BOUNDS.items():
            a = F.dense_warp(c.depth_i[b], c.depth_j[b], c.K_i[b], c.K_j[b], c.T[b], ccth, np.float64)
            q = F.dense_warp(c.depth_i[b], c.depth_j[b], c.K_i[b], c.K_j[b], c.T[b], ccth, np.float32)
            valid = c.depth_i[b] > 0
            _same(a[0][valid], q[0][valid], (name, b, tag))  # a hole's projection divides by the clamped z: not exact, not compared
            assert np.array_equal(a[1], q[1]) and a[2] == q[2] and a[2] == (int(valid.sum()), int(a[1].sum()))
            runs[tag] = a
            # the reference's float32 run
            _same(GOLD[f"dense.{name}.{b}.{tag}.warp"][valid], a[0][valid], (name, b, tag, "fixture"))
            assert np.array_equal(np.unpackbits(GOLD[f"dense.{name}.{b}.{tag}.visible"])[:a[1].size].astype(bool), a[1]), (name, b, tag)
        changed += int((runs["none"][1] != runs["eq"][1]).sum()) + int((runs["eq"][1] != runs["above"][1]).sum())
    assert changed > 0 or name == "5x7", "the cycle check and the strict bound decide something in this case"


def _fixture_close(g, a, what):
    """the reference's own float32 run of the sampler is not exact on a 9 x 11 map: its x / W * 2 - 1 round trip through
    grid_sample's normalised coordinates takes four roundings of 2^-24 at magnitude <= max(H, W), a coordinate error of
    4 * 2^-24 * 11 pixels, times the steepest slope of the maps (values in [-2, 2]: at most 4 per pixel and axis, 8 for both),
    plus the interpolation's own four roundings at magnitude 2.  Same NaNs, and values within that."""
    g, a = np.asarray(g, np.float64), np.asarray(a, np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(a)), what
    bound = 8 * (4 * 2.0 ** -24 * 11) + 4 * 2.0 ** -24 * 2
    assert np.nanmax(np.abs(g - a), initial=0.0) <= bound, (what, np.nanmax(np.abs(g - a)), bound)


def test_samplers_against_the_fixture():
    fm, pts = F.sample_case(3)
    for b in range(2):
        a, q = F.sample_fmap(pts[b], fm[b]), F.sample_fmap(pts[b], fm[b], np.float32)
        _same(a, q, b)
        _fixture_close(GOLD["sample_fmap"][b], a, ("fixture", b))
        assert np.isnan(a).any() and (a == 0).any()
    fm, pts = F.sample_case(1)
    for b in range(2):
        d, valid = F.sample_depth(pts[b], fm[b, 0])
        d32, valid32 = F.sample_depth(pts[b], fm[b, 0], np.float32)
        _same(d, d32, b)
        assert np.array_equal(valid, valid32)
        _fixture_close(GOLD["sample_depth.d"][b], d, ("fixture", b))
        assert np.array_equal(GOLD["sample_depth.valid"][b], valid)
    # the planted taps: an on-grid point beside NaNs is its own pixel; a weighted NaN sends the sample to the nearest pixel
    a = F.sample_fmap(pts[0][:4], F.sample_case(3)[0][0])
    assert (a[0] == 0.75).all() and (a[1] == 0.5).all() and np.isnan(a[2]).all() and np.isnan(a[3]).all()


def test_project_against_the_fixture():
    c = F.occlusion_scene(257)
    for tag, ccth in BOUNDS.items():
        exp = F.occlusion_expected(257, ccth, True, False)
        for b in range(c.B):
            for side, (pk, vk) in enumerate((("proj_0to1", "visible0"), ("proj_1to0", "visible1"))):
                _same(GOLD[f"project.{b}.{side}.{tag}.proj"], exp[b][pk], (tag, b, side))
                assert np.array_equal(GOLD[f"project.{b}.{side}.{tag}.visible"], exp[b][vk]), (tag, b, side)


def _relative(got, exp):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nanmax(np.where(exp == 0, np.abs(got), np.abs(got - exp) / np.abs(exp)))


def test_epipolar_against_the_fixture():
    for n, m in F.EPI_SHAPES:
        p0, p1, E = F.epipolar_case(n, m)
        g = GOLD[f"epi_all.{n}x{m}"]
        for b in range(g.shape[0]):
            exp = F.epipolar_all(p0[b], p1[b], E[b])
            assert np.isfinite(exp).all() and _relative(g[b].astype(np.float64), exp) <= F.EPI_GATE, (n, m, b)
    p0, p1, E = F.epipolar_case(260, 260, cols=(2, 3))
    for sq in (True, False):
        for b in range(2):
            exp = F.epipolar_pairs(p0[b], p1[b], E[b], sq)
            assert _relative(GOLD[f"epi_pairs.{int(sq)}"][b].astype(np.float64), exp) <= F.EPI_GATE, (sq, b)
            got = epipolar.sym_epipolar_distance(torch.from_numpy(p0[b]), torch.from_numpy(p1[b]), torch.from_numpy(E[b]), squared=sq).numpy()
            assert _relative(got.astype(np.float64), exp) <= F.EPI_GATE, (sq, b, "the package's own, on the CPU")
    p0, p1, Fm = F.general_epipolar_case()
    g = META["epi_general"]
    exp = F.epipolar_all(p0[0], p1[0], Fm[0])
    assert np.abs(GOLD["epi_general"][0] - exp).max() <= g["bound"] and g["bound"] == 2 * g["floor"] + 4 * float(np.spacing(np.float32(g["max"])))


def test_pose_errors_against_the_fixture():
    T, estimates = F.pose_error_case()
    for k, (R, t) in enumerate(estimates):
        t_err, r_err = epipolar.relative_pose_error(torch.from_numpy(T), torch.from_numpy(R), torch.from_numpy(t))
        # the same float32 operators in the same order; three roundings (quotient, arccos, degrees) of 2^-24 on values below 180
        assert np.allclose([float(t_err), float(r_err)], GOLD["pose_error"][k], rtol=0, atol=180 * 3 * 2.0 ** -24), k
    assert float(epipolar.relative_pose_error(torch.from_numpy(T), torch.from_numpy(estimates[0][0]), torch.from_numpy(estimates[0][1]),
                                              ignore_gt_t_thr=2.0)[0]) == 0
    R1, R2, t = epipolar.decompose_essential_matrix(epipolar.T_to_E(wrappers.Pose.from_4x4mat(torch.from_numpy(T)[None])))
    Rt = torch.from_numpy(T[:3, :3])
    assert min(float((R1[0] - Rt).abs().max()), float((R2[0] - Rt).abs().max())) < 1e-5
    assert abs(abs(float((t[0] * torch.from_numpy(T[:3, 3])).sum())) - 1) < 1e-5 and float(torch.det(R1[0])) > 0.99


# ------------------------------------------------------------------------------------------------ the module surface
def test_module_surface():
    mods = {"depth": depth, "epipolar": epipolar, "utils": utils, "metrics_util": mutil}
    for mod, names in META["signatures"].items():
        for name, sig in names.items():
            fn = getattr(mods[mod], name)
            if sig is not None:
                ours = inspect.signature(fn)
                theirs = [p.split(":")[0].split("=")[0].strip() for p in sig.strip("()").split(",") if p.strip()] if "->" not in sig else None
                if theirs is not None:
                    assert [p if not p.startswith("**") else p for p in theirs] == [("**" if v.kind == v.VAR_KEYWORD else "") + k
                                                                                   for k, v in ours.parameters.items()], (mod, name, sig, str(ours))
    for name in ("distort_points", "J_distort_points"):
        with pytest.raises(NotImplementedError, match="pinhole"):
            getattr(utils, name)(None, None)
    # defaults that callers rely on
    d = {k: v.default for k, v in inspect.signature(depth.project).parameters.items()}
    assert d["ccth"] is None and d["sample_depth_fun"] is depth.sample_depth and d["sample_depth_kwargs"] is None
    assert inspect.signature(epipolar.sym_epipolar_distance_all).parameters["eps"].default == 1e-15
    assert inspect.signature(epipolar.sym_epipolar_distance).parameters["squared"].default is True
    for fn, name in ((wrappers.Pose, "transform"), (wrappers.Pose, "__matmul__"), (wrappers.Camera, "image2cam"), (wrappers.Camera, "cam2image")):
        assert callable(getattr(fn, name))
    assert "label_cc_th" in inspect.signature(pkg.DifferentTimeEvaluator.__init__).parameters
    assert callable(pairs.pair_overlap) and callable(NM.gt_matches_cc)
    assert pkg.native.lib().einx_abi_version() == 6  # additive symbols only


def test_plain_torch_helpers():
    v = torch.tensor([[1.0, 2.0, 3.0]])
    w = torch.tensor([[-2.0, 0.5, 4.0]])
    assert torch.equal((utils.skew_symmetric(v) @ w[..., None])[..., 0], torch.linalg.cross(v, w))
    assert utils.to_homogeneous(v).tolist() == [[1.0, 2.0, 3.0, 1.0]] and utils.to_homogeneous(v.numpy()).tolist() == [[1.0, 2.0, 3.0, 1.0]]
    with pytest.raises(ValueError):
        utils.to_homogeneous([1.0, 2.0])
    assert utils.from_homogeneous(torch.tensor([2.0, 4.0, 2.0])).tolist() == [1.0, 2.0]
    assert utils.batched_eye_like(torch.zeros(2, 5, dtype=torch.float64), 3).shape == (2, 3, 3)
    T = torch.eye(3)
    T[0, 2] = 2.0
    assert utils.transform_points(T, torch.tensor([[1.0, 1.0]])).tolist() == [[3.0, 1.0]]
    assert utils.is_inside(torch.tensor([[[1.0, 1.0], [0.0, 1.0], [3.0, 1.0]]]), torch.tensor([[3.0, 3.0]])).tolist() == [[True, False, False]]
    R = utils.so3exp_map(torch.tensor([[0.0, 0.0, np.pi / 2], [0.0, 0.0, 0.0]]))
    assert torch.allclose(R[0], torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), atol=1e-6) and torch.equal(R[1], torch.eye(3))
    g = utils.get_image_coords(torch.zeros(1, 2, 3))
    assert g.shape == (1, 2, 3, 2) and g[0, 1, 2].tolist() == [2.5, 1.5]
    pts = torch.tensor([[1.0, 5.0, -1.0], [1.0, 1.0, 1.0], [0.2, 0.9, 0.5]])
    H = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    assert mutil.warp_points(pts, H).tolist() == [[2.0, 6.0, 0.0], [1.0, 1.0, 1.0], pts[2].tolist()]
    kept, mask = mutil.keep_true_points(pts, H, (4, 4))
    assert mask.tolist() == [True, False, True] and kept[0].tolist() == [1.0, -1.0]
    best, idx = mutil.select_k_best_points(pts, 2)
    assert idx.tolist() == [1, 2] and best.shape == (3, 2)
    assert mutil.filter_points(pts, (4, 4))[1].tolist() == [True, False, False]


def test_wrappers_against_the_restatement():
    """Pose.transform, Camera.image2cam and Camera.cam2image compose to the restatement's forward projection (CPU tensors)"""
    c = F.occlusion_scene(257)
    for b in range(c.B):
        exp = F.occlusion_expected(257, None, True, True, np.float32)[b]
        cam0, cam1 = wrappers.Camera(torch.from_numpy(c.K0[b:b + 1])), wrappers.Camera(torch.from_numpy(c.K1[b:b + 1]))
        T = wrappers.Pose.from_4x4mat(torch.from_numpy(c.T01[b:b + 1]))
        d0, v0 = torch.from_numpy(c.pre[b][0])[None], torch.from_numpy(c.pre[b][1])[None]
        p3 = cam0.image2cam(torch.from_numpy(c.kp0[b])[None])
        assert p3.shape[-1] == 3 and (p3[..., 2] == 1).all()
        uv, ok = cam1.cam2image(T.transform(p3 * d0[..., None]))
        _same(uv[0].numpy(), exp["proj_0to1"], b)
        assert np.array_equal((ok & v0)[0].numpy(), exp["visible0"])
        assert torch.equal(T @ p3, T.transform(p3))
        back = (T.inv() @ T).to_4x4mat()
        assert torch.equal(back, torch.eye(4)[None])


# ------------------------------------------------------------------------------------------------ refusals
def test_named_refusals():
    with pytest.raises(NotImplementedError, match="kornia"):
        depth.sample_normals_from_depth(None, None, None)
    cam = wrappers.Camera(torch.eye(3)[None])
    T = wrappers.Pose.from_4x4mat(torch.eye(4)[None])
    with pytest.raises(TypeError, match="agg"):
        epipolar.generalized_epi_dist(torch.zeros(1, 2, 2), torch.zeros(1, 2, 2), cam, cam, T)
    with pytest.raises(RuntimeError, match="same number of pixels"):
        depth.dense_warp_consistency(torch.ones(1, 4, 6), torch.ones(1, 5, 5), T, cam, cam)
    with pytest.raises(TypeError, match="unexpected keyword"):
        depth.dense_warp_consistency(torch.ones(1, 4, 6), torch.ones(1, 6, 4), T, cam, cam, cc_th=1.0)
    with pytest.raises(ValueError, match="label_cc_th"):
        pkg.DifferentTimeEvaluator(None, 5, label_cc_th=0.0)
    gt = import_module(pkg.__name__ + ".core.geometry.gt_generation")
    assert "cc_th" in inspect.signature(gt.gt_matches_from_pose_depth).parameters  # stays refused there: an existing test pins it


def _project_params(**kw):
    p = _lib.GeomProjectParams()
    p.struct_size = kw.get("size", ctypes.sizeof(_lib.GeomProjectParams))
    p.B, p.sides, p.kp_yx, p.cc, p.cc_bound = kw.get("B", 2), kw.get("sides", 1), 0, kw.get("cc", 0), kw.get("bound", 1.0)
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for k in range(2):
        s = p.side[k]
        for name in s._ptrs:
            setattr(s, name, None if name in kw.get("null", ()) else ptr)
        s.cap, s.cols, s.H, s.W, s.Ho, s.Wo = kw.get("cap", 8), kw.get("cols", 2), 4, 4, kw.get("Ho", 4), 4
    return p, buf


PROJECT_BAD = {"struct_size": dict(size=8), "B_0": dict(B=0), "sides_3": dict(sides=3), "cap_0": dict(cap=0), "cols_1": dict(cols=1),
               "nan_bound": dict(cc=1, bound=float("nan")), "no_kp": dict(null=("kp",)), "no_motion": dict(null=("T", "T_other")),
               "no_depth": dict(null=("depth", "d_in", "valid_in")), "depth_without_validity": dict(null=("valid_in",)),
               "cc_without_other_depth": dict(cc=1, null=("depth_other", "dj_in", "validj_in")), "cc_other_map_size_0": dict(cc=1, Ho=0, null=("dj_in", "validj_in"))}


@pytest.mark.parametrize("name", list(PROJECT_BAD))
def test_c_refusals_project(name):
    """every refusal returns an error with a message that names the entry before anything touches the device"""
    L = pkg.native.lib()
    p, buf = _project_params(**PROJECT_BAD[name])
    assert L.einx_geom_project(ctypes.byref(p), None) != 0
    msg = L.einx_last_error().decode()
    assert msg.startswith("einx_geom_project: ") and len(msg) > len("einx_geom_project: "), msg


def test_c_refusals_other_entries():
    L = pkg.native.lib()
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert L.einx_geom_project(None, None) != 0 and L.einx_geom_dense_warp(None, None) != 0
    p = _lib.GeomDenseParams()
    p.struct_size = ctypes.sizeof(_lib.GeomDenseParams)
    p.B, p.sides, p.cc = 1, 1, 1
    p.counts = ptr
    for name in p.side[0]._ptrs:
        setattr(p.side[0], name, ptr)
    p.side[0].depth_other = None
    p.side[0].H, p.side[0].W = 4, 4
    assert L.einx_geom_dense_warp(ctypes.byref(p), None) != 0 and b"einx_geom_dense_warp: " in L.einx_last_error()
    p.cc, p.counts = 0, None
    assert L.einx_geom_dense_warp(ctypes.byref(p), None) != 0 and b"counts" in L.einx_last_error()
    assert L.einx_geom_sample(ptr, 1, 0, 4, 4, ptr, 4, 0, ptr, None, None) != 0 and b"einx_geom_sample: " in L.einx_last_error()
    assert L.einx_geom_sample(ptr, 1, 3, 4, 4, ptr, 4, 0, ptr, ptr, None) != 0 and b"valid" in L.einx_last_error()
    assert L.einx_epipolar_all(ptr, 4, ptr, 2, ptr, 1, 4, 4, 1e-15, ptr, None) != 0 and b"einx_epipolar_all: " in L.einx_last_error()
    assert L.einx_epipolar_all(ptr, 2, ptr, 2, ptr, 0, 4, 4, 1e-15, ptr, None) != 0
    # nothing to do is not an error, and nothing is launched
    assert L.einx_epipolar_all(None, 2, None, 2, None, 1, 0, 4, 1e-15, None, None) == 0
    assert L.einx_geom_sample(None, 1, 3, 4, 4, None, 0, 0, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ label_cc_th=None changes nothing
class _Feats:
    class det:
        positions, counts = "kp", "cnt"
    ordering = "yx"


def test_labels_without_cc_take_todays_path(monkeypatch):
    calls = []
    monkeypatch.setattr(NM, "gt_matches", lambda *a, **k: calls.append(("gt_matches", a, k)) or "plain")
    monkeypatch.setattr(NM, "gt_matches_cc", lambda *a, **k: calls.append(("gt_matches_cc", a, k)) or "cc")
    f = NM.batch_gt_matches.__wrapped__
    assert f(_Feats, _Feats, "d0", "d1", "K0", "K1", "T", None, 3, 5) == "plain"
    assert f(_Feats, _Feats, "d0", "d1", "K0", "K1", "T", None, 3, 5, cc_th=None) == "plain"
    assert calls[0] == calls[1] == ("gt_matches", ("kp", "kp", "cnt", "cnt", "d0", "d1", "K0", "K1", "T", None),
                                    {"pos_th": 3, "neg_th": 5, "ordering": "yx"})
    assert f(_Feats, _Feats, "d0", "d1", "K0", "K1", "T", None, 3, 5, cc_th=4.0) == "cc"
    assert calls[2][0] == "gt_matches_cc" and calls[2][2]["cc_th"] == 4.0
    E = pkg.DifferentTimeEvaluator
    assert inspect.signature(E.__init__).parameters["label_cc_th"].default is None
