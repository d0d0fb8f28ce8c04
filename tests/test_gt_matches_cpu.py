"""CPU tests of the ground-truth matches: the numpy restatement (tests/gt_matches_ref.py) against the reference's
fixture (tests/golden/gt_matches.npz), the fixture's own margins, and the host-side parts of the package (size query, refusals,
the Pose / Camera holders).

Tolerances: floats against the reference within the fixture's stored bound = 2 x the reference's own measured float32 noise
(against float64) + 4 ulp of the largest coordinate / depth; nothing is typed in here.  Discrete outputs are compared exactly:
the generator searched seeds until every decision of the reference clears its threshold by 16 noise floors."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import gt_matches_ref as R
from helpers import Golden, load_pkg

pkg = load_pkg()
_lib = import_module(pkg.__name__ + "._lib")
G = Golden("gt_matches")
POSE = [(name, b) for name in R.POSE_CASES for b in range(G.cases[name]["B"])]


def _pair(name, b):
    c = G.cases[name]
    sc = R.POSE_CASES[name](c["seed"])
    n, m = int(sc["n"][b]), int(sc["m"][b])
    return c, sc, n, m, R.fixture_pair(G, f"{name}.{b}", n, m)


def _close(got, exp, bound, what):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(exp)), f"{what}: NaN pattern"
    fin = ~np.isnan(exp)
    err = float(np.abs(got - exp)[fin].max()) if fin.any() else 0.0
    print(f"{what}: max |error| {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


@pytest.mark.parametrize("name,b", POSE, ids=[f"{n}{b}" for n, b in POSE])
def test_restatement_equals_reference_pose_form(name, b):
    c, sc, n, m, exp = _pair(name, b)
    pre = R.precomputed_depths(sc, b) if name == "b" else None
    if exp is None:  # the early return: n == 0 or m == 0
        m0, m1, _ = R.label(sc["kp0"][b, :n], sc["kp1"][b, :m], None, None, None, None, None, None, c["pos_th"], c["neg_th"])
        assert np.array_equal(m0, G[f"{name}.{b}.tuple.matches0"]) and np.array_equal(m1, G[f"{name}.{b}.tuple.matches1"])
        assert G[f"{name}.{b}.tuple.assignment"].shape == (n, m) and (m0 == -1).all() and (m1 == -1).all()
        return
    e = R.project(sc, b, np.float32, depths=pre)
    for side in "01":
        assert np.array_equal(e[f"visible{side}"], exp[f"visible{side}"])
        _close(e[f"d{side}"], exp[f"depth_keypoints{side}"], c["bounds"]["depth"], f"{name}.{b} depth{side}")
    _close(e["proj01"], exp["proj_0to1"], c["bounds"]["proj"], f"{name}.{b} proj_0to1")
    _close(e["proj10"], exp["proj_1to0"], c["bounds"]["proj"], f"{name}.{b} proj_1to0")
    kp0, kp1 = sc["kp0"][b, :n], sc["kp1"][b, :m]
    m0, m1, pos0 = R.label(kp0, kp1, e["proj01"], e["proj10"], e["visible0"], e["visible1"], e["valid0"], e["valid1"], c["pos_th"], c["neg_th"])
    assert np.array_equal(m0, exp["matches0"]) and np.array_equal(m1, exp["matches1"])
    assert np.array_equal(R.assignment_from_pos0(pos0, m), exp["assignment"])
    rw = R.reward_pose(kp0, kp1, e["proj01"], e["proj10"], e["visible0"], e["visible1"], sc["K0"][b], sc["K1"][b], sc["T01"][b], c["pos_th"], c["neg_th"])
    sure = np.ones(n * m, bool)
    sure[exp["reward_unsure"]] = False
    assert c["dense_margins"] is False or sure.all()
    assert np.array_equal(rw.reshape(-1)[sure], exp["reward"].reshape(-1)[sure])
    assert sure.mean() > 0.999


@pytest.mark.parametrize("name", ["c", "c_neg_lt_pos"])
def test_restatement_equals_reference_homography_form(name):
    c = G.cases[name]
    sc = R.homography_scene(c["seed"], c["B"], c["n"], c["m"])
    for b in range(c["B"]):
        p01, p10 = R.warp(sc["kp0"][b], sc["H"][b]), R.warp(sc["kp1"][b], sc["H"][b], inverse=True)
        _close(p01, G[f"{name}.proj_0to1"][b], c["bounds"]["proj"], f"{name}.{b} proj_0to1")
        _close(p10, G[f"{name}.proj_1to0"][b], c["bounds"]["proj"], f"{name}.{b} proj_1to0")
        m0, m1, pos0 = R.label(sc["kp0"][b], sc["kp1"][b], p01, p10, None, None, None, None, c["pos_th"], c["neg_th"])
        assert np.array_equal(m0, G[f"{name}.matches0"][b]) and np.array_equal(m1, G[f"{name}.matches1"][b])
        n, m = c["n"], c["m"]
        assert np.array_equal(R.assignment_from_pos0(pos0, m), np.unpackbits(G[f"{name}.assignment"]).reshape(-1)[:c["B"] * n * m].reshape(c["B"], n, m)[b])
        assert np.array_equal(R.reward_homography(sc["kp0"][b], sc["kp1"][b], p01, p10, c["pos_th"], c["neg_th"]), G[f"{name}.reward"][b])
    if name == "c_neg_lt_pos":
        assert c["neg_th"] < c["pos_th"] and (G[f"{name}.reward"] == 0).any()


def test_stored_margins_clear_the_stored_floors():
    """margins are stored in units of their floor; every decision the tests compare exactly clears MARGIN floors"""
    factor = G.meta["margin_factor"]
    assert factor >= 16
    for c in G.meta["cases"]:
        need = ["neg", "argmin"] + (["front", "inside"] if c["kind"] == "pose" else ["reward_pos", "reward_neg"])
        if c["kind"] == "pose" and c["dense_margins"]:
            need += ["reward_pos", "reward_epi"]
        for k in need:
            assert c["margins"][k] >= factor, (c["name"], k, c["margins"][k])
        assert all(v > 0 for v in c["floors"].values())
    assert G.cases["d"]["dense_margins"] is False and all(G.cases[k]["dense_margins"] for k in "ab")


@pytest.mark.parametrize("name,b", [p for p in POSE if p != ("a", 2)], ids=lambda v: str(v))
def test_labelling_of_reference_projections_is_bit_exact(name, b):
    """stage B is exact arithmetic on given projections: fed the reference's own proj_* / visible*, it gives the reference's labels"""
    c, sc, n, m, exp = _pair(name, b)
    pre = R.precomputed_depths(sc, b) if name == "b" else None
    valid = R.project(sc, b, np.float32, depths=pre)  # validity of the sampled depths: exact (asserted through `visible` above)
    m0, m1, pos0 = R.label(sc["kp0"][b, :n], sc["kp1"][b, :m], exp["proj_0to1"], exp["proj_1to0"], exp["visible0"], exp["visible1"],
                           valid["valid0"], valid["valid1"], c["pos_th"], c["neg_th"])
    assert np.array_equal(m0, exp["matches0"]) and np.array_equal(m1, exp["matches1"])
    assert np.array_equal(R.assignment_from_pos0(pos0, m), exp["assignment"])


def test_average_precision_closed_form():
    """AP = precision x (recall - r_first) against the reference's cumulative-sum expression: at most 1023 float32 differences of
    magnitude <= 1 are summed there, an error of at most 1023 * 2^-24 = 6.1e-5 < 1e-4; the ratios themselves are 1-ulp float32"""
    cases = R.pr_cases()
    assert set(cases) == {"mixed", "full", "tiny", "all_ignored", "no_prediction"}
    for name, (m, gt, sc) in cases.items():
        got = np.stack([R.match_pr(m[b], gt[b], sc[b]) for b in range(len(m))])
        err = np.abs(got - G[f"pr.{name}"]).max()
        print(f"pr.{name}: max |closed form - reference| {err:.2e}")
        assert err <= 1e-4, name
    assert G["pr.mixed"][0, 3] > 0.1 and (G["pr.all_ignored"] == 0).all() and (G["pr.no_prediction"][:, :2] == 0).all()
    assert np.isnan(R.match_pr(np.zeros(0), np.zeros(0), np.zeros(0))).all()


def _params(B=3, cap0=70, cap1=90, cols0=2, cols1=2, size=None):
    p = _lib.GtMatchesParams()
    p.struct_size = ctypes.sizeof(_lib.GtMatchesParams) if size is None else size
    p.B, p.cap0, p.cap1, p.cols0, p.cols1 = B, cap0, cap1, cols0, cols1
    return p


def test_workspace_query():
    L = pkg.native.lib()
    q = lambda p: L.einx_gt_matches_ws_bytes(ctypes.byref(p))  # noqa: E731
    small, full = q(_params()), q(_params(32, 1024, 1024, 3, 3))
    assert small > 0 and small % 256 == 0
    assert full >= 32 * (1024 + 1024) * 12 and full < 2 * 32 * (1024 + 1024) * 12  # three words per keypoint, no N x M region
    for bad in (_params(B=0), _params(cap0=0), _params(cap1=-1), _params(cols0=1), _params(cols1=0), _params(size=8), _params(B=70000)):
        assert q(bad) == 0
    assert L.einx_gt_matches_ws_bytes(None) == 0
    assert L.einx_abi_version() == 6  # additive symbols only


def test_refused_arguments_and_empty_input():
    gt = import_module(pkg.__name__ + ".core.geometry.gt_generation")
    W = import_module(pkg.__name__ + ".core.geometry.wrappers")
    kp0, kp1 = torch.zeros(1, 4, 2), torch.zeros(1, 5, 2)
    K = torch.eye(3)[None]
    cam, T = W.Camera.from_calibration_matrix(K), W.Pose.from_4x4mat(torch.eye(4)[None])
    depth = torch.ones(1, 8, 8)
    with pytest.raises(NotImplementedError, match="epi_th"):
        gt.gt_matches_from_pose_depth(kp0, kp1, cam, cam, depth, depth, T, T, epi_th=1.0)
    with pytest.raises(NotImplementedError, match="cc_th"):
        gt.gt_matches_from_pose_depth(kp0, kp1, cam, cam, depth, depth, T, T, cc_th=1.0)
    with pytest.raises(NotImplementedError, match="pinhole"):
        W.Camera(K, distortion=torch.zeros(1, 2))  # two distortion parameters
    W.Camera(K, distortion=torch.zeros(1, 0))
    assert (gt.IGNORE_FEATURE, gt.UNMATCHED_FEATURE) == (-2, -1)
    # the reference's quirk: a TUPLE when either side is empty (no device needed: nothing is launched)
    for fn, args in ((gt.gt_matches_from_pose_depth, (cam, cam, depth, depth, T, T)), (gt.gt_matches_from_homography, (torch.eye(3)[None],))):
        for a, b in ((kp0[:, :0], kp1), (kp0, kp1[:, :0])):
            r = fn(a, b, *args)
            assert isinstance(r, tuple) and len(r) == 3
            assert r[0].shape == (1, a.shape[1], b.shape[1]) and r[0].dtype == torch.bool and not r[0].any()
            assert r[1].dtype == torch.int64 and r[1].shape == (1, a.shape[1]) and (r[1] == -1).all()
            assert r[2].dtype == torch.int64 and r[2].shape == (1, b.shape[1]) and (r[2] == -1).all()


def test_pose_and_camera_holders():
    W = import_module(pkg.__name__ + ".core.geometry.wrappers")
    sc = R.scene_a(G.cases["a"]["seed"])
    T = torch.from_numpy(sc["T01"])
    P = W.Pose.from_4x4mat(T)
    assert torch.equal(P.R, T[:, :3, :3]) and torch.equal(P.t, T[:, :3, 3]) and torch.equal(P.to_4x4mat(), T)
    Q = W.Pose.from_Rt(P.R, P.t)
    assert torch.equal(Q.R, P.R) and torch.equal(Q.t, P.t)
    np.testing.assert_allclose(P.inv().to_4x4mat().numpy(), sc["T10"], atol=1e-6)
    np.testing.assert_allclose(P.inv().inv().to_4x4mat().numpy(), sc["T01"], atol=1e-6)
    np.testing.assert_allclose(R.invert_pose_f32(sc["T01"]), sc["T10"], atol=1e-6)  # the kernel's NULL-T_1to0 path
    with pytest.raises(ValueError):
        W.Pose.from_Rt(torch.eye(3)[None], torch.zeros(2, 3))
    K = torch.from_numpy(sc["K1"])
    cam = W.Camera.from_calibration_matrix(K)
    assert torch.equal(cam.calibration_matrix(), K)
    assert cam.size[0].tolist() == [100.0, 48.0] and cam.f[0].tolist() == [80.0, 80.0] and cam.c[0].tolist() == [50.0, 24.0]
    skewed = K.clone()
    skewed[:, 0, 1] = 0.3  # only focal lengths and the principal point are the camera's
    assert torch.equal(W.Camera.from_calibration_matrix(skewed).calibration_matrix(), K)


def test_same_time_evaluator_refuses_depth():
    """a same-time item that carries depth maps is an error, not something dropped silently; the different-time evaluator wants
    the pose beside them (host logic only: no device is touched)"""
    H = import_module(pkg.__name__ + ".harness")
    same, diff = object.__new__(pkg.SameTimeEvaluator), object.__new__(pkg.DifferentTimeEvaluator)
    batch = lambda pose, depth: H._Batch([], None, None, pose, depth)  # noqa: E731
    same._validate(batch(None, None))  # accepted: does not raise
    diff._validate(batch(None, None))
    with pytest.raises(ValueError, match="SameTimeEvaluator takes no depth"):
        same._validate(batch(("K0", "K1", "T"), ("d0", "d1")))
    with pytest.raises(ValueError, match="pose"):
        diff._validate(batch(None, ("d0", "d1")))
    diff._validate(batch(("K0", "K1", "T"), ("d0", "d1")))
