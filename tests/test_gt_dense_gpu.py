"""GPU tests (-m gpu), component: dense-grid ground-truth matches and pair covisibility (csrc/gt_matches.hip gt_dense_*, DESIGN.md
8n).  (a) against the dense float64 restatement on exact inputs (tests/gt_dense_f64.py; test_gt_dense_cpu.py shows that fp32
evaluates them exactly and what each case plants), (b) against the generic gt_matches fed grid_keypoints on arbitrary inputs (both
evaluate the same fp32 expressions), (c) frame stacks and the counts-only call, (d) run twice and replayed from a graph into
poisoned buffers, (e) select_pairs against a loop over the generic path.  Every comparison is array_equal."""
from importlib import import_module

import numpy as np
import pytest
import torch

import gt_dense_f64 as D
from gpu_support import DEV, _np, _t, pkg

pytestmark = pytest.mark.gpu
M = import_module(pkg.__name__ + ".core.metrics._native_metrics")
G = import_module(pkg.__name__ + ".core.geometry.gt_generation")
P = import_module(pkg.__name__ + ".datasets.pairs")
N = import_module(pkg.__name__ + "._native")
DTYPES = {"matches0": torch.int64, "matches1": torch.int64, "matching_scores0": torch.float32, "matching_scores1": torch.float32,
          "proj_0to1": torch.float32, "proj_1to0": torch.float32, "depth_keypoints0": torch.float32, "depth_keypoints1": torch.float32,
          "valid0": torch.bool, "valid1": torch.bool, "visible0": torch.bool, "visible1": torch.bool, "counts": torch.int32}
KEYS = D.STAGE_A + D.STAGE_B


def _dense(c, T10=True, **kw):
    return M.gt_matches_dense(_t(c.depth0), _t(c.depth1), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10) if T10 else None, pos_th=c.pos_th,
                              neg_th=c.neg_th, **kw)


def _same_bits(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and _np(a[k]).tobytes() == _np(b[k]).tobytes(), (tag, k)


# ------------------------------------------------------------------------------------------------ (a) exact cases
@pytest.mark.parametrize("name", D.CASES)
def test_exact_cases(name):
    c = D.case(name)
    for T10 in (True, False):  # the explicit inverse, and the kernel's own (R^T, -R^T t): exact on these poses
        got = _dense(c, T10)
        for k in KEYS + ("counts",):
            exp = D.stacked(name, k)
            assert got[k].dtype == DTYPES[k] and tuple(got[k].shape) == exp.shape, (name, k, got[k].dtype, got[k].shape)
            assert np.array_equal(_np(got[k]).astype(exp.dtype), exp, equal_nan=True), (name, k, T10)
    cam = lambda K: G.Camera.from_calibration_matrix(_t(K))  # noqa: E731
    r = G.gt_matches_dense_grid(cam(c.K0), cam(c.K1), _t(c.depth0), _t(c.depth1), G.Pose.from_4x4mat(_t(c.T01)), G.Pose.from_4x4mat(_t(c.T10)),
                                pos_th=c.pos_th, neg_th=c.neg_th)
    assert "assignment" not in r and "reward" not in r and set(G.DENSE_GRID_KEYS) <= set(r)
    for k in G.DENSE_GRID_KEYS:
        assert r[k].dtype == DTYPES[k] and _np(r[k]).tobytes() == _np(got[k]).tobytes(), (name, k)
    for j, k in enumerate(("num_matches0", "num_matches1", "num_visible0", "num_visible1")):
        assert r[k].dtype == torch.int32 and np.array_equal(_np(r[k]), D.stacked(name, "counts")[:, j]), (name, k)
    ratio = D.stacked(name, "valid_ratio")
    assert r["valid_ratio"].dtype == torch.float32 and np.array_equal(_np(r["valid_ratio"]), ratio, equal_nan=True), name
    assert np.isnan(ratio).any() == (name == "behind")


# ------------------------------------------------------------------------------------------------ (b) the generic peer
def _generic(c, b=slice(None), depth0=None, depth1=None):
    """the generic gt_matches on the grid keypoints of both maps (ordering "yx", as check_indices calls it)"""
    d0, d1 = (c.depth0[b] if depth0 is None else depth0), (c.depth1[b] if depth1 is None else depth1)
    B = d0.shape[0]
    kp0 = P.grid_keypoints(*d0.shape[1:], "yx", DEV)[None].expand(B, -1, -1).contiguous()
    kp1 = P.grid_keypoints(*d1.shape[1:], "yx", DEV)[None].expand(B, -1, -1).contiguous()
    return M.gt_matches(kp0, kp1, None, None, _t(d0), _t(d1), _t(c.K0[b]), _t(c.K1[b]), _t(c.T01[b]), _t(c.T10[b]), pos_th=c.pos_th,
                        neg_th=c.neg_th, ordering="yx")


def _counts_of(r):
    return torch.stack([(r["matches0"] > -1).sum(1), (r["matches1"] > -1).sum(1), r["visible0"].sum(1), r["visible1"].sum(1)], 1).to(torch.int32)


@pytest.mark.parametrize("B,size0,size1,seed", [(3, (24, 32), (20, 28), 11), (3, (33, 47), (33, 47), 12), (1, (260, 346), (260, 346), 13)])
def test_equals_generic_gt_matches_on_arbitrary_inputs(B, size0, size1, seed):
    """non-exact seeded inputs (noisy depths with holes, rotations about all three axes, different intrinsics per side): both paths
    compute the same fp32 expressions, so every stage A and stage B output is equal bit for bit.  33 x 47 = 1551 points is no
    multiple of 64 or 256 and crosses the generic kernel's 1024-point chunk; 260 x 346 is the full MVSEC size."""
    c = D.random_scene(seed, B, size0, size1)
    got, exp = _dense(c), _generic(c)
    for k in KEYS:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, k
        assert _np(got[k]).tobytes() == _np(exp[k]).tobytes(), (k, int((_np(got[k]) != _np(exp[k])).sum()))
    assert torch.equal(got["counts"], _counts_of(exp))
    assert int(got["counts"][:, 0].min()) > size0[0] * size0[1] // 20  # scenes with matches
    if B == 1:
        return
    got2 = _dense(c, T10=False)  # the kernel's own inverse: the same code as the generic path's
    exp2 = M.gt_matches(P.grid_keypoints(*size0, "yx", DEV)[None].expand(B, -1, -1).contiguous(),
                        P.grid_keypoints(*size1, "yx", DEV)[None].expand(B, -1, -1).contiguous(), None, None, _t(c.depth0), _t(c.depth1),
                        _t(c.K0), _t(c.K1), _t(c.T01), None, pos_th=c.pos_th, neg_th=c.neg_th, ordering="yx")
    for k in KEYS:
        assert _np(got2[k]).tobytes() == _np(exp2[k]).tobytes(), k


# ------------------------------------------------------------------------------------------------ (c) frame stacks
def test_frame_stacks_and_counts_only():
    c = D.random_scene(21, 5, (24, 32), (24, 32))
    stack = np.concatenate([c.depth0, c.depth1[:2]])  # 7 frames, both sides read the same stack
    idx0, idx1 = [3, 3, 0, 6, 2], [5, 3, 0, 1, 2]  # repeats, and idx0 == idx1 in pairs 1, 2 and 4
    for dev_idx in (False, True):
        i0, i1 = (torch.tensor(i, dtype=torch.int32, device=DEV) if dev_idx else i for i in (idx0, idx1))
        got = M.gt_matches_dense(_t(stack), _t(stack), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10), idx0=i0, idx1=i1)
        for b in range(5):
            one = M.gt_matches_dense(_t(stack[idx0[b]][None]), _t(stack[idx1[b]][None]), _t(c.K0[b:b + 1]), _t(c.K1[b:b + 1]), _t(c.T01[b:b + 1]),
                                     _t(c.T10[b:b + 1]))
            for k in KEYS + ("counts",):
                assert _np(got[k][b]).tobytes() == _np(one[k][0]).tobytes(), (b, k)
        only = M.gt_matches_dense(_t(stack), _t(stack), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10), idx0=i0, idx1=i1, labels=False)
        assert set(only) == {"counts"} and torch.equal(only["counts"], got["counts"])
        cov = P.covisibility(_t(stack), _t(stack), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10), idx0=i0, idx1=i1)
        assert torch.equal(cov["counts"], got["counts"]) and cov["valid_ratio"].dtype == torch.float32
        assert np.array_equal(_np(cov["valid_ratio"]), np.array([D.ratio_f32(r) for r in _np(got["counts"])]), equal_nan=True)
    assert int(got["counts"][:, 0].min()) > 30
    # host-visible indices outside the stack are refused; device indices are clamped to [0, F)
    with pytest.raises(IndexError):
        M.gt_matches_dense(_t(stack), _t(stack), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10), idx0=[0, 1, 2, 3, 7], idx1=idx1)
    with pytest.raises(ValueError):
        M.gt_matches_dense(_t(stack[:3]), _t(stack), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10))  # no indices: a frame per pair
    with pytest.raises(ValueError):
        M.gt_matches_dense(_t(stack), _t(stack), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10), pos_th=0)
    wild = torch.tensor([9, -4, 0, 6, 2], dtype=torch.int32, device=DEV)
    clamped = M.gt_matches_dense(_t(stack), _t(stack), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10), idx0=wild, idx1=i1, labels=False)
    inside = M.gt_matches_dense(_t(stack), _t(stack), _t(c.K0), _t(c.K1), _t(c.T01), _t(c.T10), idx0=[6, 0, 0, 6, 2], idx1=idx1, labels=False)
    assert torch.equal(clamped["counts"], inside["counts"])


# ------------------------------------------------------------------------------------------------ (d) replay
def test_twice_and_graph_replay_into_poisoned_buffers(monkeypatch):
    c = D.random_scene(31, 3, (33, 47), (24, 32))
    args = [_t(a) for a in (c.depth0, c.depth1, c.K0, c.K1, c.T01, c.T10)]
    first, second = M.gt_matches_dense(*args), M.gt_matches_dense(*args)
    _same_bits(first, second, "twice")
    kept = []
    real = N._workspace

    def workspace(nbytes, device):
        kept.append(real(nbytes, device))
        return kept[-1]
    monkeypatch.setattr(N, "_workspace", workspace)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        out = M.gt_matches_dense(*args)
    ws = kept[-1]
    for poison in (0xFF, 0x00):  # NaN floats, -1 indices, all flags set; then zeros
        ws.fill_(poison)
        for k, v in out.items():
            v.view(torch.uint8).fill_(poison) if v.dtype != torch.bool else v.fill_(bool(poison))
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS + ("counts",):
            got = out[k].bool() if first[k].dtype == torch.bool else out[k]
            assert _np(got).tobytes() == _np(first[k]).tobytes(), (poison, k)


# ------------------------------------------------------------------------------------------------ (e) select_pairs end to end
def test_select_pairs_equals_a_loop_over_the_generic_path():
    """a synthetic 6-frame sequence of 40 x 52 maps: a camera moving sideways in front of a noisy slanted plane with holes"""
    F, H, W = 6, 40, 52
    c = D.random_scene(41, F, (H, W), (H, W), holes=15)
    depth = c.depth0
    K = D._kmat(48.0, W / 2, H / 2).astype(np.float32)
    poses = np.stack([D._pose(D._rot(0.004 * k, -0.01 * k, 0.02 * k), [0.11 * k, 0.02 * k, 0.01 * k]) for k in range(F)])
    indices = [(a, b) for a in range(F) for b in range(F)]  # the diagonal is skipped
    lo, hi = 0.6, 0.75  # every pair of this sequence lies inside the default (0.4, 0.8): a narrower range, the same rule
    r = P.select_pairs(depth, K, poses, indices, ratio_range=(lo, hi), batch=7)
    cand = np.array([p for p in indices if p[0] != p[1]])
    assert np.array_equal(r["candidates"], cand)
    T01, T10 = P.relative_transforms(poses, cand)
    kept, ratios = [], []
    sc = D.Case()
    sc.pos_th, sc.neg_th = 3, 5
    for i, (a, b) in enumerate(cand):
        sc.K0 = sc.K1 = K[None]
        sc.T01, sc.T10 = T01[i:i + 1], T10[i:i + 1]
        g = _generic(sc, depth0=depth[a:a + 1], depth1=depth[b:b + 1])
        cnt = _np(_counts_of(g))[0]
        assert np.array_equal(cnt, r["counts"][i]), (a, b)
        ratio = D.ratio_f32(cnt)
        ratios.append(ratio)
        if lo < ratio < hi:
            kept.append([a, b])
    assert np.array_equal(r["valid_ratio"], np.array(ratios, np.float32), equal_nan=True)
    assert r["pairs"].tolist() == kept and 0 < len(kept) < len(cand)  # the rule selects: some pairs in, some out
    one = P.select_pairs(depth, K, poses, indices, ratio_range=(lo, hi), batch=64)
    assert np.array_equal(one["pairs"], r["pairs"]) and np.array_equal(one["counts"], r["counts"])
    # frames, poses and indices that are device tensors already
    dev = P.select_pairs(_t(depth), _t(K), _t(poses), _t(np.array(indices)), ratio_range=(lo, hi), batch=7)
    assert np.array_equal(dev["pairs"], r["pairs"]) and np.array_equal(dev["counts"], r["counts"])
    # verify=True reports relative_pose on the dense matches of each kept pair and never touches the selection
    v = P.select_pairs(depth, K, poses, indices[:8], ratio_range=(lo, hi), verify=True)
    plain = P.select_pairs(depth, K, poses, indices[:8], ratio_range=(lo, hi))
    assert np.array_equal(v["pairs"], plain["pairs"]) and np.array_equal(v["counts"], plain["counts"]) and len(v["pairs"]) > 0
    for k in ("R_err", "t_err", "inliers"):
        assert v[k].shape == (len(v["pairs"]),) and v[k].dtype == np.float64 and not np.isnan(v[k]).any(), k
    found = np.isfinite(v["R_err"])
    assert found.any() and (v["inliers"][found] > 0).all() and (v["inliers"][found] <= 1).all()
    assert P.select_pairs(depth, K, poses, indices)["pairs"].tolist() == [[a, b] for (a, b), q in zip(cand, ratios) if 0.4 < q < 0.8]
