"""Relative pose on the device (csrc/pose.hip): the kernels against the float64 restatement of the contract (tests/pose_f64.py),
the reference's RelativePoseEstimation API on top of them, and DifferentTimeEvaluator's pose path."""
import numpy as np
import pytest
import torch

import pose_f64 as P
from gpu_support import DEV, _np, _t, pkg, synth

pytestmark = pytest.mark.gpu
from importlib import import_module  # noqa: E402

_nm = import_module(pkg.__name__ + ".core.metrics._native_metrics")
_mm = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
CODES = {v: k for k, v in _nm.POSE_STATUS.items()}
CAP = 1024


def _batch():
    """B = 18 ragged pairs: N in {5, 6, 8, 50, 300, 1024}, several outlier ratios, degenerate sets, forward driving"""
    rng = np.random.default_rng(2024)
    spec = [(5, 0.0, 0.0), (6, 0.0, 0.0), (8, 0.3, 0.0), (50, 0.5, 0.2), (300, 0.5, 0.3), (1024, 0.5, 0.1), (50, 0.0, 0.0),
            (300, 0.5, 0.6), (8, 0.5, 0.0), (1024, 0.5, 0.3), (300, 0.0, 0.0), (6, 0.5, 0.0)]
    pairs = [P.scene(rng, n, noise=nz, outliers=o) for n, nz, o in spec]
    k0, k1, K, _, T = P.scene(rng, 40)
    same = np.repeat(k0[:1], 40, 0)
    pairs.append((same, same.copy(), K, K.copy(), T))                            # every point identical
    line = np.stack([np.linspace(20, 200, 30), np.linspace(30, 150, 30), np.ones(30)], 1).astype(np.float32)
    pairs.append((line, line[::-1].copy(), K, K.copy(), T))                       # collinear
    pairs.append((k0[:4], k1[:4], K, K.copy(), T))                                # N < 5
    pairs.append((k0[:0], k1[:0], K, K.copy(), T))                                # no match at all
    pairs.append(P.scene(rng, 200, t_dir=P.FORWARD, max_deg=3.0))                  # 16: forward driving, noise free
    pairs.append(P.scene(rng, 300, noise=0.5, outliers=0.3, t_dir=P.FORWARD, max_deg=3.0))  # 17: forward, 30 % outliers
    return pairs


def _stack(pairs):
    B = len(pairs)
    mk0 = np.zeros((B, CAP, 3), np.float32)
    mk1 = np.zeros((B, CAP, 3), np.float32)
    nm = np.zeros(B, np.int32)
    for b, (a0, a1, _, _, _) in enumerate(pairs):
        mk0[b, :len(a0)], mk1[b, :len(a1)], nm[b] = a0, a1, len(a0)
    K0 = np.stack([p[2] for p in pairs])
    K1 = np.stack([p[3] for p in pairs])
    T = np.stack([p[4] for p in pairs])
    return _t(mk0), _t(mk1), _t(nm), _t(K0), _t(K1), _t(T)


def _run(args, **kw):
    return [_np(x) for x in _nm.relative_pose(*args, **kw)]


@pytest.fixture(scope="module")
def batch():
    pairs = _batch()
    args = _stack(pairs)
    out = _run(args)
    torch.cuda.synchronize()
    ref = [P.relative_pose(a0, a1, K0, K1) for a0, a1, K0, K1, _ in pairs]
    return pairs, args, out, ref


# pairs whose chosen iteration differs between the two solver routes for an understood reason (none: pair 17, forward driving
# with 30 % outliers, was pinned here until the degree-10 polynomial kept its small leading coefficients)
ITER_DIFFERS = set()


def test_kernel_matches_restatement(batch):
    pairs, _, (R, t, mask, status, rows), ref = batch
    near, worst = [], [0.0, 0.0, 0.0]
    for b, r in enumerate(ref):
        n = len(pairs[b][0])
        if b in ITER_DIFFERS:  # pinned: reported, and held to ground truth by test_ground_truth_bounds
            assert status[b] >= 0 and (status[b] >> 4) != r["it"][0], f"pair {b} now agrees: unpin it"
            continue
        if r["status"] != "ok":
            assert status[b] == CODES[r["status"]], (b, status[b], r["status"])
            assert not mask[b].any() and np.all(np.isinf(rows[b, :3])) and rows[b, 3] == 0.0
            continue
        it, s = r["it"]
        # the chosen iteration must agree; the solution's index inside the sample may not (a root that one route keeps and the
        # other loses to the det E guard shifts the indices), the model itself is compared through R and t below
        assert status[b] >= 0 and (status[b] >> 4) == it, (b, status[b], r["it"])
        assert not mask[b, n:].any(), b  # past the pair's matches the mask is zero
        diff = np.nonzero(mask[b, :n] != r["mask"])[0]
        if len(diff):  # allowed only where the float64 error sits within 1e-6 (relative) of thr^2: reported
            a0, a1, K0, K1 = pairs[b][:4]
            x1, x2 = P.normalize(a0[:, 1::-1], K0), P.normalize(a1[:, 1::-1], K1)
            thr2 = P.ransac_threshold(1.0, K0, K1) ** 2
            _, e64 = P.sampson_f32(r["E"], x1, x2)
            assert np.all(np.abs(e64[diff] - thr2) <= 1e-6 * thr2), f"pair {b}: mask differs at {diff[:10]}"
            near.append((b, diff.tolist()))
        # both solver routes polish every solution by Gauss-Newton on the essential constraints of E itself
        e = P.pose_errors(pairs[b][4], r["R"], r["t"])
        d = (np.abs(R[b] - r["R"]).max(), min(np.abs(t[b] - r["t"]).max(), np.abs(t[b] + r["t"]).max()), np.abs(rows[b, :3] - e).max())
        worst = [max(w, v) for w, v in zip(worst, d)]
        assert not np.isnan(R[b]).any()
        assert rows[b, 3] == r["mask"].mean()
    assert worst[0] < 1e-9 and worst[1] < 1e-9 and worst[2] < 1e-5, f"max |dR|, |dt|, |d errors| = {worst}"
    assert not near, f"near-threshold mask differences (allowed, none expected with these seeds): {near}"


def test_ground_truth_bounds(batch):
    """the CPU test's bounds (tests/pose_f64.py:GT_BOUNDS): noise-free pairs, 0.5 px noise with 10-60 % outliers, forward driving"""
    pairs, _, (R, t, mask, status, rows), _ = batch
    bounds = {6: "noise_free", 10: "noise_free", 16: "noise_free", 4: "outliers_30", 5: "outliers_30", 9: "outliers_30",
              17: "outliers_30", 7: "outliers_60"}
    for b, k in bounds.items():
        assert status[b] >= 0 and rows[b, 2] < P.GT_BOUNDS[k], (b, rows[b])
        if k == "noise_free":
            assert rows[b, 3] == 1.0, (b, rows[b])


LOST_ROOTS = {9: 2}  # problem 9: four real roots within 0.11 of each other (z = -1.4947 .. -1.3913): the device finds two


def test_essential_5pt_matches_restatement():
    rng = np.random.default_rng(7)
    x1, x2 = rng.normal(size=(24, 5, 2)), rng.normal(size=(24, 5, 2))
    E, ns = _nm.essential_5pt(_t(x1), _t(x2))
    E, ns = _np(E), _np(ns)
    lost = {}
    for i in range(24):
        ref = P.solve5(x1[i], x2[i])
        # every kernel solution is one of the restatement's (same order); on clustered roots the degree-10 polynomial can lose a
        # pair of close real roots in fp64: the problems where that happens with these seeds are pinned below
        zr = [Er[2, 1] for Er in ref]
        prev = -1
        for k in range(ns[i]):
            j = int(np.argmin([abs(E[i, k, 2, 1] - z) for z in zr]))
            assert j > prev
            prev = j
            assert np.abs(E[i, k] - ref[j]).max() < 5e-8 * max(1.0, np.abs(ref[j]).max()), (i, k)  # worst of these seeds: 1.1e-8
        if ns[i] != len(ref):
            lost[i] = len(ref) - int(ns[i])
    assert lost == LOST_ROOTS, f"roots lost by the kernel per problem: {lost}"


def test_batch_alone_repeat_and_graph(batch):
    pairs, args, out, _ = batch
    for b in (4, 0, 9):
        one = _run([a[b:b + 1] for a in args])
        for x, y in zip(one, out):
            assert np.array_equal(x[0], y[b], equal_nan=True), b
    again = _run(args)
    for x, y in zip(again, out):
        assert np.array_equal(x, y, equal_nan=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _nm.relative_pose(*args)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = _nm.relative_pose(*args)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(res, out):
        assert np.array_equal(_np(x), y, equal_nan=True)


def test_reference_api(batch, capsys):
    pairs, _, (R, t, mask, status, rows), _ = batch
    rpe = _mm.RelativePoseEstimation("RPE", pose_thresh=[5, 10, 20])
    for b in (4, 14):  # a pose and the < 5 failure path
        a0, a1, K0, K1, T = pairs[b]
        # T in float64: with a float32 T the reference takes |t_gt| in float32 (BLAS sdot), the device in float64
        d = rpe.update_one(_t(a0), _t(a1), torch.from_numpy(K0), torch.from_numpy(K1), torch.from_numpy(T.astype(np.float64)))
        keys = ["RPE_R_errs", "RPE_t_errs", "RPE_pose_errs", "RPE_inliers"] + [f"RPE@{k}_ratio" for k in (5, 10, 20)]
        assert list(d) == keys
        if b == 14:
            assert d["RPE_R_errs"] == np.inf and d["RPE_inliers"] == 0.0 and d["RPE@5_ratio"] == 0.0
            assert "Not enough points" in capsys.readouterr().out
        else:
            np.testing.assert_allclose([d["RPE_R_errs"], d["RPE_t_errs"], d["RPE_pose_errs"]], rows[b, :3], atol=1e-5)
            assert d["RPE_inliers"] == rows[b, 3]
            assert isinstance(d["RPE@5_ratio"], np.float32)
    assert len(rpe.error_list) == 2 and rpe.error_list[1] == np.inf
    assert set(rpe.compute_all_auc()) == {"5", "10", "20"}
    sel = [4, 5, 14]
    out = rpe.update_batch([_t(pairs[b][0]) for b in sel], [_t(pairs[b][1]) for b in sel], [torch.from_numpy(pairs[b][2]) for b in sel],
                           [torch.from_numpy(pairs[b][3]) for b in sel], [torch.from_numpy(pairs[b][4].astype(np.float64)) for b in sel])
    assert len(rpe.error_list) == 3
    assert abs(out["RPE_pose_errs"] - np.mean(rows[[4, 5], 2])) < 1e-5
    auc = _mm.compute_auc(list(rows[sel, 2]), [5, 10, 20])
    for k in (5, 10, 20):
        assert abs(out[f"RPE@{k}_auc"] - auc[str(k)]) < 1e-6


def _model():
    cfg = pkg.default_config("SP_MNN", event_channels=5)
    for sec in (cfg.event_extractor.vgg, cfg.image_extractor.superpointv1):
        sec.detection_top_k = 128
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=33)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    return model


def test_harness_pose_path():
    from helpers import synth_raw_events
    model = _model()
    H, W, B = 100, 124, 3
    evs = [synth_raw_events(dict(seed=500 + b, n=6000, H=H, W=W, bins=5, frac=False, pneg=False)) for b in range(B)]
    img = synth.synth_image(92, B, H, W)
    rng = np.random.default_rng(5)
    K = np.array([[60.0, 0, W / 2], [0, 61.0, H / 2], [0, 0, 1]], np.float32)
    T = np.stack([np.eye(4)] * B)  # float64 (see test_reference_api)
    for b in range(B):
        T[b, :3, :3] = P.rotation(rng.normal(size=3), 5.0)
        T[b, :3, 3] = rng.normal(size=3)
    K0, K1, Td = _t(np.stack([K] * B)), _t(np.stack([K] * B)), _t(T)
    plain = pkg.DifferentTimeEvaluator(model, bins=5, resolution=(W, H))
    rows0, _ = plain.step(evs, _t(img.copy()))
    with_pose = pkg.DifferentTimeEvaluator(model, bins=5, resolution=(W, H))
    rows1, (_, _, m) = with_pose.step(evs, _t(img.copy()), None, pose=(K0, K1, Td))
    assert torch.equal(rows0, rows1)
    assert set(plain.result()) == set(plain.names)
    res = with_pose.result()
    rpe = _mm.RelativePoseEstimation("RPE", pose_thresh=[5, 10, 20])
    per = []
    for b in range(B):
        per.append(rpe.update_one(m["matched_kpts0"][b], m["matched_kpts1"][b], torch.from_numpy(K), torch.from_numpy(K), torch.from_numpy(T[b])))
    for k in per[0]:
        v = np.array([d[k] for d in per], np.float64)
        v = v[np.isfinite(v)]
        ref = np.mean(v) if len(v) else np.nan
        if k.endswith("_ratio"):
            assert res[k] == ref or (np.isnan(res[k]) and np.isnan(ref)), k
        else:
            np.testing.assert_allclose(res[k], ref, atol=1e-5, equal_nan=True, err_msg=k)
    auc = rpe.compute_all_auc()
    for t in (5, 10, 20):
        assert abs(res[f"RPE@{t}_auc"] - auc[str(t)]) < 1e-8
    assert set(res) == set(plain.names) | set(per[0]) | {f"RPE@{t}_auc" for t in (5, 10, 20)}
    # run() with the pose as the 4th element of an item: the same rows and the same pose keys
    runner = pkg.DifferentTimeEvaluator(model, bins=5, resolution=(W, H))
    got = list(runner.run([(evs, _t(img.copy()), None, (K0, K1, Td))]))
    assert torch.equal(got[0][0], rows0)
    r2 = runner.result()
    for k in res:
        assert r2[k] == res[k] or (np.isnan(r2[k]) and np.isnan(res[k])), k
