"""Homography on the device (csrc/homography.hip): the kernels against the float64 restatement of the contract
(tests/homography_f64.py) and against ground truth, the reference's HomographyEstimation API on top of them, and
SameTimeEvaluator's HE path.

Measured on the MI355X over `homography_f64.batch()`: |H_dev - H_f64|_F / |H_f64|_F at most 5.4e-10 (pairs 9 and
15, the tail of the polish; 1e-13 or less on most pairs), HE_errors equal on every pair, einx_homography_dlt within 3.3e-11
(4 points) and 6.1e-14 (50 points) of numpy; each gate below is 10 x its measured value.  No pair is pinned."""
import numpy as np
import pytest
import torch

import homography_f64 as Hm
from gpu_support import DEV, _np, _t, pkg, synth

pytestmark = pytest.mark.gpu
from importlib import import_module  # noqa: E402

_nm = import_module(pkg.__name__ + ".core.metrics._native_metrics")
_mm = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
CODES = {v: k for k, v in _nm.HOMOGRAPHY_STATUS.items()}
CAP = 1024
THR = (3, 5, 10)

# gates = 10 x the largest difference measured on the MI355X over this batch (two fp64 implementations with different
# eigen-solvers and reduction orders)
H_MEASURED, H_GATE = 5.412e-10, 5.412e-9          # |H_dev - H_f64|_F / |H_f64|_F
ERR_MEASURED, ERR_GATE = 0.0, 0.0                 # |HE_errors_dev - HE_errors_f64| in px: both sides round H to the same float32
DLT_MEASURED = {4: 3.258e-11, 50: 6.132e-14}       # einx_homography_dlt against numpy, relative Frobenius
DLT_GATE = {k: 10 * v for k, v in DLT_MEASURED.items()}
PINNED = set()  # pairs that diverge for an understood reason (none)


def _stack(pairs, cols=3, ordering="yx"):
    B = len(pairs)
    mk0 = np.zeros((B, CAP, cols), np.float32)
    mk1 = np.zeros((B, CAP, cols), np.float32)
    nm = np.zeros(B, np.int32)
    for b, (a0, a1, _) in enumerate(pairs):
        if ordering == "xy":
            a0, a1 = a0.copy(), a1.copy()
            a0[:, :2], a1[:, :2] = a0[:, 1::-1], a1[:, 1::-1]
        mk0[b, :len(a0)], mk1[b, :len(a1)], nm[b] = a0[:, :cols], a1[:, :cols], len(a0)
    Ht = np.stack([p[2] for p in pairs]).astype(np.float32)
    return _t(mk0), _t(mk1), _t(nm), _t(np.array([Hm.IMG_SHAPE] * B, np.int32)), _t(Ht)  # the shape on the device: capturable


def _run(args, **kw):
    return [_np(x) for x in _nm.homography(*args, **kw)]


@pytest.fixture(scope="module")
def batch():
    pairs = Hm.batch()
    args = _stack(pairs)
    out = _run(args)
    torch.cuda.synchronize()
    ref = [Hm.homography(a0, a1) for a0, a1, _ in pairs]
    return pairs, args, out, ref


def test_kernel_matches_restatement(batch):
    pairs, _, (H, mask, status, rows), ref = batch
    worst_h, worst_e = 0.0, 0.0
    assert len(PINNED) <= 2
    for b, r in enumerate(ref):
        n = len(pairs[b][0])
        want = Hm.rows(r, pairs[b][2].astype(np.float32), Hm.IMG_SHAPE, THR)
        if r["status"] != "ok":
            assert Hm.BATCH_FAIL[b] == r["status"]
            assert status[b] == CODES[r["status"]], (b, status[b], r["status"])
            assert not mask[b].any() and not H[b].any() and rows[b].tolist() == want
            continue
        assert b not in Hm.BATCH_FAIL
        assert status[b] == r["it"], (b, status[b], r["it"])
        assert np.array_equal(mask[b, :n], r["mask"]) and not mask[b, n:].any(), b
        dh = np.linalg.norm(H[b] - r["H"]) / np.linalg.norm(r["H"])
        de = abs(rows[b, 3] - want[3])
        print(f"pair {b}: N {n} it {status[b]} |dH| rel {dh:.3e} HE_errors {rows[b, 3]:.6f} diff {de:.3e}")
        worst_h, worst_e = max(worst_h, dh), max(worst_e, de)
        assert rows[b, 4] == want[4], b
        # the restatement's error is farther than the gate from every threshold, for EVERY pair: the ratios must be equal
        assert all(abs(want[3] - t) > ERR_GATE for t in THR), b
        assert rows[b, :3].tolist() == want[:3], b
    print(f"measured: max |dH| rel {worst_h:.3e}, max |d HE_errors| {worst_e:.3e} px")
    assert worst_h < 1e-6, "a difference of this size between two fp64 routes is a bug, not a gate"
    assert worst_h <= H_GATE and worst_e <= ERR_GATE, (worst_h, worst_e)


def test_ground_truth(batch):
    """every pair with N >= 50, at most 50 % outliers and at most 0.5 px noise: mean corner error below the script's smallest
    threshold, for the kernels and for the restatement alone"""
    pairs, _, (H, mask, status, rows), ref = batch
    assert len(Hm.BATCH_GT) >= 6
    for b in Hm.BATCH_GT:
        want = Hm.rows(ref[b], pairs[b][2].astype(np.float32), Hm.IMG_SHAPE, THR)
        assert status[b] >= 0 and rows[b, 3] < Hm.GT_BOUND and want[3] < Hm.GT_BOUND, (b, rows[b], want)


@pytest.mark.parametrize("npts", [4, 50])
def test_dlt_matches_numpy(npts):
    rng = np.random.default_rng(70 + npts)
    x1 = np.stack([rng.uniform(0, 345, (24, npts)), rng.uniform(0, 259, (24, npts))], 2).astype(np.float32).astype(np.float64)
    Ht = [Hm.random_homography(rng) for _ in range(24)]
    x2 = np.stack([Hm.warp(h, p) for h, p in zip(Ht, x1)]) + (rng.normal(scale=0.5, size=x1.shape) if npts > 4 else 0.0)
    x2 = x2.astype(np.float32).astype(np.float64)
    H, ok = _nm.homography_dlt(_t(x1), _t(x2))
    H, ok = _np(H), _np(ok)
    worst = 0.0
    for i in range(24):
        ref = Hm.dlt(x1[i], x2[i])
        assert ok[i] == 1 and ref is not None
        worst = max(worst, np.linalg.norm(H[i] - ref) / np.linalg.norm(ref))
    print(f"measured: einx_homography_dlt, {npts} points: max rel diff {worst:.3e}")
    assert worst < 1e-6
    assert worst <= DLT_GATE[npts], worst
    same = np.repeat(x1[:1, :1], npts, 1)  # every point identical: no model
    _, ok = _nm.homography_dlt(_t(same), _t(same))
    assert _np(ok)[0] == 0


def test_orderings_and_columns(batch):
    pairs, _, out, _ = batch
    for cols, ordering in ((2, "yx"), (3, "xy"), (2, "xy")):
        got = _run(_stack(pairs, cols, ordering), ordering=ordering)
        for x, y in zip(got, out):
            assert np.array_equal(x, y, equal_nan=True), (cols, ordering)


def test_batch_alone_slot_repeat_and_graph(batch):
    pairs, args, out, _ = batch
    mk0, mk1, nm, shape, Ht = args
    for b in (9, 0, 14, 3):
        one = _run((mk0[b:b + 1], mk1[b:b + 1], nm[b:b + 1], shape[b:b + 1], Ht[b:b + 1]))
        for x, y in zip(one, out):
            assert np.array_equal(x[0], y[b], equal_nan=True), b
    perm = torch.arange(len(pairs) - 1, -1, -1, device=mk0.device)  # every pair at another slot
    moved = _run((mk0[perm].contiguous(), mk1[perm].contiguous(), nm[perm].contiguous(), shape, Ht[perm].contiguous()))
    for x, y in zip(moved, out):
        assert np.array_equal(x, y[::-1], equal_nan=True)
    again = _run(args)
    for x, y in zip(again, out):
        assert np.array_equal(x, y, equal_nan=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _nm.homography(*args)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = _nm.homography(*args)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(res, out):
        assert np.array_equal(_np(x), y, equal_nan=True)


def test_reference_api(batch, capsys):
    pairs, _, (H, mask, status, rows), _ = batch
    he = _mm.HomographyEstimation("HE", correctness_thresh=[3, 5, 10])
    keys = [f"HE@{k}_ratio" for k in (3, 5, 10)] + ["HE_errors", "HE_inliers"]
    for b in (9, 18, 16):  # a homography, fewer than 4 matches, no homography
        a0, a1, Ht = pairs[b]
        n = len(a0)
        d = he.update_one(Hm.IMG_SHAPE, _t(a0), _t(a1), torch.from_numpy(Ht))
        assert list(d) == keys
        printed = capsys.readouterr().out
        if b == 9:
            assert printed == ""
            assert isinstance(d["HE_errors"], np.ndarray) and d["HE_errors"].dtype == np.float32 and d["HE_errors"].shape == ()
            assert isinstance(d["HE@3_ratio"], np.ndarray) and d["HE@3_ratio"].dtype == np.float32
            assert isinstance(d["HE_inliers"], float)
            assert float(d["HE_errors"]) == rows[b, 3] and d["HE_inliers"] == rows[b, 4]
            assert [float(d[k]) for k in keys[:3]] == rows[b, :3].tolist()
            Hp, m = he.estimate_homography(_t(a0), _t(a1), ordering="yx")
            assert torch.is_tensor(Hp) and Hp.dtype == torch.float64 and Hp.shape == (3, 3) and Hp.device == he.to_device
            assert isinstance(m, np.ndarray) and m.shape == (n, 1) and m.dtype == np.uint8
            assert np.array_equal(_np(Hp), H[b]) and np.array_equal(m[:, 0].astype(bool), mask[b, :n])
        else:
            assert d["HE_errors"] == np.inf and d["HE_inliers"] == 0.0 and d["HE@3_ratio"] == 0.0
            assert ("Not enough points to estimate homography" if b == 18 else "Homography is None while trying to recover pose.") in printed
            assert he.estimate_homography(_t(a0), _t(a1)) == (None, None)
            capsys.readouterr()
    assert len(he.error_list) == 3 and he.error_list[1] == np.inf and he.error_list[0] == rows[9, 3]
    assert set(he.compute_all_auc()) == {"3", "5", "10"}
    sel = [9, 13, 18]
    out = he.update_batch([Hm.IMG_SHAPE] * 3, [_t(pairs[b][0]) for b in sel], [_t(pairs[b][1]) for b in sel],
                          [torch.from_numpy(pairs[b][2]) for b in sel])
    assert len(he.error_list) == 3
    assert list(out) == keys + [f"HE@{k}_auc" for k in (3, 5, 10)]
    assert out["HE_errors"] == np.inf  # update_batch's plain mean (:338-339) keeps the inf of the pair without a homography
    assert out["HE_inliers"] == np.mean([rows[9, 4], rows[13, 4], 0.0])
    auc = _mm.compute_auc([rows[9, 3], rows[13, 3], np.inf], [3, 5, 10])
    for k in (3, 5, 10):
        assert out[f"HE@{k}_auc"] == auc[str(k)]


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


def _plant(model, batches):
    """SP + MNN with synthetic weights finds one or two matches per pair, too few for any homography: after every real forward,
    overwrite the match result the evaluator reads (model._last_match: mk0 / mk1 / nmatch, in place) with the next planted batch
    of synthetic matches.  Returns the list that collects what was planted, one (mk0, mk1, nmatch) per forward."""
    real, seen = model._finish, []

    def finish(p):
        out = real(p)
        mr = model._last_match
        k0, k1, cnt = batches[len(seen) % len(batches)]
        mr.mk0.copy_(_t(k0))
        mr.mk1.copy_(_t(k1))
        mr.nmatch.copy_(_t(cnt))
        seen.append((mr.mk0.clone(), mr.mk1.clone(), cnt))
        return out

    model._finish = finish
    return seen


def test_harness_he_path():
    from helpers import synth_raw_events
    model = _model()
    H, W, B, cap = 100, 124, 3, 128
    rng = np.random.default_rng(8)
    spec = [[(100, 0.3, 0.2), (60, 0.5, 0.4), (3, 0.0, 0.0)], [(128, 0.0, 0.0), (80, 1.0, 0.5), (30, 0.5, 0.3)],
            [(40, 2.0, 0.3), (128, 0.5, 0.6), (0, 0.0, 0.0)]]  # (N, noise, outliers) per pair: two pairs with fewer than 4 matches
    batches, homs = [], []
    for row in spec:
        k0, k1, cnt, hom = np.zeros((B, cap, 3), np.float32), np.zeros((B, cap, 3), np.float32), np.zeros(B, np.int32), []
        for b, (n, nz, o) in enumerate(row):
            a0, a1, Ht = Hm.scene(rng, n, noise=nz, outliers=o, W=W, H=H, shift=8.0)
            k0[b, :n], k1[b, :n], cnt[b] = a0, a1, n
            hom.append(Ht)
        batches.append((k0, k1, cnt))
        homs.append(_t(np.stack(hom).astype(np.float32)))
    evs = [synth_raw_events(dict(seed=700 + b, n=6000, H=H, W=W, bins=5, frac=False, pneg=False)) for b in range(B)]
    img = synth.synth_image(60, B, H, W)
    plain = pkg.SameTimeEvaluator(model, bins=5, resolution=(W, H))
    rows_plain, _ = plain.step(evs, _t(img.copy()), homs[0])
    assert model._last_match.mk0.shape == (B, cap, 3)
    seen = _plant(model, batches)
    with_he = pkg.SameTimeEvaluator(model, bins=5, resolution=(W, H), he_thresh=(3, 5, 10))
    planted = pkg.SameTimeEvaluator(model, bins=5, resolution=(W, H))
    he = _mm.HomographyEstimation("HE", correctness_thresh=[3, 5, 10])
    per = []
    for k in range(3):  # a few synthetic batches with a known homography
        rows1, (ef, _, _) = with_he.step(evs, _t(img.copy()), homs[k])
        mk0, mk1, cnt = seen[-1]
        for b in range(B):
            per.append(he.update_one(ef["image_size"][b], mk0[b, :cnt[b]], mk1[b, :cnt[b]], homs[k][b]))
    seen.clear()
    for k in range(3):
        rows0, _ = planted.step(evs, _t(img.copy()), homs[k])
    assert torch.equal(rows0, rows1)  # the HE path leaves the other metrics' rows alone
    assert set(plain.result()) == set(plain.names) == set(planted.result())  # he_thresh=None: the keys of the parent commit
    res = with_he.result()
    keys = [f"HE@{k}_ratio" for k in (3, 5, 10)] + ["HE_errors", "HE_inliers"]
    assert set(res) == set(plain.names) | set(keys) | {f"HE@{t}_auc" for t in (3, 5, 10)}
    assert sum(np.isfinite(float(d["HE_errors"])) for d in per) == 7 and len(per) == 9
    for k in keys:  # the script's means (test_events-image_same-time.py:271-274): over the finite values
        v = np.array([float(d[k]) for d in per], np.float64)
        v = v[np.isfinite(v)]
        print(k, res[k], v.tolist())
        assert res[k] == np.mean(v), k
    assert 0.0 < res["HE@3_ratio"] < 1.0
    auc = he.compute_all_auc()
    for t in (3, 5, 10):
        assert res[f"HE@{t}_auc"] == auc[str(t)]
    for k in plain.names:
        assert res[k] == planted.result()[k] or (np.isnan(res[k]) and np.isnan(planted.result()[k]))
    # a step without a homography adds no HE row; run() carries the homography as the 3rd element of an item
    seen.clear()
    runner = pkg.SameTimeEvaluator(model, bins=5, resolution=(W, H), he_thresh=(3, 5, 10))
    got = list(runner.run([(evs, _t(img.copy()), homs[0]), (evs, _t(img.copy()))]))
    assert len(got) == 2 and len(runner._he_rows) == 1
    r2 = runner.result()
    for k in keys:
        v = np.array([float(d[k]) for d in per[:B]], np.float64)
        v = v[np.isfinite(v)]
        assert r2[k] == np.mean(v), k
