"""GPU tests (-m gpu), component: a recording on the device and its pair batches (datasets/recording.py).  A synthetic
recording at the geometry of test_pose_gpu.py::test_harness_pose_path (100 x 124): 8 depth frames, 12 images, a 40-knot pose
track, 20,000 events.  Every `pair_batches` item is compared with the same assembly made on the host from the arrays and the
float64 restatement (tests/poses_f64.py); then DifferentTimeEvaluator runs on the batches to the end."""
from importlib import import_module

import numpy as np
import pytest
import torch

import poses_f64 as P
from helpers import synth, synth_raw_events
from gpu_support import DEV, _np, pkg

pytestmark = pytest.mark.gpu

H, W = 100, 124
EVENTS_DT = 0.08
PAIRS = np.array([[0, 1], [1, 3], [2, 2], [5, 4], [7, 0], [3, 6], [6, 7]])
BATCH = 3
pairs_mod = import_module(pkg.__name__ + ".datasets.pairs")
poses = import_module(pkg.__name__ + ".datasets.poses")
recording_mod = import_module(pkg.__name__ + ".datasets.recording")


def _arrays():
    ev = synth_raw_events(dict(seed=700, n=20000, H=H, W=W, bins=5, frac=False, pneg=False))
    t0 = ev["t"][0]
    assert 0.9 < ev["t"][-1] - t0 < 1.2
    image_ts = t0 + 0.10 + 0.07 * np.arange(12)
    depth_ts = t0 + 0.12 + 0.09 * np.arange(8)
    images = np.clip(np.rint(synth.synth_image(70, 12, H, W)[:, 0]), 0, 255).astype(np.uint8)
    rng = np.random.default_rng(71)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.stack([3.0 + np.sin(xx / 17.0 + k) + 0.5 * np.cos(yy / 11.0 - k) for k in range(8)]).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.1] = np.nan  # holes as they come
    stamps = t0 - 0.01 + 0.027 * np.arange(40)
    assert stamps[-1] > depth_ts[-1]
    trans = np.cumsum(rng.normal(size=(40, 3)) * 0.01, 0)
    R, cur = np.empty((40, 3, 3)), np.eye(3)
    for n in range(40):
        cur = cur @ P.rotvec_matrix(rng.normal(size=3) * 0.004)
        R[n] = cur
    K = np.array([[60.0, 0, W / 2], [0, 61.0, H / 2], [0, 0, 1]], np.float32)
    return dict(events=ev, images=images, image_ts=image_ts, depth=depth, depth_ts=depth_ts, K=K), (stamps, trans, R)


@pytest.fixture(scope="module")
def recording():
    arrays, (stamps, trans, R) = _arrays()
    track = poses.PoseTrack(stamps, trans, R, device=DEV)
    rec = recording_mod.Recording(poses=track, device=DEV, **arrays)
    return rec, arrays, (stamps, trans, P.knots(R))


def _bound(T):
    return 2.0 ** -23 * np.maximum(1.0, np.abs(T[:, :3, 3]).max(1))


def test_pairing_and_poses_at_depth(recording):
    rec, a, (stamps, trans, quats) = recording
    idx = P.nearest_index_dense(a["image_ts"], a["depth_ts"])
    assert rec.image_index.dtype == torch.int64 and np.array_equal(_np(rec.image_index), idx)
    assert np.array_equal(rec.paired_image_ts, a["image_ts"][idx]) and len(set(idx.tolist())) > 4 and len(rec) == 8
    got = rec.poses_at_depth()
    assert got is rec.poses_at_depth() and got.dtype == torch.float32 and got.shape == (8, 4, 4)
    want = P.interpolate(stamps, trans, quats, a["depth_ts"])[0].astype(np.float32)
    assert (np.abs(_np(got).astype(np.float64) - want).max((1, 2)) <= _bound(want)).all()
    # tensors that already lie on the device are used as they are
    again = recording_mod.Recording(rec.events, rec.images, a["image_ts"], rec.depth, a["depth_ts"], rec.poses, a["K"], device=DEV)
    assert again.images.data_ptr() == rec.images.data_ptr() and again.depth.data_ptr() == rec.depth.data_ptr() and again.events is rec.events


def test_pair_batches_against_the_host_assembly(recording):
    rec, a, (stamps, trans, quats) = recording
    ev_t = a["events"]["t"]
    idx = P.nearest_index_dense(a["image_ts"], a["depth_ts"])
    T01, _, bad = P.relative(stamps, trans, quats, a["depth_ts"][PAIRS[:, 0]], a["depth_ts"][PAIRS[:, 1]])
    assert bad == 0
    T01 = T01.astype(np.float32)
    items = list(rec.pair_batches(PAIRS, batch=BATCH, events_dt=EVENTS_DT))
    assert [len(it[0]) for it in items] == [3, 3, 1]
    worst = 0.0
    for k, (win, img, hom, (K0, K1, T), (d0, d1)) in enumerate(items):
        p = PAIRS[k * BATCH:(k + 1) * BATCH]
        ts = a["image_ts"][idx[p[:, 0]]]
        assert win.sequence is rec.events and hom is None
        assert np.array_equal(win.begin, np.searchsorted(ev_t, ts - EVENTS_DT, side="left"))
        assert np.array_equal(win.end, np.searchsorted(ev_t, ts, side="right")) and (win.counts > 500).all()
        assert img.dtype == torch.float32 and img.shape == (len(p), 1, H, W)
        assert np.array_equal(_np(img)[:, 0], a["images"][idx[p[:, 1]]].astype(np.float32))
        for got, i in ((d0, p[:, 0]), (d1, p[:, 1])):
            assert got.dtype == torch.float32 and np.array_equal(_np(got).view(np.uint32), a["depth"][i].view(np.uint32))
        for got in (K0, K1):
            assert got.is_contiguous() and np.array_equal(_np(got), np.stack([a["K"]] * len(p)))
        want = T01[k * BATCH:(k + 1) * BATCH]
        d = np.abs(_np(T).astype(np.float64) - want).max((1, 2)) / _bound(want)
        worst = max(worst, float(d.max()))
        assert T.dtype == torch.float32 and (d <= 1.0).all()
    print(f"T_0to1 of {len(PAIRS)} pairs: worst difference {worst:.3f} of the bound")
    assert int(rec.poses.out_of_range) == 0
    assert list(rec.pair_batches(np.zeros((0, 2), np.int64))) == []
    for bad_pairs, exc in (([[0, 8]], IndexError), ([[-1, 2]], IndexError), ([0, 1, 2], ValueError), ([[0.5, 1.0]], ValueError)):
        with pytest.raises(exc):
            next(rec.pair_batches(bad_pairs))
    with pytest.raises(ValueError):
        next(rec.pair_batches(PAIRS, batch=0))


def _model():
    """the SP + MNN model on synthetic weights of test_pose_gpu.py"""
    cfg = pkg.default_config("SP_MNN", event_channels=5)
    for sec in (cfg.event_extractor.vgg, cfg.image_extractor.superpointv1):
        sec.detection_top_k = 128
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=33)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    return model


def test_evaluator_runs_on_the_pair_batches_to_the_end(recording):
    rec, _, _ = recording
    ev = pkg.DifferentTimeEvaluator(_model(), bins=5, resolution=(W, H))
    out = list(ev.run(rec.pair_batches(PAIRS, batch=BATCH, events_dt=EVENTS_DT)))
    assert [o[0].shape[0] for o in out] == [3, 3, 1] and ev.pairs == len(PAIRS)
    res = ev.result()
    for key in ("RPE_R_errs", "RPE_t_errs", "RPE_pose_errs", "RPE_inliers", "RPE@5_ratio", "RPE@10_auc", "RPE@20_auc"):
        assert key in res, key
    assert ev.last_gt is not None and len(ev._pose_rows) == 3 and sum(r.shape[0] for r in ev._pose_rows) == len(PAIRS)


def test_select_pairs_through_the_recording(recording):
    rec, a, _ = recording
    cand = np.array([[0, 1], [0, 2], [3, 3], [1, 4], [7, 6], [2, 5]])
    got = rec.select_pairs(cand, batch=4)
    want = pairs_mod.select_pairs(a["depth"], a["K"], rec.poses_at_depth(), cand, batch=4, device=DEV)
    assert sorted(got) == sorted(want) and len(got["candidates"]) == 5
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    with pytest.raises(IndexError):
        rec.select_pairs([[0, 9]])
