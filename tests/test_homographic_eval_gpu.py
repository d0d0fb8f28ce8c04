"""GPU tests (-m gpu), component: HomographicEvaluator (harness.py) on a small synthetic EIM at B = 2: under the
identity it is SameTimeEvaluator bit for bit; under a fixed homography its rows are those of the metric calls made by hand on
warp_perspective's output, `step` and `run(depth=2)` agree, the caller's images are untouched and the image network detects
nothing on an invalid pixel."""
from importlib import import_module

import numpy as np
import pytest
import torch

from helpers import synth, synth_raw_events
from gpu_support import DEV, _eim_model, _t, pkg

pytestmark = pytest.mark.gpu

warp = import_module(pkg.__name__ + ".datasets.warp")
hom = import_module(pkg.__name__ + ".core.geometry.homography")
harness = import_module(pkg.__name__ + ".harness")
M = import_module(pkg.__name__ + ".core.metrics._native_metrics")
H0, W0, B0 = 52, 70, 2
HE = (3, 5, 10)


def _same(a, b):
    return a == b or (a != a and b != b)


@pytest.fixture(scope="module")
def batches():
    """(an SP + MNN model, two batches of raw events and images at B0 x H0 x W0)"""
    _, model, _ = _eim_model("SP_MNN", seed=11)
    out = []
    for k in range(2):
        evs = [synth_raw_events(dict(seed=700 + 10 * k + b, n=2500, H=H0, W=W0, bins=5, frac=False, pneg=False)) for b in range(B0)]
        out.append((evs, synth.synth_image(80 + k, B0, H0, W0)))
    return model, out


def _zoom_out(B, shape, seed=3):
    """the inverse of a sampled homography: the source is a quadrilateral inside the destination, invalid pixels around it"""
    return np.linalg.inv(hom.sample_homographies(B, shape, rng=np.random.RandomState(seed), difficulty=0.4))


class _Sampler:
    """seeded, and remembers what it returned: the draws of a run are those of its batches in order"""

    def __init__(self, seed):
        self.rng, self.calls = np.random.RandomState(seed), []

    def __call__(self, B, shape):
        assert shape == (W0, H0)
        H = np.linalg.inv(hom.sample_homographies(B, shape, rng=self.rng, difficulty=0.4))
        self.calls.append(H)
        return H


def test_identity_sampler_is_the_same_time_evaluator(batches):
    model, data = batches
    eye = lambda B, shape: np.tile(np.eye(3), (B, 1, 1))  # noqa: E731
    hev = pkg.HomographicEvaluator(model, bins=5, resolution=(W0, H0), he_thresh=HE, sampler=eye)
    ste = pkg.SameTimeEvaluator(model, bins=5, resolution=(W0, H0), he_thresh=HE)
    for evs, img in data:
        rows_h, (ef_h, imf_h, m_h) = hev.step(evs, _t(img.copy()))
        rows_s, (ef_s, imf_s, m_s) = ste.step(evs, _t(img.copy()), torch.eye(3, device=DEV)[None].repeat(B0, 1, 1))
        assert bool(hev.last_warp[2].all())  # the identity: every pixel valid
        assert torch.equal(rows_h, rows_s)
        for b in range(B0):
            assert torch.equal(imf_h["sparse_positions"][b], imf_s["sparse_positions"][b])
            assert torch.equal(m_h["matches0"][b], m_s["matches0"][b])
    a, b = hev.result(), ste.result()
    assert list(b) == list(a)[:len(b)]
    for k in b:
        assert _same(a[k], b[k]), (k, a[k], b[k])
    assert set(a) - set(b) <= set(M.MATCH_PR_NAMES) | {"warp_valid_ratio"} and a["warp_valid_ratio"] == 1.0
    print({k: a[k] for k in a if k not in b})


def test_fixed_homography_rows_are_the_metric_calls_by_hand(batches):
    model, data = batches
    evs, img = data[0]
    H = _zoom_out(B0, (W0, H0))
    hev = pkg.HomographicEvaluator(model, bins=5, resolution=(W0, H0), he_thresh=HE, sampler=lambda B, shape: H)
    images = _t(img.copy())
    keep = images.clone()
    rows, (ef, imf, matches) = hev.step(evs, images)
    assert torch.equal(images, keep)  # not even SuperPoint's in-place scaling reached the caller's tensor
    H_used, _, valid = hev.last_warp
    share = valid.float().mean(dim=(1, 2, 3)).tolist()
    print("valid share", share, "image keypoints", [int(p.shape[0]) for p in imf["sparse_positions"]])
    assert all(0.2 < s < 0.98 for s in share)
    # no keypoint of the image side lies on an invalid pixel
    yx = imf._batched.ordering == "yx"
    for b in range(B0):
        pos = imf["sparse_positions"][b]
        assert pos.shape[0] > 0
        r, c = (pos[:, 0], pos[:, 1]) if yx else (pos[:, 1], pos[:, 0])
        assert bool(valid[b, 0, r.floor().long(), c.floor().long()].all()), b
    # by hand: the same warp, the model on it with the mask, the metric ops on its result
    rep, events_mask = hev.last_inputs
    warped, valid2 = warp.warp_perspective(_t(img.copy()), H)
    assert torch.equal(valid2, valid)
    ef2, imf2, _ = model(rep, warped, events_mask, valid2)
    Ht = torch.from_numpy(H).to(DEV, torch.float32)
    mr = model._last_match
    exp_rows = M.batch_metrics(ef2._batched, imf2._batched, mr, Ht, hev.mma_thr, hev.vdd_thr)
    assert torch.equal(torch.nan_to_num(rows, nan=-7.0), torch.nan_to_num(exp_rows, nan=-7.0))
    e, i = ef2._batched, imf2._batched
    gt = M.gt_matches(e.det.positions, i.det.positions, e.det.counts, i.det.counts, homography=Ht, pos_th=3, neg_th=6, ordering=e.ordering)
    assert torch.equal(gt["matches0"], hev.last_gt["matches0"]) and torch.equal(gt["matches1"], hev.last_gt["matches1"])
    positives = int((gt["matches0"] > -1).sum())
    print("positive labels", positives, "of", int(e.det.counts.sum()), "event keypoints")
    assert positives > 0  # the labels are not the empty ones an unrelated pair would give
    pr = M.match_pr(mr, gt["matches0"], e.det.counts)
    res = hev.result()
    assert set(res) == set(hev.names) | {k for k in res if k.startswith("HE")} | set(M.MATCH_PR_NAMES) | {"warp_valid_ratio"}
    assert len([k for k in res if k.startswith("HE")]) == 8
    for k, col in zip(M.MATCH_PR_NAMES, pr.T.tolist()):
        col = [v for v in col if v == v]
        assert res[k] == pytest.approx(sum(col) / len(col), rel=1e-12), k
    for k, col in zip(hev.names, exp_rows.T.tolist()):
        col = [v for v in col if v == v]
        assert res[k] == pytest.approx(sum(col) / max(len(col), 1), rel=1e-12), k
    assert res["warp_valid_ratio"] == pytest.approx(sum(share) / B0, rel=1e-6)
    print(res)


def test_step_and_run_agree_and_draw_in_batch_order(batches):
    model, data = batches
    s_step, s_run = _Sampler(21), _Sampler(21)
    stepped = pkg.HomographicEvaluator(model, bins=5, resolution=(W0, H0), he_thresh=HE, sampler=s_step)
    streamed = pkg.HomographicEvaluator(model, bins=5, resolution=(W0, H0), he_thresh=HE, sampler=s_run)
    by_step = [stepped.step(evs, _t(img.copy()))[0] for evs, img in data]
    by_run = [rows for rows, _ in streamed.run([(evs, _t(img.copy())) for evs, img in data], depth=2)]
    assert len(s_step.calls) == len(s_run.calls) == 2 and all(np.array_equal(a, b) for a, b in zip(s_step.calls, s_run.calls))
    assert not np.array_equal(s_step.calls[0], s_step.calls[1])
    for a, b in zip(by_step, by_run):
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
    a, b = stepped.result(), streamed.result()
    assert list(a) == list(b)
    for k in a:
        assert _same(a[k], b[k]), (k, a[k], b[k])
    with pytest.raises(ValueError, match="samples the pair's homography itself"):
        list(streamed.run([(data[0][0], _t(data[0][1].copy()), torch.eye(3, device=DEV))]))


def test_matcher_loss_needs_lightglue_and_reports_its_rows(batches):
    model, data = batches
    with pytest.raises(ValueError, match="needs a LightGlue matcher"):
        pkg.HomographicEvaluator(model, bins=5, resolution=(W0, H0), sampler=_Sampler(1), matcher_loss=True)
    with pytest.raises(ValueError, match="needs a LightGlue matcher"):  # as DifferentTimeEvaluator refuses it
        pkg.DifferentTimeEvaluator(model, bins=5, resolution=(W0, H0), matcher_loss=True)
    _, lg_model, _ = _eim_model("SP_LG", seed=11)
    hev = pkg.HomographicEvaluator(lg_model, bins=5, resolution=(W0, H0), sampler=_Sampler(5), matcher_loss=True)
    evs, img = data[0]
    _, (ef, imf, _) = hev.step(evs, _t(img.copy()))
    lg, gt = lg_model.matcher.matcher, hev.last_gt
    e, i = ef._batched, imf._batched
    rows = pkg.native.lg_assign_nll(lg._pack()[0], lg_model._last_match, None, gt["matches0"], gt["matches1"], pos0=gt["pos0"], n=e.det.counts,
                                    m=i.det.counts)
    exp = harness.matcher_loss_rows(rows, float(lg.conf.loss.nll_balancing))
    res = hev.result()
    print({k: res.get(k) for k in harness.MATCHER_LOSS_NAMES}, exp.tolist())
    fin = torch.isfinite(exp)
    assert bool(fin.all(1).any())  # some pair has keypoints on both sides
    for j, k in enumerate(harness.MATCHER_LOSS_NAMES):
        col = exp[:, j][fin[:, j]]
        assert res[k] == pytest.approx(float(col.mean()), rel=1e-12), k
