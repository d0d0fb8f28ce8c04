"""GPU tests (-m gpu), component: DifferentTimeEvaluator(label_cc_th=).  A synthetic pair batch in which a
foreground plane at depth 1 stands before a background at depth 4 and the second camera has moved sideways: part of what view 0
sees of the background is behind the foreground in view 1 (and the other way round).  Without the cycle check those keypoints
count as visible; with it they do not, and the labels follow.

The two networks see unrelated synthetic inputs, so their keypoints correspond by chance only: at the evaluator's default
pos_th = 3 a run on an MI355X found 140 hidden keypoints and not one positive among them, which leaves nothing for the labels to
differ in.  The evaluators here label with gt_pos_th = 10 and gt_neg_th = 12 (the evaluator's own attributes), under which a
keypoint's projection usually has a mutual nearest neighbour within reach."""
from importlib import import_module

import numpy as np
import pytest
import torch

from gpu_support import DEV, _np, _t, pkg
from helpers import synth, synth_raw_events

pytestmark = pytest.mark.gpu
M = import_module(pkg.__name__ + ".core.metrics._native_metrics")
H, W, B, BINS = 260, 346, 2, 5
F_, TX = 256.0, 1.0 / 8     # parallax f t / z: 8 pixels on the background (z = 4), 32 on the foreground (z = 1)
FG0 = (100, 200)            # the foreground's columns in view 0; in view 1 it stands 32 pixels further right


@pytest.fixture(scope="module")
def batch():
    cfg = pkg.default_config("SP_MNN", event_channels=BINS)
    model = pkg.EIM(cfg, device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=31)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    evs = [synth_raw_events(dict(seed=810 + b, n=20000, H=H, W=W, bins=BINS, frac=False, pneg=False)) for b in range(B)]
    img = synth.synth_image(95, B, H, W)
    depth0, depth1 = np.full((B, H, W), 4.0, np.float32), np.full((B, H, W), 4.0, np.float32)
    depth0[:, :, FG0[0]:FG0[1]] = 1.0
    depth1[:, :, FG0[0] + 32:FG0[1] + 32] = 1.0
    K = np.tile(np.array([[F_, 0, W / 2], [0, F_, H / 2], [0, 0, 1]], np.float32), (B, 1, 1))
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, 0, 3] = TX
    return model, evs, img, (_t(K), _t(K), _t(T)), (_t(depth0), _t(depth1))  # the image as numpy: every step uploads its own copy


def _make(model, **kw):
    ev = pkg.DifferentTimeEvaluator(model, bins=BINS, resolution=(W, H), **kw)
    ev.gt_pos_th, ev.gt_neg_th = 10, 12
    return ev


def test_label_cc_th_hides_what_the_foreground_covers(batch):
    model, evs, img, pose, depth = batch
    plain, cc = _make(model), _make(model, label_cc_th=1.0)
    rows0, (ef, imf, _) = plain.step(evs, _t(img), None, pose=pose, depth=depth)
    rows1, _ = cc.step(evs, _t(img), None, pose=pose, depth=depth)
    assert _np(rows0).tobytes() == _np(rows1).tobytes()  # the returned rows do not depend on the labels
    a, b = plain.last_gt, cc.last_gt
    assert set(a) == set(b)
    kp0, kp1 = ef._batched.det.positions, imf._batched.det.positions
    n, m = ef._batched.det.counts, imf._batched.det.counts
    assert ef._batched.ordering == "yx"
    # stage A apart from the visibility is what it was
    for k in ("proj_0to1", "proj_1to0", "depth_keypoints0", "depth_keypoints1", "valid0", "valid1"):
        assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k
    hidden0, hidden1 = a["visible0"] & ~b["visible0"], a["visible1"] & ~b["visible1"]
    assert not (b["visible0"] & ~a["visible0"]).any() and not (b["visible1"] & ~a["visible1"]).any()  # the check only removes
    # the hidden keypoints are the background's whose projection lands on the other view's foreground, and no others; a pixel
    # either side of the foreground's edges the bilinear sample mixes both surfaces and is not judged here
    for hidden, vis, kp, d, proj, lo, hi in ((hidden0, a["visible0"], kp0, a["depth_keypoints0"], a["proj_0to1"], FG0[0] + 32, FG0[1] + 32),
                                             (hidden1, a["visible1"], kp1, a["depth_keypoints1"], a["proj_1to0"], FG0[0], FG0[1])):
        u = proj[..., 0]
        background = vis & (d > 3.9)  # a keypoint on its own map's edge between the surfaces samples something in between: not judged
        covered = background & (u > lo + 1) & (u < hi - 1)
        clear = (vis & (d < 1.1)) | (background & ((u < lo - 1) | (u > hi + 1)))
        assert covered.any() and hidden[covered].all() and not hidden[clear].any()
    # stage B decides the labels from those flags: what gt_label gives on them
    want = M.gt_label(kp0, kp1, n, m, b["proj_0to1"], b["proj_1to0"], b["visible0"], b["visible1"], b["valid0"], b["valid1"], pos_th=10, neg_th=12,
                      ordering="yx")
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "pos0"):
        assert torch.equal(b[k], want[k]), k
    # the labels changed, and only through a hidden keypoint.  A positive of two keypoints that both stay visible survives (hiding
    # other rows and columns cannot move an arg-min away from its minimum), so a lost or moved positive has a hidden end; a hidden
    # row keeps -1 and -2 and loses a positive; any other changed row went from -2 to a positive that a hidden keypoint had blocked
    for mine, other, m_plain, m_cc in ((hidden0, hidden1, a["matches0"], b["matches0"]), (hidden1, hidden0, a["matches1"], b["matches1"])):
        changed = m_plain != m_cc
        partner_hidden = torch.gather(other, 1, m_plain.clamp(min=0)) & (m_plain > -1)
        was_pos = mine & (m_plain > -1)
        print(f"hidden {int(mine.sum())}, of them positives {int(was_pos.sum())}, labels changed {int(changed.sum())}")
        assert changed.any() and was_pos.any()
        assert (mine | partner_hidden)[changed & (m_plain > -1)].all()
        assert (m_cc[was_pos] < 0).all() and torch.equal(m_cc[mine & (m_plain < 0)], m_plain[mine & (m_plain < 0)])
        rest = changed & ~mine & (m_plain < 0)
        assert (m_plain[rest] == -2).all() and (m_cc[rest] > -1).all()
    res = cc.result()
    for k in M.MATCH_PR_NAMES:
        assert k in res and k in plain.result()


def test_label_cc_th_none_changes_nothing(batch):
    model, evs, img, pose, depth = batch
    default, none = _make(model), _make(model, label_cc_th=None)
    r0, _ = default.step(evs, _t(img), None, pose=pose, depth=depth)
    r1, _ = none.step(evs, _t(img), None, pose=pose, depth=depth)
    assert _np(r0).tobytes() == _np(r1).tobytes()
    for k in default.last_gt:
        assert _np(default.last_gt[k]).tobytes() == _np(none.last_gt[k]).tobytes(), k
    a, b = default.result(), none.result()
    assert list(a) == list(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)
