"""GPU tests (-m gpu), component: workspaces.  Nothing writes past what its *_ws_bytes query returned.

Most calls of the C ABI take a workspace and no size (einx_mnn*, einx_lightglue, einx_detect, einx_pair_metrics), so a size query
that drifted from the call's walk would be a silent device overrun.  Here every workspace the package allocates (they all come
from _native._workspace) gets GUARD bytes of a pattern behind it: the allocation is larger, so a stray write lands in the guard
and not outside the allocation, and after a synchronize every guard must still hold the pattern.  Each op runs once at B = 1 and
once as a small batch with ragged counts.  Whether the outputs are right is the rest of the suite's job."""
from importlib import import_module

import numpy as np
import pytest
import torch

from helpers import synth
from gpu_support import DEV, _bench_like_model, _lgcfg_model, _t, pkg

pytestmark = pytest.mark.gpu

GUARD = 4096
PATTERN = 0xA5
N = pkg.native
bt = import_module(pkg.__name__ + ".core.modules.matchers._batched")
nm = import_module(pkg.__name__ + ".core.metrics._native_metrics")
rep = import_module(pkg.__name__ + ".datasets.representations")


@pytest.fixture
def guards(monkeypatch):
    """[(nbytes, the guard behind a workspace of that size)] of every workspace allocated while the fixture is live"""
    made = []

    def guarded(nbytes, device):
        nbytes = int(nbytes)
        buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=device)
        buf[nbytes:] = PATTERN
        made.append((nbytes, buf[nbytes:]))
        return buf[:nbytes]

    monkeypatch.setattr(N, "_workspace", guarded)
    return made


def _intact(made, at_least):
    torch.cuda.synchronize()
    assert len(made) >= at_least, f"{len(made)} workspaces went through _native._workspace, expected at least {at_least}"
    for nbytes, tail in made:
        bad = int((tail != PATTERN).sum())
        assert bad == 0, f"{bad} of the {GUARD} guard bytes behind a workspace of {nbytes} bytes were overwritten"


def _forward(cfg_name, B, seed):
    _, model, _ = _bench_like_model(cfg_name, seed=seed)
    ev, mask = synth.synth_events(seed, B, 5)
    if B > 1:  # ragged counts: the event mask of the last pair keeps a corner only
        mask[-1, :, 40:, :] = False
        mask[-1, :, :, 60:] = False
    return model, _t(ev), _t(synth.synth_image(seed, B)), _t(mask)


def _ragged(B, cap, r):
    n = [int(r.integers(max(1, cap // 2), cap + 1)) for _ in range(B)]
    n[0] = cap
    if B > 1:
        n[-1] = max(1, cap // 7)
    return n


def _pair_batches(B, cap0, cap1, din, seed):
    r = np.random.default_rng(seed)
    H, W = 260, 346
    pbs = []
    for cap in (cap0, cap1):
        cnt = _ragged(B, cap, r)
        d = r.uniform(-1, 1, (B, cap, din)).astype(np.float32)
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        k = np.stack([r.uniform(0, H, (B, cap)), r.uniform(0, W, (B, cap)), r.uniform(0, 1, (B, cap))], 2).astype(np.float32)
        pb = bt.PairBatch()
        pb.kpts, pb.desc, pb.counts = _t(k), _t(d), _t(np.asarray(cnt, np.int32))
        pb.cap, pb.B, pb.image_size, pb.counts_host = cap, B, (H, W), None
        pbs.append(pb)
    return pbs


@pytest.mark.parametrize("B", [1, 3])
def test_sp_mnn_forward_with_and_without_log_assignment(guards, B):
    model, ev, img, mask = _forward("SP_MNN", B, seed=21)
    for want in (True, False):
        model.matcher.matcher.want_log_assignment = want
        model(ev, img.clone(), mask)
    _intact(guards, at_least=6)  # two extractors and the matcher, twice


@pytest.mark.parametrize("B,cap0,cap1", [(1, 1024, 1024), (3, 130, 70), (2, 37, 1000)])
def test_mnn_with_ratio_and_distance_thresholds(guards, B, cap0, cap1):
    p0, p1 = _pair_batches(B, cap0, cap1, 128, seed=5)
    for kw in (dict(ratio_thresh=0.9, distance_thresh=1.2), dict(ratio_thresh=0.9), dict(distance_thresh=1.2), dict()):
        for want_la in (True, False):
            N.mnn(p0.desc, p0.counts, p1.desc, p1.counts, want_la=want_la, **kw)
    N.mnn(p0.desc, p0.counts, p1.desc, p1.counts, want_la=False, gather=(p0.kpts, p1.kpts, 3))
    _intact(guards, at_least=9)


@pytest.mark.parametrize("B", [1, 3])
def test_sp_lightglue_forward_equal_caps(guards, B):
    """equal capacities: the two sides stacked in one [2B, cap, width] array per buffer"""
    model, ev, img, mask = _forward("SP_LG", B, seed=22)
    model(ev, img.clone(), mask)
    _intact(guards, at_least=3)


@pytest.mark.parametrize("B,cap0,cap1", [(1, 100, 300), (3, 1024, 640), (2, 70, 200), (3, 130, 130), (1, 37, 37)])
def test_lightglue_call_unequal_and_odd_caps(guards, B, cap0, cap1):
    conf = dict(input_dim=128, descriptor_dim=192, num_heads=3, n_layers=2)
    lg, _ = _lgcfg_model(dict(conf, wseed=700))
    p0, p1 = _pair_batches(B, cap0, cap1, conf["input_dim"], seed=6)
    lg.match_batched(p0, p1)
    _intact(guards, at_least=1)


@pytest.mark.parametrize("B", [1, 3])
def test_silk_forward(guards, B):
    model, ev, img, mask = _forward("SiLK_MNN", B, seed=23)
    model(ev, img.clone(), mask)
    _intact(guards, at_least=3)


@pytest.mark.parametrize("counts", [[20000], [3000, 0, 777], [0, 0]])
def test_voxel_grid_and_events_mask(guards, counts):
    H, W = 260, 346
    evs = []
    for i, n in enumerate(counts):
        r = np.random.default_rng(30 + i)
        evs.append({"x": r.uniform(0, W - 1, n).astype(np.float32), "y": r.uniform(0, H - 1, n).astype(np.float32),
                    "t": 1.5e9 + np.sort(r.uniform(0, 1, n)), "p": r.integers(0, 2, n).astype(np.float32)})
    for normalize in (True, False):
        rep.events_to_voxel_grid_batch(evs, (5, H, W), normalize=normalize, device=DEV)
    rep.events_mask_batch(evs, (W, H), device=DEV)
    rep.events_to_voxel_grid_batch(evs, (3, 97, 131), normalize=True, device=DEV)
    rep.events_mask_batch(evs, (131, 97), device=DEV)
    _intact(guards, at_least=5)


@pytest.mark.parametrize("B", [1, 3])
def test_batch_metrics(guards, B):
    model, ev, img, mask = _forward("SP_MNN", B, seed=24)
    evb, imb, mr = model.forward_batched(ev, img.clone(), mask)
    nm.batch_metrics(evb, imb, mr)
    _intact(guards, at_least=4)


@pytest.mark.parametrize("B,cap", [(1, 1024), (4, 300), (3, 37)])
def test_relative_pose_and_homography(guards, B, cap):
    r = np.random.default_rng(40 + B)
    mk0 = np.stack([r.uniform(0, 260, (B, cap)), r.uniform(0, 346, (B, cap)), r.uniform(0, 1, (B, cap))], 2).astype(np.float32)
    mk1 = mk0 + r.normal(0, 2.0, mk0.shape).astype(np.float32)
    nmatch = np.asarray(_ragged(B, cap, r), np.int32)
    if B > 1:
        nmatch[1] = 0
    K = np.tile(np.array([[300.0, 0, 173], [0, 300.0, 130], [0, 0, 1]]), (B, 1, 1))
    nm.relative_pose(_t(mk0), _t(mk1), _t(nmatch), _t(K), _t(K))
    nm.homography(_t(mk0), _t(mk1), _t(nmatch))
    _intact(guards, at_least=2)


def test_guard_sees_a_write_past_a_short_workspace(monkeypatch):
    """The check's own check.  A matcher workspace handed out 256 bytes short of the query still lies inside its allocation, and
    the last region (the second-neighbour column keys, zeroed by a memset when a ratio threshold is set) then reaches 256 bytes
    into the guard: exactly those must have lost the pattern."""
    made = []

    def short(nbytes, device):
        nbytes = int(nbytes) - 256
        buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=device)
        buf[nbytes:] = PATTERN
        made.append(buf[nbytes:])
        return buf[:nbytes]

    monkeypatch.setattr(N, "_workspace", short)
    p0, p1 = _pair_batches(1, 64, 64, 128, seed=7)  # 64 column keys of 4 bytes: the last region is 256 bytes
    N.mnn(p0.desc, p0.counts, p1.desc, p1.counts, want_la=False, ratio_thresh=0.9)
    torch.cuda.synchronize()
    assert len(made) == 1
    assert int((made[0][:256] != PATTERN).sum()) == 256 and int((made[0][256:] != PATTERN).sum()) == 0
