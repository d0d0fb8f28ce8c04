"""CPU tests of the evaluators' bookkeeping (harness.py): the running-mean accumulator against a literal restatement of the three
folds it replaced, result() assembled from hand-fed rows, `run`'s validation before anything is enqueued (`_validate` itself:
test_gt_matches_cpu.py), and a world_size-2 gloo run in which one rank has nothing to add to two of the three accumulators.  No
device and no library call: the evaluators are built with model=None."""
import datetime
import os
import sys
import time
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import ROOT, load_pkg
from test_pose_gloo import _free_port

pkg = load_pkg()
H = import_module(pkg.__name__ + ".harness")
NAMES = H.metric_names((1, 3), (1, 3))  # the evaluators' default thresholds


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return a == b or (a != a and b != b)


# ------------------------------------------------------------------------------------------ the accumulator
def _restated(batches, finite_only):
    """what the evaluators did before they shared one accumulator: every 64 batches concatenated, summed over the pairs and added
    to the running sums; `_fold` / `_fold_pr` skipped NaN (nan_to_num(rows).sum(0)), `_fold_losses` everything non-finite
    (where(isfinite, rows, 0).sum(0))"""
    sums = counts = None
    for i in range(0, len(batches), 64):
        rows = torch.cat(batches[i:i + 64], 0)
        if finite_only:
            ok = torch.isfinite(rows)
            s = torch.where(ok, rows, torch.zeros_like(rows)).sum(0)
        else:
            ok = ~torch.isnan(rows)
            s = torch.nan_to_num(rows).sum(0)
        c = ok.sum(0).double()
        sums, counts = (s, c) if sums is None else (sums + s, counts + c)
    return sums, counts


def _planted_batches():
    g = torch.Generator().manual_seed(1234)
    batches = [torch.randn(3, 4, dtype=torch.float64, generator=g) * 3.0 for _ in range(130)]  # folds at 64 and 128, 2 batches remain
    for b in batches:
        b[:, 3] = float("nan")  # a column without any value
    batches[0][1, 0] = float("nan")
    batches[70][2, 0] = -0.0
    batches[129][0, 0] = float("nan")
    batches[5][0, 1] = float("inf")  # one infinity per column: two of nan_to_num's largest floats would overflow the sum
    batches[100][2, 2] = float("-inf")
    batches[64][1, 2] = float("nan")
    return batches


@pytest.mark.parametrize("finite_only", [False, True])
def test_running_mean_equals_the_three_folds_it_replaced(finite_only):
    batches = _planted_batches()
    acc = H._RunningMean(4, finite_only=finite_only)
    for i, b in enumerate(batches):
        acc.add(b)
        assert len(acc.pending) == (i + 1) % 64  # lazy: nothing is reduced between the folds
    assert acc.counts[0] == 3 * 128 - 1  # folded at 64 and 128 batches; one NaN of column 0 is in the remainder
    s, c = acc.reduced("cpu")
    assert acc.pending == []
    es, ec = _restated(batches, finite_only)
    assert torch.equal(s, es) and torch.equal(c, ec) and torch.equal(_bits(s), _bits(es))
    assert ec.tolist() == [388.0, 389.0 if finite_only else 390.0, 388.0 if finite_only else 389.0, 0.0]
    for empty_is_nan, expect in ((False, es / ec.clamp_min(1)), (True, es / ec)):
        got = torch.tensor(H._RunningMean.means(s, c, empty_is_nan=empty_is_nan), dtype=torch.float64)
        assert torch.equal(_bits(got), _bits(expect))
    assert H._RunningMean.means(s, c)[3] == 0.0 and np.isnan(H._RunningMean.means(s, c, empty_is_nan=True)[3])
    if finite_only:
        assert abs(float(s[1])) < 1e4 and abs(float(s[2])) < 1e4
    else:  # the NaN-only rule counts an infinity as nan_to_num's largest float, which absorbs the rest of its column
        big = torch.finfo(torch.float64).max
        assert float(torch.nan_to_num(torch.tensor(float("inf"), dtype=torch.float64))) == big
        assert float(s[1]) == big and float(s[2]) == -big
    # reduced() hands out copies: adding more afterwards does not change what was returned
    acc.add(batches[1])
    acc.fold()
    assert torch.equal(s, es) and not torch.equal(acc.sums[:3], es[:3])


@pytest.mark.parametrize("finite_only", [False, True])
def test_running_mean_keeps_the_sign_of_a_zero_sum(finite_only):
    batches = [torch.tensor([[-0.0, float("nan")], [-0.0, -0.0]], dtype=torch.float64), torch.tensor([[-0.0, float("nan")]], dtype=torch.float64)]
    acc = H._RunningMean(2, finite_only=finite_only)
    for b in batches:
        acc.add(b)
    s, c = acc.reduced("cpu")
    es, ec = _restated(batches, finite_only)
    assert torch.equal(_bits(s), _bits(es)) and torch.equal(c, ec) and c.tolist() == [3.0, 1.0]


def test_running_mean_without_rows_reduces_zeros():
    s, c = H._RunningMean(3).reduced("cpu")
    assert s.dtype == c.dtype == torch.float64 and s.tolist() == c.tolist() == [0.0, 0.0, 0.0] and s is not c


# ------------------------------------------------------------------------------------------ result()
def _eighths(seed, shape, hi=64):
    """values k / 8: their float64 sums are exact in any order, so a mean formed by hand equals the accumulator's bit for bit"""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, hi, shape) / 8.0)


def _hand_mean(cols, skip, empty):
    out = []
    for col in cols.T:
        v = col[~skip(col)]
        out.append(float(v.sum() / len(v)) if len(v) else empty)
    return out


def _fed_same_time(he_thresh, losses):
    ev = pkg.SameTimeEvaluator(None, 5, he_thresh=he_thresh, losses=losses)
    metric = [_eighths(10 + i, (3, len(ev.names))) for i in range(3)]
    metric[1][0, 1] = float("nan")
    metric[2][:, 2] = float("nan")
    metric[0][:, 2] = metric[1][:, 2] = float("nan")  # a metric without any value: 0.0
    for rows in metric:
        ev._metric_mean.add(rows)
    return ev, torch.cat(metric, 0).numpy()


def test_result_assembles_metrics_he_and_losses():
    ev, metric = _fed_same_time((3, 5, 10), {})
    err = np.array([0.5, 4.0, np.inf, 7.25, 12.0, 2.0])
    he = np.stack([err <= 3, err <= 5, err <= 10, err, [0.9, 0.5, 0.0, 0.4, 0.2, 0.8]], 1).astype(np.float64)
    ev._he_rows += [torch.from_numpy(he[:4]), torch.from_numpy(he[4:])]
    loss = [_eighths(30 + i, (3, 3)) for i in range(2)]
    loss[0][1] = float("nan")
    loss[1][0, 0] = float("inf")
    loss[1][2, 1] = float("-inf")
    for rows in loss:
        ev._loss_mean.add(rows)
    res = ev.result()
    expect = dict(zip(NAMES, _hand_mean(metric, np.isnan, 0.0)))
    assert list(expect) == list(ev.names) and expect[ev.names[2]] == 0.0
    expect.update(H.he_summary(he, (3, 5, 10)))
    expect.update(zip(H.LOSS_NAMES, _hand_mean(torch.cat(loss, 0).numpy(), lambda v: ~np.isfinite(v), float("nan"))))
    assert set(res) == set(expect) and len(expect) == len(ev.names) + 8 + 3
    for k in expect:
        assert _same(res[k], expect[k]), (k, res[k], expect[k])
    assert res["HE_errors"] == np.mean(err[np.isfinite(err)]) and res["HE@3_ratio"] == 2 / 6
    # a loss without any finite value: NaN, the mean of nothing
    ev2, _ = _fed_same_time(None, {})
    ev2._loss_mean.add(torch.tensor([[1.5, float("nan"), float("nan")], [2.5, float("inf"), float("inf")]], dtype=torch.float64))
    r2 = ev2.result()
    assert r2["extractor_keypoints_loss"] == 2.0 and np.isnan(r2["extractor_descriptor_loss"]) and np.isnan(r2["loss"])
    assert set(r2) == set(ev2.names) | set(H.LOSS_NAMES)


def test_result_without_he_and_losses_has_the_metric_keys_only():
    for cls in (pkg.SameTimeEvaluator, pkg.DifferentTimeEvaluator):
        ev = cls(None, 5)
        rows = _eighths(3, (4, len(ev.names)))
        ev._metric_mean.add(rows)
        res = ev.result()
        assert list(res) == list(ev.names)
        assert list(res.values()) == _hand_mean(rows.numpy(), np.isnan, 0.0)
        assert torch.equal(ev.sums, rows.sum(0)) and torch.equal(ev.counts, torch.full((len(ev.names),), 4.0, dtype=torch.float64))


def test_result_before_the_first_batch_is_an_error():
    with pytest.raises(Exception):
        pkg.SameTimeEvaluator(None, 5).result()


# ------------------------------------------------------------------------------------------ validation
def test_run_validates_before_it_touches_the_model():
    """model=None: enqueueing anything would be an AttributeError"""
    item = ([], torch.zeros(1, 1, 8, 8), None, ("K0", "K1", "T"), ("d0", "d1"))
    with pytest.raises(ValueError, match="takes no depth"):
        list(pkg.SameTimeEvaluator(None, 5).run([item]))
    with pytest.raises(ValueError, match="pose"):
        list(pkg.DifferentTimeEvaluator(None, 5).run([item[:3] + (None, item[4])]))
    with pytest.raises(ValueError, match="pose"):
        pkg.DifferentTimeEvaluator(None, 5).step(item[0], item[1], depth=item[4])


# ------------------------------------------------------------------------------------------ process group
def _rank_rows(rank):
    """(metric rows, precision / recall rows, loss rows) of a rank; rank 1 has neither depth maps nor losses to account"""
    metric = _eighths(50 + rank, (5 if rank == 0 else 9, len(NAMES)))
    metric[1, 3] = float("nan")
    if rank == 1:
        return metric, None, None
    pr, loss = _eighths(60, (5, 4), hi=9), _eighths(61, (5, 3))
    pr[2] = float("nan")  # a pair without keypoints
    loss[3, 1] = float("inf")
    return metric, pr, loss


def _feed(evaluators, ranks):
    diff, same = evaluators
    for rank in ranks:
        metric, pr, loss = _rank_rows(rank)
        diff._metric_mean.add(metric)
        same._metric_mean.add(metric)
        if pr is not None:
            diff._pr_mean.add(pr)
            same._loss_mean.add(loss)
    return diff.result(), same.result()


def _evaluators():
    p = load_pkg()
    return p.DifferentTimeEvaluator(None, 5), p.SameTimeEvaluator(None, 5, losses={})


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    # a rank left alone in a collective fails after this long instead of waiting for ever
    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    torch.save(_feed(_evaluators(), [rank]), f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_means_all_reduce_world2_with_a_rank_that_adds_nothing(tmp_path):
    out = str(tmp_path / "means.pt")
    ctx = mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a rank hangs in a collective")
    single = _feed(_evaluators(), [0, 1])
    assert set(single[0]) == set(NAMES) | set(H.MATCH_PR_NAMES)
    assert set(single[1]) == set(NAMES) | set(H.LOSS_NAMES)
    for rank in (0, 1):
        got = torch.load(f"{out}.{rank}", weights_only=False)
        for g, s in zip(got, single):
            assert list(g) == list(s)
            for k in s:
                assert _same(g[k], s[k]), (rank, k, g[k], s[k])
