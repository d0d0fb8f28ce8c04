"""world_size-2 gloo run of SameTimeEvaluator's HE gather: per-pair homography rows (three ratios, error, inlier ratio) of
different counts per rank go through harness.gather_rows, and the summary of the union equals the single-process one (an AUC
cannot be all-reduced from sums)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import ROOT, load_pkg


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rows(rank, empty_rank=-1):
    if rank == empty_rank:  # a rank that was given no homography still takes part in the gather
        return np.zeros((0, 5))
    rng = np.random.default_rng(200 + rank)
    n = 5 if rank == 0 else 9  # ragged: the gather pads to the largest count
    err = np.abs(rng.normal(scale=4.0, size=n)).astype(np.float32).astype(np.float64)
    r = np.stack([err <= 3, err <= 5, err <= 10, err, rng.uniform(0, 1, n)], 1).astype(np.float64)
    r[1] = [0.0, 0.0, 0.0, np.inf, 0.0]  # a pair without a homography
    return r


def _worker(rank, world, port, out, empty_rank):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    pkg = load_pkg()
    from importlib import import_module
    harness = import_module(pkg.__name__ + ".harness")
    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
    rows = harness.gather_rows(torch.from_numpy(_rows(rank, empty_rank)))
    res = harness.he_summary(rows, (3, 5, 10))
    if rank == 0:
        torch.save({"rows": rows, "res": res}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("empty_rank", [-1, 1])
def test_he_rows_gather_world2(tmp_path, empty_rank):
    out = str(tmp_path / "he.pt")
    mp.spawn(_worker, args=(2, _free_port(), out, empty_rank), nprocs=2, join=True)
    got = torch.load(out, weights_only=False)
    union = np.concatenate([_rows(0, empty_rank), _rows(1, empty_rank)], 0)
    assert np.array_equal(got["rows"].numpy(), union)
    pkg = load_pkg()
    from importlib import import_module
    harness = import_module(pkg.__name__ + ".harness")
    mm = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
    single = harness.he_summary(torch.from_numpy(union), (3, 5, 10))
    auc = mm.compute_auc(list(union[:, 3]), [3, 5, 10])
    for t in (3, 5, 10):
        assert got["res"][f"HE@{t}_auc"] == single[f"HE@{t}_auc"] == auc[str(t)]
    assert np.isfinite(got["res"]["HE_errors"]) and got["res"]["HE_errors"] == np.mean(union[np.isfinite(union[:, 3]), 3])
    assert got["res"] == single
