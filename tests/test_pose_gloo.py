"""world_size-2 gloo run of DifferentTimeEvaluator's pose gather: per-pair pose rows of different counts per rank go through
harness.gather_pose_rows, and the AUC of the union equals the single-process one (an AUC cannot be all-reduced from sums)."""
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
    if rank == empty_rank:  # a rank that was given no poses still takes part in the gather
        return np.zeros((0, 4))
    rng = np.random.default_rng(100 + rank)
    n = 5 if rank == 0 else 9  # ragged: the gather pads to the largest count
    r = np.abs(rng.normal(scale=8.0, size=(n, 4)))
    r[:, 2] = np.maximum(r[:, 0], r[:, 1])
    r[:, 3] = rng.uniform(0, 1, n)
    r[1] = [np.inf, np.inf, np.inf, 0.0]  # a pair without a pose
    return r


def _worker(rank, world, port, out, empty_rank):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    pkg = load_pkg()
    from importlib import import_module
    harness = import_module(pkg.__name__ + ".harness")
    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
    rows = harness.gather_pose_rows(torch.from_numpy(_rows(rank, empty_rank)))
    res = harness.rpe_summary(rows, (5, 10, 20))
    if rank == 0:
        torch.save({"rows": rows, "res": res}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("empty_rank", [-1, 1])
def test_pose_rows_gather_world2(tmp_path, empty_rank):
    out = str(tmp_path / "rpe.pt")
    mp.spawn(_worker, args=(2, _free_port(), out, empty_rank), nprocs=2, join=True)
    got = torch.load(out, weights_only=False)
    union = np.concatenate([_rows(0, empty_rank), _rows(1, empty_rank)], 0)
    assert np.array_equal(got["rows"].numpy(), union)
    pkg = load_pkg()
    from importlib import import_module
    harness = import_module(pkg.__name__ + ".harness")
    mm = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
    single = harness.rpe_summary(torch.from_numpy(union), (5, 10, 20))
    auc = mm.compute_auc(list(union[:, 2]), [5, 10, 20])
    for t in (5, 10, 20):
        assert got["res"][f"RPE@{t}_auc"] == single[f"RPE@{t}_auc"] == auc[str(t)]
    assert got["res"] == single
