"""LightGlue.loss in eval mode for ONE pair, restated in float64 numpy from its contract (the reference's
core/modules/matchers/lightglue.py:66-133, :751-769).  Not collected by pytest (no test_ prefix).  The log-assignment comes from
tests/lg_f64.py::log_assignment, whose float32 run is the peer implementation the bound is taken from.

Also the integer-built label recipes the tests and the fixture generator share (`labels`)."""
import numpy as np
import torch

import lg_f64

SUM_NAMES = ("S_pos", "num_pos", "S_neg0", "num_neg0", "S_neg1", "num_neg1", "row_sum", "n")
LOSS_KEYS = ("total", "last", "assignment_nll", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable", "row_norm")


def head_dict(sd, prefix):
    """the four tensors of one MatchAssignment head out of a numpy state dict"""
    return {k: sd[prefix + k] for k in ("final_proj.weight", "final_proj.bias", "matchability.weight", "matchability.bias")}


def log_assignment(x0, x1, head, dtype=torch.float64):
    """[n+1, m+1] numpy, float64 (or the float32 peer) on the given descriptors"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    with torch.no_grad():
        return lg_f64.log_assignment(t(x0), t(x1), head, "", dtype).numpy()


def sums(la, gt0, gt1, W):
    """the op's eight numbers (einx.h: einx_lg_assign_nll) from a log-assignment [n+1, m+1]: W [n, m] any 0/1 matrix"""
    la = np.asarray(la, np.float64)
    n, m = la.shape[0] - 1, la.shape[1] - 1
    if n == 0 or m == 0:
        return np.zeros(8)
    W = np.asarray(W, np.float64)
    neg0, neg1 = np.asarray(gt0) == -1, np.asarray(gt1) == -1
    return np.array([(W * la[:n, :m]).sum(), W.sum(), la[:n, m][neg0].sum(), neg0.sum(), la[n, :m][neg1].sum(), neg1.sum(),
                     np.exp(la[:n, :]).sum(), n], np.float64)


def values(rows, balancing=0.5):
    """{key: float64} of LOSS_KEYS from one row of `sums`; NaN everywhere for a pair without keypoints on a side"""
    s_pos, n_pos, s_n0, n_n0, s_n1, n_n1, row_sum, n = [float(v) for v in rows]
    if n == 0:
        return {k: float("nan") for k in LOSS_KEYS}
    num_pos = max(n_pos, 1.0)
    den = max(n_n0, 1.0) + max(n_n1, 1.0)
    nll_pos = -s_pos / num_pos
    nll_neg = -(s_n0 + s_n1) / den
    nll = balancing * nll_pos + (1 - balancing) * nll_neg
    return {"total": nll, "last": nll, "assignment_nll": nll, "nll_pos": nll_pos, "nll_neg": nll_neg, "num_matchable": num_pos,
            "num_unmatchable": den / 2.0, "row_norm": row_sum / n}


def loss(x0, x1, head, gt0, gt1, W, balancing=0.5, dtype=torch.float64):
    """one pair: (values dict, the eight sums, the log-assignment)"""
    la = log_assignment(x0, x1, head, dtype)
    rows = sums(la, gt0, gt1, W)
    return values(rows, balancing), rows, la


def scatter(pos0, m):
    """the dense 0/1 matrix [n, m] of pos0 (-1 = no positive in the row)"""
    W = np.zeros((len(pos0), m), np.uint8)
    rows = np.nonzero(np.asarray(pos0) >= 0)[0]
    W[rows, np.asarray(pos0)[rows]] = 1
    return W


KINDS = ("edges", "nopos", "ignore")


def labels(kind, n, m):
    """integer-built labels of one pair: gt0 [n], gt1 [m] int64 (a match index, -1 unmatched, -2 ignored) and pos0 [n] int32.
    'edges':  positives in two rows of three, among them -- where the pair is large enough -- columns 127 and 128 from rows 126 ..
              129, i.e. on both sides of the 128-wide tile edge along both axes, and the last row's in the last column (unless that
              is row 129); every fifth row is labelled -1 whether or not it has a positive (neg_th < pos_th makes such rows in the
              reference); the columns cycle through match / -1 / -2.
    'nopos':  no positive at all, rows and columns a mix of -1 and -2.
    'ignore': every label is -2: all eight sums but row_sum and n are zero."""
    i, j = np.arange(n), np.arange(m)
    if kind == "ignore":
        return np.full(n, -2, np.int64), np.full(m, -2, np.int64), np.full(n, -1, np.int32)
    if kind == "nopos":
        return np.where(i % 2 == 0, -1, -2).astype(np.int64), np.where(j % 3 == 0, -1, -2).astype(np.int64), np.full(n, -1, np.int32)
    assert kind == "edges", kind
    pos0 = np.where(i % 3 != 2, (i * 5 + 1) % m, -1).astype(np.int32)
    pos0[n - 1] = m - 1
    if n > 129 and m > 128:
        pos0[126], pos0[127], pos0[128], pos0[129] = 127, 128, 127, 128
    gt0 = np.where(pos0 >= 0, pos0, np.where(i % 2 == 0, -1, -2)).astype(np.int64)
    gt0[i % 5 == 0] = -1
    gt1 = np.where(j % 3 == 0, (j * 7) % n, np.where(j % 3 == 1, -1, -2)).astype(np.int64)
    return gt0, gt1, pos0


def dense_multi(n, m):
    """a 0/1 matrix that is no scatter of any pos0: several positives in a row, and empty rows"""
    i, j = np.arange(n)[:, None], np.arange(m)[None, :]
    return ((i * 3 + j * 7) % 11 == 0).astype(np.uint8)
