"""Evaluation harnesses with the call patterns of the reference's test_events-image_same-time.py:130-283
 and test_events-image_different_time.py:187-264, entirely on the device:

    raw events --(events.hip)--> voxel grid + events mask
               --(EIM: conv/detect/desc/mnn|lightglue kernels)--> keypoints, descriptors, matches
               --(metrics.hip)--> MR, MMA@1/3, VDD@1/3 per pair  --> means (all-reduced across ranks)

               --(pose.hip, DifferentTimeEvaluator with poses)--> RANSAC relative pose, R / t / pose errors per pair
                  --> RPE means and AUC@t (per-pair errors all-gathered across ranks)

               --(homography.hip, evaluators built with he_thresh, steps given a homography)--> RANSAC homography, refit, LM
                  polish, mean corner error per pair --> HE means and AUC@t (per-pair rows all-gathered across ranks)

               --(gt_matches.hip, DifferentTimeEvaluator with poses and depth maps)--> ground-truth matches of the keypoints,
                  match_recall / match_precision / accuracy / average_precision per pair --> means (all-reduced across ranks)

               --(loss.hip, SameTimeEvaluator with losses)--> the two extractor losses per pair --> means (all-reduced across ranks)

    images --(warp.hip, HomographicEvaluator)--> the image under a sampled homography + its valid mask --> the image network;
               the same homography --> MMA / VDD / HE as above and (gt_matches.hip) ground-truth matches without depth

Every batch is a `_Batch`, whichever entry point it came through: `step` and `run` differ only in how they enqueue it
(`_enqueue_batch`), and finish it the same way (`_finish_batch`: the model's host side, `_account`, `_account_losses`).  What
ends as a mean (metrics, losses, precision / recall) goes through one `_RunningMean` each; what ends as an AUC keeps its rows
(`_he_rows`, `_pose_rows`, `_gathered_summary`).
"""
from collections import deque
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native as native
from .core.metrics._native_metrics import (MATCH_PR_NAMES, batch_absolute_pose, batch_gt_matches, batch_homography, batch_metrics,
                                            batch_metrics_pose, batch_relative_pose, gt_matches, match_pr, metric_names, pose_metric_names,
                                            refine_relative_pose)
from .datasets.representations import EventStage, build_representation, events_representation_batch


LOSS_NAMES = ("extractor_keypoints_loss", "extractor_descriptor_loss", "loss")  # val_extractor.py:167-172 (VAL_ prefix added there)


def _grouped():
    """a process group is up: `result()` takes part in its collectives"""
    return torch.distributed.is_available() and torch.distributed.is_initialized()


class _Batch(NamedTuple):
    """the arguments of `step`, and an item of `run` (a plain tuple of the first 2 to 5 of them, in this order)"""
    events_list: list
    images: torch.Tensor
    homography: Optional[torch.Tensor] = None
    pose: Optional[tuple] = None
    depth: Optional[tuple] = None
    image_mask: Optional[torch.Tensor] = None  # the image extractor's score mask (HomographicEvaluator: the warp's valid pixels)


class _RunningMean:
    """Column means of per-pair float64 rows [B,width] that stay on the device.  `add` only keeps the batch's rows: they are
    folded into sums and counts lazily, 64 batches at a time (concatenated, summed, added to the running sums) -- eight small
    reductions per batch on the forward's stream were a third of what the evaluation loop cost on top of the forward
    (profiles/r06_notes.md 3).  An entry is skipped when it is NaN, or with `finite_only` when it is not finite; an infinity that
    is not skipped counts as nan_to_num's largest float."""

    def __init__(self, width, finite_only=False):
        self.width, self.finite_only = width, finite_only
        self.pending, self.sums, self.counts = [], None, None

    def add(self, rows):
        self.pending.append(rows)
        if len(self.pending) >= 64:
            self.fold()

    def fold(self):
        if not self.pending:
            return
        rows = torch.cat(self.pending, 0)
        self.pending = []
        ok = torch.isfinite(rows) if self.finite_only else ~torch.isnan(rows)
        s, c = torch.where(ok, torch.nan_to_num(rows), 0.0).sum(0), ok.sum(0).double()
        self.sums = s if self.sums is None else self.sums + s
        self.counts = c if self.counts is None else self.counts + c

    def reduced(self, device):
        """(sums, counts) over every rank.  Nothing added here: zeros on `device`, so that this rank still takes part -- a rank
        that skipped the collective would leave the others waiting in it."""
        self.fold()
        if self.sums is None:
            s, c = (torch.zeros(self.width, dtype=torch.float64, device=device) for _ in range(2))
        else:
            s, c = self.sums.clone(), self.counts.clone()
        if _grouped():
            torch.distributed.all_reduce(s)
            torch.distributed.all_reduce(c)
        return s, c

    @staticmethod
    def means(sums, counts, empty_is_nan=False):
        """a column in which nothing was counted gives 0.0, or with `empty_is_nan` NaN, as the mean of nothing"""
        return (sums / (counts if empty_is_nan else counts.clamp_min(1))).tolist()


def kept_ratio_rows(live, n, m, cap0, cap1):
    """[B,1] float64 on the device: (live0 + live1) / (n + m) per pair from a MatchResult's `live` [2B] and the counts it was called
    with; NaN, which the means skip, for a pair with n + m == 0"""
    B = n.shape[0]
    total = (n.clamp(0, cap0) + m.clamp(0, cap1)).double()
    kept = (live[:B] + live[B:]).double()
    return torch.where(total > 0, kept / total.clamp_min(1.0), torch.full_like(total, float("nan")))[:, None]


class SameTimeEvaluator:
    def __init__(self, model, bins, resolution=(346, 260), mma_thr=(1, 3), vdd_thr=(1, 3), he_thresh=None, he_ransac_thresh=3.0,
                 he_conf=0.995, representation_type="VoxelGrid", losses=None):
        """model: EIM (eval mode); bins: the event network's in_channels; resolution: (W, H) like MVSECDataset.RESOLUTION.
        representation_type: the datasets' switch (MVSEC.py:706-718): "VoxelGrid", "TimeSurface", "EventStack" or
        "EventDistanceMap" -- what `step` and `run` build from the raw events on the device.
        he_thresh: HomographyEstimation's correctness thresholds (the script's [3, 5, 10]); None (default): no homography
        estimation, nothing is launched for it and result() has no HE key.  With thresholds, every batch whose `homography` is
        given also runs the RANSAC homography of its matches on the device (csrc/homography.hip; the script's
        HE.update_one, test_events-image_same-time.py:189-194) with no host synchronisation, and result() adds HE@t_ratio,
        HE_errors, HE_inliers and HE@t_auc (:269-277).
        losses: the dict of core.loss.build_losses (any mapping with `keypoints_loss` / `descriptors_loss`), None (default):
        nothing is launched for it and result() is unchanged.  With losses, every batch also enqueues the two extractor losses of
        the reference's stage-1 validation loop (val_extractor.py:154-163: keypoints_loss(events_feats, image_feats, events_mask,
        padder), descriptors_loss(events_feats, image_feats, events_mask)) on the device (csrc/loss.hip) with no
        host synchronisation, one value per pair as that loop forms them at its batch size of 1, and result() adds
        extractor_keypoints_loss, extractor_descriptor_loss and loss (their per-pair sum): each the mean over the pairs where it is
        finite (:183-186)."""
        self.losses = losses
        self._loss_mean = _RunningMean(len(LOSS_NAMES), finite_only=True)
        self.he_thresh = None if he_thresh is None else tuple(he_thresh)
        self.he_ransac_thresh, self.he_conf = float(he_ransac_thresh), float(he_conf)
        self._he_rows = []
        self._he_shapes = {}
        self.model = model
        self.bins = int(bins)
        build_representation(representation_type)  # an unknown name raises here, not in the first batch
        self.representation_type = representation_type
        self.resolution = tuple(int(v) for v in resolution)
        self.mma_thr, self.vdd_thr = tuple(mma_thr), tuple(vdd_thr)
        self.names = metric_names(self.mma_thr, self.vdd_thr)
        self._metric_mean = _RunningMean(len(self.names))
        self._stop_mean = _RunningMean(1)  # layers run per pair, when the matcher stops pairs early (LightGlue.early_stop)
        self._kept_mean = _RunningMean(1)  # (live0 + live1) / (n + m) per pair, when the matcher prunes points (LightGlue.point_pruning, 8j)
        self._stages = {}  # (slot, on its own stream, device) -> EventStage
        self.pairs = 0

    @torch.no_grad()
    def step(self, events_list, images, homography=None):
        """events_list: B dicts {"x","y","t","p"} of numpy arrays, or an EventWindows (datasets/sequence.py): B windows
        into a sequence whose events are on the device already -- nothing is packed or uploaded for the batch then, the results are
        those of the dicts `events_list.events_list()`.  images: [B,1,H,W] float (0..255) on the device
        (scaled in place by SuperPoint exactly like the reference).  Returns the per-pair metric rows [B,K] (device)."""
        return self._step(_Batch(events_list, images, homography))

    def _step(self, batch):
        self._validate(batch)
        return self._finish_batch(batch, *self._enqueue_batch(batch, 0, on_stage_stream=False))  # synchronous: its stage is free again

    def _validate(self, batch):
        """the same-time evaluation has no use for depth maps, so a batch that carries some is an error, not something to drop
        silently"""
        if batch.depth is not None:
            raise ValueError(f"einx: {type(self).__name__} takes no depth maps (DifferentTimeEvaluator does, together with pose=)")

    def _enqueue_batch(self, batch, slot, on_stage_stream):
        """Device side of one batch, nothing waits: raw events -> representation -> both networks and the matcher.  Returns what
        `_finish_batch` takes after the batch.
        on_stage_stream=False (`step`): the image network does not depend on the events, so it is enqueued FIRST and the host packs /
        uploads the raw events (38 MB, ~2.5 ms) under its ~4 ms of device work; the event network follows (round 6: 11.7 -> see
        profiles/r06_notes.md).
        on_stage_stream=True (`run`): upload AND representation kernels of batch i + 1 on the stage's own stream: they run beside
        batch i's convolutions (0.3 ms of memory- / latency-bound kernels per batch leave the main stream's chain).  (Every
        in-flight slot on a stream of its own, so that batch i's tail could overlap batch i + 1's head, measured the same: 8.89
        vs 8.84 ms per batch, profiles/r06_notes.md.)
        An EventWindows batch has nothing to pack or upload: the stage only lends its stream to `run`."""
        W, H = self.resolution
        dev = batch.images.device
        with torch.cuda.device(dev):
            stage = self._stages.get((slot, on_stage_stream, dev))
            if stage is None:  # page-locked upload path
                stage = self._stages[(slot, on_stage_stream, dev)] = EventStage(dev)
            im = None if on_stage_stream else self.model.enqueue_image(batch.images, batch.image_mask)
            rep, mask = events_representation_batch(batch.events_list, (self.bins, H, W), normalize=True, device=dev, stage=stage,
                                                    on_stage_stream=on_stage_stream, representation_type=self.representation_type)
            # what the extractors saw (deterministic since round 4: bit-equal run to run); in `run`: of the batch enqueued last
            # (results lag by up to depth - 1 batches)
            self.last_inputs = (rep, mask)
            return self.model._enqueue(rep, batch.images, mask, batch.image_mask, slot=slot, image_feats=im), mask

    def _finish_batch(self, batch, pending, events_mask):
        """Host side of one batch: wait for the model's counts, then enqueue everything that is evaluated on its result"""
        with torch.cuda.device(batch.images.device):
            ef, imf, matches = self.model._finish(pending)
        out = self._account(ef, imf, matches, batch)
        self._account_losses(ef, imf, events_mask)
        return out

    def _account_losses(self, ef, imf, events_mask):
        """[B,3] float64 rows (keypoints loss, descriptors loss, their sum) of the batch's pairs, kept on the device; an entry of
        `losses` that is missing or has no per-pair form (core.loss.Pass) gives NaN, which the means skip"""
        if self.losses is None:
            return
        from .core.modules.utils.util import Padder
        bf = ef._batched
        padder = Padder(tuple(bf.image_size), bf.cell)
        cols = []
        for key in ("keypoints_loss", "descriptors_loss"):
            pair_values = getattr(self.losses.get(key), "pair_values", None)
            if pair_values is None:
                cols.append(torch.full((bf.B,), float("nan"), dtype=torch.float64, device=bf.raw.device))
            else:
                cols.append(pair_values(ef, imf, events_mask, padder))
        self._loss_mean.add(torch.stack([cols[0], cols[1], cols[0] + cols[1]], 1))

    def _account(self, ef, imf, matches, batch):
        # the matcher's result is read from the model AFTER its _finish, which may have re-run the matcher (NMS retry)
        rows = batch_metrics(ef._batched, imf._batched, self.model._last_match, batch.homography, self.mma_thr, self.vdd_thr)
        self._metric_mean.add(rows)
        self.pairs += rows.shape[0]
        self._account_stop(self.model._last_match)
        self._account_kept(self.model._last_match, ef._batched, imf._batched)
        if self.he_thresh is not None and batch.homography is not None:
            mr = self.model._last_match
            key = (tuple(ef._batched.image_size), mr.mk0.shape[0], mr.mk0.device)
            shape = self._he_shapes.get(key)
            if shape is None:  # (H, W) of the forward for every pair, uploaded once
                shape = self._he_shapes[key] = torch.tensor([key[0]] * key[1], dtype=torch.int32, device=key[2])
            self._he_rows.append(batch_homography(mr, shape, batch.homography, self.he_ransac_thresh, self.he_conf, ordering=ef._batched.ordering,
                                                  he_thr=self.he_thresh)[3])
        return rows, (ef, imf, matches)

    def _account_stop(self, mr):
        stop = getattr(mr, "stop", None)
        if stop is not None:
            self._stop_mean.add(stop.double()[:, None])

    def _account_kept(self, mr, bf0, bf1):
        live = getattr(mr, "live", None)
        if live is not None:
            self._kept_mean.add(kept_ratio_rows(live, bf0.counts, bf1.counts, mr.kept0.shape[1], mr.kept1.shape[1]))

    @property
    def sums(self):
        self._metric_mean.fold()
        return self._metric_mean.sums

    @property
    def counts(self):
        self._metric_mean.fold()
        return self._metric_mean.counts

    @torch.no_grad()
    def run(self, batches, depth=2):
        """The evaluation LOOP (test_events-image_same-time.py:130-194 iterates a DataLoader): `batches` yields
        (events_list, images[, homography[, pose[, depth]]]) like the arguments of `step`; one `step` result per batch comes back, in order.
        Up to `depth` batches are in flight: batch i + 1's events are concatenated into page-locked memory, uploaded with
        non-blocking copies and its kernels enqueued (EIM.forward_stream's mechanism) BEFORE the host waits for batch i's
        counts, so packing and the PCIe transfer hide under the device's work instead of adding to it (an item whose first
        element is an EventWindows has neither).  Same kernels, same results as `step`; every `images` tensor must stay untouched until its result has been yielded."""
        depth = max(int(depth), 1)
        pending = deque()
        for k, item in enumerate(batches):
            batch = _Batch(*item)
            self._validate(batch)  # raises before anything of the batch is enqueued
            pending.append((batch, *self._enqueue_batch(batch, k % depth, on_stage_stream=True)))
            if len(pending) >= depth:
                yield self._finish_batch(*pending.popleft())
        while pending:
            yield self._finish_batch(*pending.popleft())

    def result(self):
        """Mean of every metric over the pairs seen so far; sums are all-reduced when a process group is up."""
        if self.sums is None:
            raise RuntimeError("einx: result() before the first batch")
        dev = self.sums.device
        out = dict(zip(self.names, _RunningMean.means(*self._metric_mean.reduced(dev))))
        if self.he_thresh is not None:
            out.update(_gathered_summary(self._he_rows, len(self.he_thresh) + 2, he_summary, self.he_thresh))
        if self.losses is not None:  # no finite value for a key: NaN
            out.update(zip(LOSS_NAMES, _RunningMean.means(*self._loss_mean.reduced(dev), empty_is_nan=True)))
        s, c = self._stop_mean.reduced(dev)
        if float(c.max()) > 0:  # some rank's matcher stopped pairs early: the mean number of layers a pair ran
            out["matcher_stop_layer"] = _RunningMean.means(s, c)[0]
        s, c = self._kept_mean.reduced(dev)
        if float(c.max()) > 0:  # some rank's matcher pruned points: the mean share of a pair's keypoints that survived
            out["matcher_kept_ratio"] = _RunningMean.means(s, c)[0]
        return out


def gather_rows(rows):
    """[P,K] per-pair rows of this rank (pose rows: K = 4, homography rows: K = thresholds + 2; the same K on every rank) -> the
    rows of every rank (concatenated in rank order).  An AUC cannot be all-reduced from sums: the rows are all-gathered, padded
    to the largest count (on the CPU under gloo)."""
    if not _grouped():
        return rows
    world = torch.distributed.get_world_size()
    dev = rows.device if torch.distributed.get_backend() == "nccl" else torch.device("cpu")
    rows = rows.to(dev, torch.float64)
    n = torch.tensor([rows.shape[0]], dtype=torch.int64, device=dev)
    counts = [torch.zeros_like(n) for _ in range(world)]
    torch.distributed.all_gather(counts, n)
    counts = [int(c) for c in counts]
    pad = torch.full((max(counts), rows.shape[1]), float("nan"), dtype=torch.float64, device=dev)
    pad[:rows.shape[0]] = rows
    parts = [torch.empty_like(pad) for _ in range(world)]
    torch.distributed.all_gather(parts, pad)
    return torch.cat([p[:c] for p, c in zip(parts, counts)], 0)


gather_pose_rows = gather_rows  # the name it had while the pose rows were its only user


def _gathered_summary(batches, width, summary, thresholds):
    """an estimator's keys of result(): its per-batch row tensors [P,width] concatenated, gathered over the ranks and summarised;
    {} when no rank has a row.  Every rank takes part in the gather, with zero rows if it ran no estimation: a rank that skipped
    the collective would leave the others waiting in it."""
    rows = gather_rows(torch.cat(batches, 0) if batches else torch.empty((0, width), dtype=torch.float64))
    return summary(rows, thresholds) if rows.shape[0] else {}


def _summary(cols, errors, thresholds, name):
    """per-pair columns {key: values} -> the mean of each key over its finite values, as the scripts form every key of their result
    dicts, plus AUC@t over the finite errors"""
    from .core.metrics.matching_metrics import compute_auc
    out = {k: np.mean(v[np.isfinite(v)]) for k, v in cols.items()}
    auc = compute_auc(list(errors), thresholds)
    for t in thresholds:
        out[f"{name}@{t}_auc"] = auc[f"{t}"]
    return out


def _rows_f64(rows, width):
    return np.asarray(rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows, dtype=np.float64).reshape(-1, width)


def he_summary(rows, he_thresh=(3, 5, 10), name="HE"):
    """the HE keys of test_events-image_same-time.py:269-277 from per-pair rows ((error <= t) per threshold, mean corner error,
    inlier ratio; 0.., inf, 0 for a pair without a homography): the mean of each key over its finite values, as the script forms
    every key of its result_dict, and AUC@t over the finite errors"""
    nt = len(he_thresh)
    r = _rows_f64(rows, nt + 2)
    cols = {f"{name}@{t}_ratio": r[:, i] for i, t in enumerate(he_thresh)}
    cols[f"{name}_errors"] = r[:, nt]
    cols[f"{name}_inliers"] = r[:, nt + 1]
    return _summary(cols, r[:, nt], he_thresh, name)


def rpe_summary(rows, pose_thresh=(5, 10, 20), name="RPE"):
    """rpe_dict of test_events-image_different_time.py:326-334 from per-pair rows (R_err, t_err, pose_err, inlier ratio; inf
    errors for a pair without a pose): the mean of each key over its finite values, AUC@t over the finite pose errors"""
    r = _rows_f64(rows, 4)
    ok = np.isfinite(r[:, 0])
    cols = {f"{name}_R_errs": r[:, 0], f"{name}_t_errs": r[:, 1], f"{name}_pose_errs": r[:, 2], f"{name}_inliers": r[:, 3]}
    for t in pose_thresh:
        cols[f"{name}@{t}_ratio"] = np.where(ok, (r[:, 2] <= t).astype(np.float32), 0.0)
    return _summary(cols, r[:, 2], pose_thresh, name)


def refined_summary(kept, _=None, name="RPE"):
    """RPE_refined_ratio from the per-pair kept column of refine_relative_pose (1 the refined pose, 0 the input pose came back, -1
    no pose): the share of the pairs with a pose whose refined pose was kept; NaN when no pair has a pose"""
    k = _rows_f64(kept, 1)[:, 0]
    posed = int(np.count_nonzero(k >= 0))
    return {f"{name}_refined_ratio": float(np.count_nonzero(k == 1)) / posed if posed else float("nan")}


def ape_summary(rows, thresholds, name="APE"):
    """the APE keys from per-pair rows of batch_absolute_pose (R_err, |t - t_gt|, t angle, inlier ratio, usable ratio; inf errors
    for a pair without a pose, which counts 0 under every threshold): the mean of each key over its finite values"""
    from .core.metrics.matching_metrics import AbsolutePoseEstimation
    return AbsolutePoseEstimation.summary(rows, thresholds, name)


MATCHER_LOSS_NAMES = ("matcher_loss", "matcher_nll_pos", "matcher_nll_neg", "matcher_row_norm")


def matcher_loss_rows(rows, balancing=0.5):
    """[B,8] rows of einx_lg_assign_nll -> [B,4] float64 = MATCHER_LOSS_NAMES per pair (losses["total"], nll_pos, nll_neg, row_norm
    of LightGlue.loss in eval mode); NaN rows for a pair without keypoints on a side.  Device arithmetic only."""
    vals, row_norm = native.lg_nll_values(rows, balancing)
    return torch.cat([vals[:, :3], row_norm[:, None]], 1)


class _MatcherLabels:
    """What an evaluator that labels its keypoints with ground-truth matches shares, whichever geometry the labels come from
    (DifferentTimeEvaluator: depth and motion; HomographicEvaluator: the homography it warped with): the matcher_metrics means
    and, with matcher_loss=True, the rows of LightGlue.loss."""

    def _init_labels(self, model, matcher_loss, pos_th, neg_th):
        self._pr_mean = _RunningMean(len(MATCH_PR_NAMES))  # of the [B,4] matcher_metrics rows (a pair without keypoints has NaN rows)
        self.gt_pos_th, self.gt_neg_th = pos_th, neg_th
        self.last_gt = None
        self.matcher_loss = bool(matcher_loss)
        if self.matcher_loss and not hasattr(getattr(model.matcher, "matcher", None), "log_assignment"):
            raise ValueError("einx: matcher_loss=True needs a LightGlue matcher: the loss is that of its assignment head (an MNN "
                             "matcher has no parameters and no loss in the validation loop)")
        self._nll_mean = _RunningMean(len(MATCHER_LOSS_NAMES), finite_only=True)  # of the [B,4] rows of matcher_loss_rows

    def _validate_labels(self):
        if getattr(self, "matcher_loss", False) and self.model.matcher.matcher.early_stop_active():
            raise ValueError("einx: matcher_loss=True with early stopping on: the loss applies the LAST assignment head, the forward's "
                             "descriptors are those of each pair's stopping layer (LightGlue.loss refuses them too, DESIGN.md 8h)")
        if getattr(self, "matcher_loss", False) and self.model.matcher.matcher.point_pruning_active():
            raise ValueError("einx: matcher_loss=True with point pruning on: the forward's descriptors hold only the surviving rows, "
                             "the labels are those of every keypoint (LightGlue.loss refuses them too, DESIGN.md 8j)")

    def _account_labels(self, gt, ef, imf):
        self.last_gt = gt
        self._pr_mean.add(match_pr(self.model._last_match, gt["matches0"], ef._batched.det.counts))
        if self.matcher_loss:  # val_matcher.py:84,100: model.matcher.matcher.loss(matches, gt), VAL_loss = losses["total"].mean()
            lg = self.model.matcher.matcher
            rows = native.lg_assign_nll(lg._pack()[0], self.model._last_match, None, gt["matches0"], gt["matches1"], pos0=gt["pos0"],
                                        n=ef._batched.det.counts, m=imf._batched.det.counts)
            self._nll_mean.add(matcher_loss_rows(rows, float(lg.conf.loss.nll_balancing)))

    def _label_results(self, out):
        s, c = self._pr_mean.reduced(self.sums.device)
        if float(c.max()) > 0:  # some rank labelled a pair that has keypoints
            out.update(zip(MATCH_PR_NAMES, _RunningMean.means(s, c)))
        if self.matcher_loss:
            s, c = self._nll_mean.reduced(self.sums.device)
            if float(c.max()) > 0:  # some rank had a pair with keypoints on both sides
                out.update(zip(MATCHER_LOSS_NAMES, _RunningMean.means(s, c)))


class DifferentTimeEvaluator(_MatcherLabels, SameTimeEvaluator):
    """Call pattern of test_events-image_different_time.py:187-264: the events come from frame i, the image from a LATER
    frame j of the sequence, and the two views are related by a known motion instead of the identity.

    * `step(events_list, images, homography)`: as SameTimeEvaluator.step, with the image-0 -> image-1 homography [B,3,3]
      of the pair (planar scenes / pure rotations; None = identity) going into MMA@t and VDD@t (metrics.hip warps the
      keypoints exactly like core/metrics/util.py:warp_points).
    * `step(events_list, images, homography, pose=(K0, K1, T_0to1))`: with the intrinsics [B,3,3] and the ground-truth motion
      [B,4,4] of the pair on the device, the RANSAC relative pose of every pair runs on the device as well (csrc/pose.hip, what
      RelativePoseEstimation.update_one computes, :251-257), with no host synchronisation; the returned rows are unchanged.
      `run()` items may carry the same tuple as a 4th element.
    * `step(..., pose=(K0, K1, T_0to1), depth=(depth0, depth1))`: with the depth maps [B,H,W] of the two views as well, the
      ground-truth matches of the batch's keypoints (events = view 0, image = view 1; csrc/gt_matches.hip, DESIGN.md 8e: what
      val_matcher.py:66-97 computes with gt_matches_from_pose_depth) and the matcher's match_recall / match_precision / accuracy /
      average_precision against them (matcher_metrics) run on the device too, with no host synchronisation; the returned rows
      are unchanged, `last_gt` keeps the batch's label tensors.  `depth` without `pose` raises.  `run()` items may carry `depth`
      as a 5th element.
    * `matcher_loss=True` (LightGlue matchers; an MNN matcher raises at construction): every batch that carries pose and depth also
      enqueues the matcher's validation loss (val_matcher.py:84: LightGlue.loss in eval mode; einx_lg_assign_nll) on
      the forward's last-layer descriptors and the batch's labels, with no host synchronisation; result() adds matcher_loss (the
      mean of losses["total"]), matcher_nll_pos, matcher_nll_neg and matcher_row_norm over the pairs that have keypoints on both
      sides.  With the default nothing is launched and result() is unchanged.
    * `reproj_thr=(1, 3)` / `epi_thr=(1, 3)` / `occlusion_th=` (all None by default: nothing is launched, rows and
      result() are unchanged).  The inherited MMA@t / VDD_* warp view 0 with a homography (None: the identity), which a pair with
      parallax does not have.  With `reproj_thr`, a batch that carries pose and depth also measures them through the depth maps and
      the motion (einx_pair_metrics_pose): result() gains DT_MMA@t, DT_judged_ratio, DT_Repeatability@t, DT_ValidDistance@t and
      DT_Angle@t.  With `epi_thr`, a batch that carries pose gains EPI@t, the share of matches within t pixels of their epipolar
      lines (no depth needed).  One call serves both; each key is the mean over the pairs where it is finite and appears once some
      pair gave a finite value.  `occlusion_th` (pixels) drops keypoints and matches the other view's depth map says are hidden;
      without `reproj_thr` it raises.  The returned rows are unchanged.
    * `label_cc_th=` (pixels; None by default: nothing changes and nothing extra is launched).  The labels above call a keypoint
      visible when it projects in front of and inside the other camera, whatever stands in between.  With `label_cc_th` a batch
      with pose and depth is labelled through gt_matches_cc: the other view's depth map is sampled at the
      projection, the point is taken back, and it stays visible only when it returns within `label_cc_th` pixels of where it
      started (the reference's project(ccth=), here with label_cc_th^2 as the bound on the squared distance).  A hidden keypoint
      can then neither become a positive nor block one; match_*, average_precision and matcher_loss follow from those labels.
    * `abs_pose_thresh=((degrees, distance), ...)` (None by default: nothing is launched and result() is unchanged).  The relative
      pose above is a rotation and a translation direction.  With `abs_pose_thresh`, a batch that carries pose and depth also
      estimates the metric pose of the image camera in the event camera's frame from the matches and view 0's depth map
      (batch_absolute_pose: P3P RANSAC and an LM refit; `abs_pose_ransac_thresh` pixels, `abs_pose_conf`), with no
      host synchronisation; result() gains APE_R_errs (degrees), APE_t_errs (the depth map's unit), APE_t_angles, APE_inliers,
      APE_usable and APE@{deg}deg_{dist}_ratio per threshold (both errors within it; a pair without a pose counts 0).  A batch
      with pose but no depth contributes no row.
    * `pose_refine=True` (False by default: nothing extra is launched and result() is unchanged).  The relative pose above is that
      of one five-point sample, as OpenCV returns it.  With `pose_refine` it is then fitted to its inliers on the device
      (refine_relative_pose, DESIGN.md 8w: Levenberg-Marquardt on the Sampson distances, kept only when no inlier is lost), with no
      host synchronisation: the RPE_* keys are those of the refined poses, and result() gains RPE_refined_ratio, the share of the
      pairs with a pose whose refined pose was kept.
    * `result()`: the metric means, plus -- once poses were given -- the reference's rpe_dict keys (RPE_R_errs, RPE_t_errs,
      RPE_pose_errs, RPE_inliers, RPE@t_ratio, RPE@t_auc; :326-334).  Under a process group the per-pair pose rows are
      all-gathered before the AUC.  Once depth was given: the four matcher_metrics means over the pairs that have keypoints.
    * `pose_inputs(matches, b)`: what the reference feeds RelativePoseEstimation.update_one for pair b
      (`matches["matched_kpts0"][b]`, `matches["matched_kpts1"][b]`, :251-257), plus the (x, y) views of
      test_events-image_different_time.py:217-224 (`[..., :2]`, flipped when the extractor's ordering is "yx").
    """

    def __init__(self, model, bins, resolution=(346, 260), mma_thr=(1, 3), vdd_thr=(1, 3), pose_thresh=(5, 10, 20), ransac_thresh=1.0,
                 ransac_conf=0.999, he_thresh=None, he_ransac_thresh=3.0, he_conf=0.995, representation_type="VoxelGrid", losses=None,
                 matcher_loss=False, reproj_thr=None, epi_thr=None, occlusion_th=None, label_cc_th=None, abs_pose_thresh=None,
                 abs_pose_ransac_thresh=8.0, abs_pose_conf=0.99, pose_refine=False):
        if not isinstance(pose_refine, (bool, np.bool_)):
            raise ValueError(f"einx: pose_refine is True or False, not {pose_refine!r}")
        self.pose_refine = bool(pose_refine)
        self._pose_kept = []  # per batch [P,1] float64: refine_relative_pose's kept column (1 refined, 0 the input pose, -1 no pose)
        if label_cc_th is not None and not float(label_cc_th) > 0:
            raise ValueError("einx: label_cc_th is a distance in pixels (> 0), or None for labels without the occlusion check")
        self.label_cc_th = None if label_cc_th is None else float(label_cc_th)
        if occlusion_th is not None and reproj_thr is None:
            raise ValueError("einx: occlusion_th needs reproj_thr: the occlusion check belongs to the depth form of the metrics")
        for name, thr in (("reproj_thr", reproj_thr), ("epi_thr", epi_thr)):
            if thr is not None and not 1 <= len(tuple(thr)) <= 4:
                raise ValueError(f"einx: {name} takes 1 to 4 thresholds")
        if losses is not None:
            raise ValueError("einx: DifferentTimeEvaluator takes no losses: its two views are not aligned pixel by pixel, which is what "
                             "the extractor losses compare (SameTimeEvaluator does)")
        super().__init__(model, bins, resolution=resolution, mma_thr=mma_thr, vdd_thr=vdd_thr, he_thresh=he_thresh,
                         he_ransac_thresh=he_ransac_thresh, he_conf=he_conf, representation_type=representation_type)
        self.pose_thresh = tuple(pose_thresh)
        self.ransac_thresh, self.ransac_conf = float(ransac_thresh), float(ransac_conf)
        self._pose_rows = []
        self.abs_pose_thresh = None if abs_pose_thresh is None else tuple((float(a), float(d)) for a, d in abs_pose_thresh)
        self.abs_pose_ransac_thresh, self.abs_pose_conf = float(abs_pose_ransac_thresh), float(abs_pose_conf)
        self._abs_pose_rows = []
        self._init_labels(model, matcher_loss, 3, 5)  # gt_matches_from_pose_depth's defaults, as val_matcher.py calls it
        # the depth / motion form of the metrics: one row layout for every batch, NaN where a batch had no depth
        self.reproj_thr = None if reproj_thr is None else tuple(reproj_thr)
        self.epi_thr = None if epi_thr is None else tuple(epi_thr)
        self.occlusion_th = None if occlusion_th is None else float(occlusion_th)
        self.dt_names = pose_metric_names(self.reproj_thr or (), self.reproj_thr or (), self.epi_thr or ())[1:]  # without MR
        self._dt_mean = _RunningMean(len(self.dt_names), finite_only=True)

    @torch.no_grad()
    def step(self, events_list, images, homography=None, pose=None, depth=None):
        return self._step(_Batch(events_list, images, homography, pose, depth))

    def _validate(self, batch):
        self._validate_labels()
        if batch.depth is not None and batch.pose is None:
            raise ValueError("einx: depth=(depth0, depth1) needs pose=(K0, K1, T_0to1): ground-truth matches come from depth AND motion")

    def _account(self, ef, imf, matches, batch):
        out = super()._account(ef, imf, matches, batch)
        if batch.depth is not None:
            K0, K1, T = batch.pose
            cc = None if self.label_cc_th is None else self.label_cc_th ** 2  # pixels -> the bound on the squared cycle distance
            self._account_labels(batch_gt_matches(ef._batched, imf._batched, batch.depth[0], batch.depth[1], K0, K1, T, None, self.gt_pos_th,
                                                  self.gt_neg_th, cc_th=cc), ef, imf)
        if batch.pose is not None:
            K0, K1, T = batch.pose
            pose = batch_relative_pose(self.model._last_match, K0, K1, T, self.ransac_thresh, self.ransac_conf, ordering=ef._batched.ordering)
            if self.pose_refine:
                mr = self.model._last_match
                _, _, _, info, rows, _ = refine_relative_pose(mr.mk0, mr.mk1, mr.nmatch, K0, K1, pose[0], pose[1], pose[2], pose[3], T,
                                                              self.ransac_thresh, ef._batched.ordering)
                self._pose_rows.append(rows)
                self._pose_kept.append(info[:, :1].to(torch.float64))
            else:
                self._pose_rows.append(pose[4])
            if self.abs_pose_thresh is not None and batch.depth is not None:
                self._abs_pose_rows.append(batch_absolute_pose(self.model._last_match, K0, K1, depth0=batch.depth[0], T_0to1=T,
                                                               thresh=self.abs_pose_ransac_thresh, conf=self.abs_pose_conf,
                                                               ordering=ef._batched.ordering)[4])
            depth = batch.depth if self.reproj_thr is not None else None
            if depth is not None or self.epi_thr is not None:  # one call for the depth form and the EPI columns
                rows = batch_metrics_pose(ef._batched, imf._batched, self.model._last_match, K0, K1, T, depth, None, self.reproj_thr or (),
                                          self.reproj_thr or (), self.epi_thr or (), self.occlusion_th)
                self._dt_mean.add(rows[:, 1:])
        return out

    def result(self):
        out = super().result()
        out.update(_gathered_summary(self._pose_rows, 4, rpe_summary, self.pose_thresh))
        if self.pose_refine:
            out.update(_gathered_summary(self._pose_kept, 1, refined_summary, None))
        if self.abs_pose_thresh is not None:
            out.update(_gathered_summary(self._abs_pose_rows, 5, ape_summary, self.abs_pose_thresh))
        self._label_results(out)
        if self.reproj_thr is not None or self.epi_thr is not None:
            s, c = self._dt_mean.reduced(self.sums.device)
            means = _RunningMean.means(s, c)
            out.update({k: v for k, v, cnt in zip(self.dt_names, means, c.tolist()) if cnt > 0})  # once a pair gave a finite value
        return out

    def pose_inputs(self, matches, b=0):
        mk0, mk1 = matches["matched_kpts0"][b], matches["matched_kpts1"][b]
        xy0, xy1 = mk0[..., :2], mk1[..., :2]
        if self.model.event_extractor.extractor.ordering == "yx":
            xy0, xy1 = torch.flip(xy0, dims=[-1]), torch.flip(xy1, dims=[-1])
        return {"matched_kpts0": mk0, "matched_kpts1": mk1, "matched_xy0": xy0, "matched_xy1": xy1}


class HomographicEvaluator(_MatcherLabels, SameTimeEvaluator):
    """Same-time pairs whose image is warped by a sampled homography before the image network sees it: the
    protocol SuperPoint, SiLK and LightGlue are validated with.  The reference's same-time script passes the identity as every
    pair's homography, under which HE is a degenerate test (a matcher that does nothing to geometry scores well); a known
    non-identity homography makes MMA / VDD / HE meaningful and gives exact ground-truth matches for ANY recording, with no
    depth: the match_recall / match_precision / accuracy / average_precision rows and the matcher's validation loss that
    DifferentTimeEvaluator can only form from depth maps.  The events stay as they are (the representations truncate event
    coordinates: warping raw events is a different operation); the events are view 0, the warped image view 1.

    * `sampler(B, (W, H)) -> [B,3,3]`: the batch's homographies, source -> destination in the continuous pixel coordinates of
      `sparse_positions` (numpy or tensor, any float dtype), e.g. `lambda B, shape: sample_homographies(B, shape, rng=rng,
      difficulty=0.5)` with core.geometry.homography.sample_homographies.  It is the only host work a batch adds, and it is called
      once per batch in batch order by `step` and by `run` at every depth: a run is reproducible from the sampler's seed.
    * `step(events_list, images)` / `run` items `(events_list, images)`: the images are warped into a NEW tensor
      (datasets.warp.warp_perspective; the caller's tensor is not written, not even by SuperPoint's in-place scaling), the valid
      pixels become the image extractor's score mask (an extractor that takes none, SiLK, detects on the zeros outside too), and
      everything SameTimeEvaluator does runs under `homography=H`, HE included when `he_thresh` is set.  `last_warp` keeps
      (H, warped, valid) of the batch enqueued last.
    * labels: gt_matches(..., homography=H) on the forward's keypoints with `gt_pos_th` / `gt_neg_th` (gt_matches_from_homography's
      3 and 6); `last_gt` keeps them.  `matcher_loss=True`: as DifferentTimeEvaluator, with the same refusals (an MNN matcher at
      construction; early stopping or point pruning when a batch arrives).
    * `result()`: the parent's keys, MATCH_PR_NAMES once a pair had keypoints, MATCHER_LOSS_NAMES when asked for, and
      `warp_valid_ratio`, the mean share of a warped image's pixels that are valid.  Nothing is read back per batch."""

    def __init__(self, model, bins, resolution=(346, 260), mma_thr=(1, 3), vdd_thr=(1, 3), he_thresh=None, he_ransac_thresh=3.0,
                 he_conf=0.995, representation_type="VoxelGrid", losses=None, *, sampler, gt_pos_th=3, gt_neg_th=6, matcher_loss=False):
        if not callable(sampler):
            raise ValueError("einx: sampler must be a callable (B, (W, H)) -> [B,3,3] homographies")
        if losses is not None:
            raise ValueError("einx: HomographicEvaluator takes no losses: its two views are not aligned pixel by pixel, which is what "
                             "the extractor losses compare (SameTimeEvaluator does)")
        super().__init__(model, bins, resolution=resolution, mma_thr=mma_thr, vdd_thr=vdd_thr, he_thresh=he_thresh,
                         he_ransac_thresh=he_ransac_thresh, he_conf=he_conf, representation_type=representation_type)
        self.sampler = sampler
        self._init_labels(model, matcher_loss, gt_pos_th, gt_neg_th)
        self._valid_mean = _RunningMean(1)
        self.last_warp = None

    def _warped(self, batch):
        """the batch `step` / `run` were given -> the batch the parent evaluates: warped images, their homographies, the valid mask"""
        from .datasets.warp import warp_perspective
        if batch.homography is not None or batch.pose is not None or batch.depth is not None or batch.image_mask is not None:
            raise ValueError("einx: HomographicEvaluator takes (events_list, images) only: it samples the pair's homography itself")
        images = batch.images
        if not torch.is_tensor(images) or images.dim() != 4:
            raise ValueError("einx: images must be a [B,1,H,W] tensor on the device")
        B = int(images.shape[0])
        H = torch.as_tensor(self.sampler(B, self.resolution))
        if tuple(H.shape) != (B, 3, 3) or not H.is_floating_point():
            raise ValueError(f"einx: the sampler must return [{B}, 3, 3] float homographies, got {tuple(H.shape)} {H.dtype}")
        warped, valid = warp_perspective(images, H)
        self.last_warp = (H, warped, valid)
        self._valid_mean.add(valid.double().mean(dim=(1, 2, 3))[:, None])
        return _Batch(batch.events_list, warped, H.to(images.device, torch.float32), image_mask=valid)

    @torch.no_grad()
    def step(self, events_list, images):
        return self._step(self._warped(_Batch(events_list, images)))

    @torch.no_grad()
    def run(self, batches, depth=2):
        """SameTimeEvaluator.run on items `(events_list, images)`; a batch is sampled and warped when the loop reaches it, so the
        sampler's draws follow batch order at every depth"""
        yield from super().run((self._warped(_Batch(*item)) for item in batches), depth)

    def _validate(self, batch):
        super()._validate(batch)
        self._validate_labels()

    def _account(self, ef, imf, matches, batch):
        out = super()._account(ef, imf, matches, batch)
        ev, im = ef._batched, imf._batched
        self._account_labels(gt_matches(ev.det.positions, im.det.positions, ev.det.counts, im.det.counts, homography=batch.homography,
                                        pos_th=self.gt_pos_th, neg_th=self.gt_neg_th, ordering=ev.ordering), ef, imf)
        return out

    def result(self):
        out = super().result()
        self._label_results(out)
        out["warp_valid_ratio"] = _RunningMean.means(*self._valid_mean.reduced(self.sums.device))[0]
        return out
