"""MatchingRatio / MeanMatchingAccuracy with the reference's class names and `update_one` signatures
(core/metrics/matching_metrics.py:30-51, :84-156), computed by csrc/metrics.hip.  RelativePoseEstimation
(:347-559) runs its RANSAC essential matrix and recoverPose on the device (csrc/pose.hip, DESIGN.md 8b: the
written algorithm, not bit parity with cv2).  HomographyEstimation (:188-345) runs its RANSAC homography, the refit and
the polish on the device as well (csrc/homography.hip, DESIGN.md 8c, on the same terms).  AbsolutePoseEstimation has no
counterpart in the reference: the metric pose from matches and view 0's depth (csrc/abs_pose.hip)."""
import numpy as np
import torch

from ._native_metrics import ABS_POSE_ROWS, HOMOGRAPHY_STATUS, POSE_STATUS, absolute_pose, homography, single_pair, relative_pose


class MatchingRatio:
    def __init__(self, name):
        self.metric_name = name

    def update_one(self, matched_keypoints1, matched_keypoints2, keypoints1, keypoints2):
        assert len(matched_keypoints1) == len(matched_keypoints2)
        r = single_pair(keypoints1, keypoints2, None, None, matched_keypoints1, matched_keypoints2, (1, 1), (1, 1), None, (), ())
        return {self.metric_name: r["MR"]}


class MeanMatchingAccuracy:
    def __init__(self, name, threshold=3, ordering="yx"):
        assert ordering in {"xy", "yx"}
        self.metric_name = name
        self._threshold = threshold
        self._ordering = ordering

    @torch.no_grad()
    def update_one(self, matched_keypoints, warped_matched_keypoints, true_homography):
        assert len(matched_keypoints) == len(warped_matched_keypoints)
        if matched_keypoints.numel() == 0 or warped_matched_keypoints.numel() == 0:
            return {self.metric_name: 0.0}
        r = single_pair(matched_keypoints[:0], warped_matched_keypoints[:0], None, None, matched_keypoints, warped_matched_keypoints,
                        (1, 1), (1, 1), true_homography, (self._threshold,), (), ordering=self._ordering)
        return {self.metric_name: r[f"MMA@{self._threshold}"]}


def compute_auc(errors, thresholds):
    """area under the recall-vs-error curve up to each threshold, normalised (matching_metrics.py:8-27);
    host-side bookkeeping over a list of per-pair errors, numpy like the reference."""
    import numpy as np
    errors = np.array(errors) if isinstance(errors, list) else errors
    errors = errors[np.isfinite(errors)].astype(np.float32)
    errors = np.sort(errors, kind="stable")
    recall = (np.arange(len(errors)) + 1) / len(errors)
    errors = np.r_[0.0, errors]
    recall = np.r_[0.0, recall]
    aucs = {}
    for thres in thresholds:
        last = np.searchsorted(errors, thres)
        rec = np.r_[recall[:last], recall[last - 1]]
        err = np.r_[errors[:last], thres]
        aucs[f"{thres}"] = float(np.sum((err[1:] - err[:-1]) * (rec[1:] + rec[:-1]) * 0.5) / thres)  # np.trapz
    return aucs


def _batch_of_one(matched_keypoints1, matched_keypoints2, to_device):
    """one pair's matches as the batch of one the device estimators take: (mk0, mk1 [1,N,cols] float32, nmatch [1] int32), on the
    keypoints' device when that is a GPU, else on to_device"""
    dev = matched_keypoints1.device if matched_keypoints1.is_cuda else to_device
    n, cols = matched_keypoints1.shape
    mk0 = matched_keypoints1.detach().to(dev, torch.float32).reshape(1, n, cols).contiguous()
    mk1 = matched_keypoints2.detach().to(dev, torch.float32).reshape(1, n, cols).contiguous()
    return mk0, mk1, torch.tensor([n], dtype=torch.int32, device=dev)


_MISSING = object()


class HomographyEstimation:
    """matching_metrics.py:188-345 with the reference's constructor, attributes and methods; estimate_homography runs
    csrc/homography.hip for the one pair (RANSAC over the 4-point DLT, refit on the inliers, LM polish: DESIGN.md 8c) and hands
    back a torch homography and a numpy mask like the reference does after cv2.findHomography."""

    def __init__(self, name, correctness_thresh=_MISSING, ordering="yx") -> None:
        if correctness_thresh is _MISSING:
            # `HomographyEstimation("HE")` is malformed in the reference too (a TypeError: the argument is required).  This build
            # raised NotImplementedError for every construction while the estimator was missing, and tests/test_pose_cpu.py:25-26 and
            # tests/test_boundary_gpu.py:40-41 pin that for this one call; every well-formed construction works.
            raise NotImplementedError(f"{type(self).__name__}: correctness_thresh (a list or tuple, e.g. [3, 5, 10]) is missing.  "
                                      "Note that the estimator behind this class is the device RANSAC of DESIGN.md 8c and not "
                                      "OpenCV's cv2.findHomography")
        self.metric_name = name
        self.to_device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
        assert type(correctness_thresh) in (list, tuple)
        self.correctness_thresh = correctness_thresh
        self.ordering = ordering
        self.error_list = []
        assert ordering in {"xy", "yx"}

    def estimate_homography(self, matched_keypoints1, matched_keypoints2, ordering="yx"):
        """(homography [3,3] float64 torch tensor on to_device, inlier mask [N,1] uint8 numpy) or (None, None), printing the
        reference's messages"""
        assert len(matched_keypoints1) == len(matched_keypoints2)
        assert matched_keypoints1.shape[1] in (2, 3)
        n = len(matched_keypoints1)
        if n < 4:
            print("Not enough points to estimate homography")
            return None, None
        H, mask, status, _ = homography(*_batch_of_one(matched_keypoints1, matched_keypoints2, self.to_device), ordering=ordering, he_thr=())
        st = int(status[0])
        if st < 0:
            assert HOMOGRAPHY_STATUS[st] == "noH"
            print("\nHomography is None while trying to recover pose.\n")
            return None, None
        return H[0].to(self.to_device), mask[0, :n].to(torch.uint8).cpu().numpy().reshape(n, 1)

    def compute_all_auc(self):
        return compute_auc(self.error_list, self.correctness_thresh)

    @torch.no_grad()
    def update_one(self, img_shape, matched_keypoints1, matched_keypoints2, true_homography):
        out_dict = {}
        pred_homography, inliers = self.estimate_homography(matched_keypoints1, matched_keypoints2, ordering=self.ordering)
        if pred_homography is None:
            errors = np.inf
            for i in range(len(self.correctness_thresh)):
                out_dict[f"{self.metric_name}@{self.correctness_thresh[i]}_ratio"] = 0.0
            out_dict[self.metric_name + "_errors"] = errors
            out_dict[self.metric_name + "_inliers"] = 0.0
            self.error_list.append(errors)
            return out_dict
        true_homography = true_homography.to(self.to_device).float()
        pred_homography = pred_homography.to(self.to_device).float()
        h, w = int(img_shape[0]), int(img_shape[1])  # a tuple, or the forward's feats["image_size"] entry
        corners = torch.tensor([[0, 0, 1], [w - 1, 0, 1], [0, h - 1, 1], [w - 1, h - 1, 1]], dtype=torch.float32, device=self.to_device)
        # the 4x3 by 3x3 products as explicit sums, left to right (what csrc/homography.hip's epilogue evaluates), not torch.mm,
        # whose accumulation order is the BLAS library's
        warp = lambda h: (corners[:, 0:1] * h[:, 0] + corners[:, 1:2] * h[:, 1]) + corners[:, 2:3] * h[:, 2]  # noqa: E731
        real_warped_corners = warp(true_homography)
        real_warped_corners = real_warped_corners[:, :2] / real_warped_corners[:, 2:]
        warped_corners = warp(pred_homography)
        warped_corners = warped_corners[:, :2] / warped_corners[:, 2:]
        d = real_warped_corners - warped_corners
        dist = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        mean_dist = (((dist[0] + dist[1]) + dist[2]) + dist[3]) / 4
        correctness = mean_dist <= torch.tensor(self.correctness_thresh, device=self.to_device, dtype=torch.float32)
        for i in range(len(self.correctness_thresh)):
            out_dict[f"{self.metric_name}@{self.correctness_thresh[i]}_ratio"] = correctness[i].float().cpu().numpy()
        out_dict[self.metric_name + "_errors"] = mean_dist.float().cpu().numpy()
        out_dict[self.metric_name + "_inliers"] = inliers.mean().item()
        self.error_list.append(mean_dist.float().item())
        return out_dict

    @torch.no_grad()
    def update_batch(self, img_shapes, matched_keypoints1, matched_keypoints2, true_homographies):
        out_dict = {}
        self.error_list = []
        assert len(matched_keypoints1) == len(matched_keypoints2) == len(true_homographies)
        for i in range(len(matched_keypoints1)):
            one_out_dict = self.update_one(img_shapes[i], matched_keypoints1[i], matched_keypoints2[i], true_homographies[i])
            for k, v in one_out_dict.items():
                out_dict.setdefault(k, []).append(v)
        auc = self.compute_all_auc()
        for k in out_dict.keys():
            out_dict[k] = np.array(out_dict[k]).mean()
        for k in self.correctness_thresh:
            out_dict[f"{self.metric_name}@{k}_auc"] = auc[f"{k}"]
        return out_dict


class RelativePoseEstimation:
    """matching_metrics.py:347-559 with the reference's constructor, attributes and methods; estimate_pose runs csrc/pose.hip
    for the one pair (RANSAC essential matrix, recoverPose's cheirality vote) and hands back numpy like cv2 does.  refine=True
    (not the reference's; off by default): the pose is then fitted to its inliers on the device and estimate_pose
    returns the refined pose and its mask."""

    def __init__(self, name, pose_thresh, ransac_thresh=1.0, ransac_conf=0.999, ordering="yx", refine=False) -> None:
        self.metric_name = name
        self.to_device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
        self.pose_thresh = pose_thresh
        self.ransac_thresh = ransac_thresh
        self.ransac_conf = ransac_conf
        self.ordering = ordering
        self.refine = bool(refine)
        self.error_list = []
        assert ordering in {"xy", "yx"}

    def estimate_pose(self, matched_keypoints1, matched_keypoints2, K0, K1, thresh, conf, ordering="yx"):
        """(R [3,3], t [3], inlier mask [N] bool) as numpy, or None (printing the reference's messages)"""
        assert len(matched_keypoints1) == len(matched_keypoints2)
        assert matched_keypoints1.shape[1] in (2, 3)
        if len(matched_keypoints1) < 5:
            print("Not enough points to estimate pose")
            return None
        mk0, mk1, nm = _batch_of_one(matched_keypoints1, matched_keypoints2, self.to_device)
        R, t, mask, status, _ = relative_pose(mk0, mk1, nm, torch.as_tensor(K0).to(mk0.device)[None], torch.as_tensor(K1).to(mk0.device)[None],
                                              None, thresh, conf, ordering, refine=self.refine)
        st = int(status[0])
        if POSE_STATUS.get(st) == "noE":
            print("\nE is None while trying to recover pose.\n")
        if st < 0:
            return None
        n = len(matched_keypoints1)
        return R[0].cpu().numpy(), t[0].cpu().numpy(), mask[0, :n].cpu().numpy()

    def relative_pose_error(self, T_0to1, R, t, ignore_gt_t_thr=0.0):
        T_0to1 = T_0to1.detach().cpu().numpy() if torch.is_tensor(T_0to1) else np.asarray(T_0to1)
        t_gt = T_0to1[:3, 3]
        n = np.linalg.norm(t) * np.linalg.norm(t_gt)
        t_err = np.rad2deg(np.arccos(np.clip(np.dot(t, t_gt) / n, -1.0, 1.0)))
        t_err = np.minimum(t_err, 180 - t_err)  # handle E ambiguity
        if not np.isfinite(np.linalg.norm(t_gt)):  # pure rotation is challenging
            t_err = 0.0
        R_gt = T_0to1[:3, :3]
        cos = (np.trace(np.dot(R.T, R_gt)) - 1) / 2
        cos = np.clip(cos, -1.0, 1.0)  # handle numercial errors
        R_err = np.rad2deg(np.abs(np.arccos(cos)))
        return t_err, R_err

    def compute_all_auc(self):
        return compute_auc(self.error_list, self.pose_thresh)

    def _fail(self, out_dict):
        out_dict[self.metric_name + "_R_errs"] = np.inf
        out_dict[self.metric_name + "_t_errs"] = np.inf
        out_dict[self.metric_name + "_pose_errs"] = np.inf
        out_dict[self.metric_name + "_inliers"] = 0.0
        for i in range(len(self.pose_thresh)):
            out_dict[f"{self.metric_name}@{self.pose_thresh[i]}_ratio"] = 0.0
        self.error_list.append(np.inf)
        return out_dict

    @torch.no_grad()
    def update_one(self, matched_keypoints1, matched_keypoints2, K0, K1, T_0to1):
        out_dict = {}
        ret = self.estimate_pose(matched_keypoints1, matched_keypoints2, K0, K1, thresh=self.ransac_thresh, conf=self.ransac_conf,
                                 ordering=self.ordering)
        if ret is None:
            return self._fail(out_dict)
        R, t, inliers = ret
        t_err, R_err = self.relative_pose_error(T_0to1, R, t, ignore_gt_t_thr=0.0)
        pose_err = np.max([R_err, t_err]) if np.isfinite(t_err) else R_err
        out_dict[self.metric_name + "_R_errs"] = R_err
        out_dict[self.metric_name + "_t_errs"] = t_err
        out_dict[self.metric_name + "_pose_errs"] = pose_err
        out_dict[self.metric_name + "_inliers"] = inliers.mean().item()
        for i in range(len(self.pose_thresh)):
            out_dict[f"{self.metric_name}@{self.pose_thresh[i]}_ratio"] = (pose_err <= self.pose_thresh[i]).astype(np.float32)
        self.error_list.append(pose_err)
        return out_dict

    @torch.no_grad()
    def update_batch(self, matched_keypoints1, matched_keypoints2, K0, K1, T_0to1):
        out_dict = {}
        self.error_list = []
        assert len(matched_keypoints1) == len(matched_keypoints2) == len(K0) == len(K1) == len(T_0to1)
        for i in range(len(matched_keypoints1)):
            one_out_dict = self.update_one(matched_keypoints1[i], matched_keypoints2[i], K0[i], K1[i], T_0to1[i])
            for k, v in one_out_dict.items():
                out_dict.setdefault(k, []).append(v)
        auc = self.compute_all_auc()
        for k in out_dict.keys():
            v = np.array(out_dict[k])
            v = v[np.isfinite(v)]
            out_dict[k] = np.mean(v)
        for k in self.pose_thresh:
            out_dict[f"{self.metric_name}@{k}_auc"] = auc[f"{k}"]
        return out_dict


class AbsolutePoseEstimation:
    """The metric pose of view 1 in view 0's frame from the matches and view 0's depth map (csrc/abs_pose.hip, DESIGN.md 8u: P3P
    RANSAC and an LM refit, a written algorithm and not OpenCV's solvePnPRansac), shaped like RelativePoseEstimation.  `thresholds`
    is a sequence of (degrees, distance) pairs: a pair of views passes one when its rotation error is within the degrees AND
    |t - t_gt| within the distance (the depth map's unit)."""

    def __init__(self, name, thresholds, ransac_thresh=8.0, ransac_conf=0.99, ordering="yx") -> None:
        assert ordering in {"xy", "yx"}
        self.metric_name = name
        self.to_device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
        self.thresholds = tuple((float(a), float(d)) for a, d in thresholds)
        self.ransac_thresh = ransac_thresh
        self.ransac_conf = ransac_conf
        self.ordering = ordering
        self.rows = []

    @staticmethod
    def threshold_key(name, deg, dist):
        return f"{name}@{deg:g}deg_{dist:g}_ratio"

    @staticmethod
    def columns(rows, thresholds, name):
        """per-pair rows [P,5] (R_err, |t - t_gt|, t angle, inlier ratio, usable ratio; inf errors for a pair without a pose) ->
        {key: per-pair values}; a pair without a pose counts 0 under every threshold"""
        r = np.asarray(rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows, dtype=np.float64).reshape(-1, 5)
        cols = {f"{name}_{k}": r[:, i] for i, k in enumerate(ABS_POSE_ROWS)}
        for deg, dist in thresholds:
            with np.errstate(invalid="ignore"):
                cols[AbsolutePoseEstimation.threshold_key(name, deg, dist)] = ((r[:, 0] <= deg) & (r[:, 1] <= dist)).astype(np.float64)
        return cols

    @staticmethod
    def summary(rows, thresholds, name="APE"):
        """the mean of every column over its finite values (NaN for a column without one)"""
        out = {}
        for k, v in AbsolutePoseEstimation.columns(rows, thresholds, name).items():
            v = v[np.isfinite(v)]
            out[k] = float(np.mean(v)) if len(v) else float("nan")
        return out

    @torch.no_grad()
    def estimate_rows(self, matched_keypoints1, matched_keypoints2, K0, K1, depth0, T_0to1):
        """the [5] float64 row of one pair (numpy)"""
        assert len(matched_keypoints1) == len(matched_keypoints2)
        assert matched_keypoints1.shape[1] in (2, 3)
        if len(matched_keypoints1) == 0:
            return np.array([np.inf, np.inf, np.inf, 0.0, np.nan])
        mk0, mk1, nm = _batch_of_one(matched_keypoints1, matched_keypoints2, self.to_device)
        dev = mk0.device
        one = lambda v: torch.as_tensor(v).to(dev)[None]  # noqa: E731
        rows = absolute_pose(mk0, mk1, nm, one(K0), one(K1), depth0=one(depth0), T_0to1=one(T_0to1), thresh=self.ransac_thresh,
                             conf=self.ransac_conf, ordering=self.ordering)[4]
        return rows[0].cpu().numpy()

    @torch.no_grad()
    def update_one(self, matched_keypoints1, matched_keypoints2, K0, K1, depth0, T_0to1):
        row = self.estimate_rows(matched_keypoints1, matched_keypoints2, K0, K1, depth0, T_0to1)
        self.rows.append(row)
        return {k: v[0] for k, v in self.columns(row[None], self.thresholds, self.metric_name).items()}

    @torch.no_grad()
    def update_batch(self, matched_keypoints1, matched_keypoints2, K0, K1, depth0, T_0to1):
        assert len(matched_keypoints1) == len(matched_keypoints2) == len(K0) == len(K1) == len(depth0) == len(T_0to1)
        self.rows = []
        for i in range(len(matched_keypoints1)):
            self.update_one(matched_keypoints1[i], matched_keypoints2[i], K0[i], K1[i], depth0[i], T_0to1[i])
        return self.compute()

    def compute(self):
        """the keys over every pair seen since construction (or the last update_batch)"""
        return self.summary(np.stack(self.rows) if self.rows else np.zeros((0, 5)), self.thresholds, self.metric_name)
