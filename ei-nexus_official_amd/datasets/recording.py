"""A rectified recording on the device, and the pair batches the different-time evaluator takes.

The reference assembles a validation pair on the host, per item (MVSECDataset_RPE_VAL.__getitem__, datasets/MVSEC.py:1035-1087):
twice get_depth_image_events_pose (:760-816: depth frame, the image paired with it, the pose interpolated at the depth stamp, the
events of the window that ends at the paired image's stamp), then get_relative_pose both ways (:818-830); the pairing itself is
get_paired_depth_and_image (:335-377).  `Recording` uploads the arrays of one sequence once -- events, images, depth frames, the
pose knots, the stamps, K -- and `pair_batches` yields, for a list of index pairs, the items of DifferentTimeEvaluator.run: all
relative transforms come from ONE PoseTrack.relative call, and a batch costs torch indexing on resident tensors plus the window
search on the host copy of the event stamps, with no device-to-host read-back."""
import numpy as np
import torch

from . import pairs as _pairs
from .poses import PoseTrack, nearest_index
from .sequence import EventSequence


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


class Recording:
    """events: an EventSequence, or the reference's dict {"x","y","t","p"}, which is wrapped in one; images: uint8 [Fi,H,W] with
    their stamps image_ts [Fi] (sorted); depth: float32 [Fd,H,W], holes (NaN) as they come, with depth_ts [Fd]; poses: a PoseTrack
    that covers every depth stamp; K: the 3x3 camera matrix of both views.  Numpy arrays are uploaded to `device` once; tensors that
    already lie there are used as they are.

    image_index [Fd] int64 (device): the image nearest in time to every depth frame (get_paired_depth_and_image's "nearest", the
    first of equally near ones); paired_image_ts [Fd] float64 (host): its stamp, where a view's event window ends.

    ValueError: shapes or types that do not match, stamps of the wrong length, an event sequence or a track on another device, a depth
    stamp outside the track."""

    def __init__(self, events, images, image_ts, depth, depth_ts, poses, K, device="cuda"):
        self.device = torch.device(device)
        if isinstance(events, EventSequence):
            self.events = events
        elif isinstance(events, dict):
            self.events = EventSequence(events, device=self.device)
        else:
            raise ValueError(f"Recording: events must be an EventSequence or a dict of numpy arrays, got {type(events).__name__}")
        if not isinstance(poses, PoseTrack):
            raise ValueError(f"Recording: poses must be a PoseTrack, got {type(poses).__name__}")
        self.poses = poses
        self.images = self._frames(images, torch.uint8, "images")
        self.depth = self._frames(depth, torch.float32, "depth")
        if self.images.shape[1:] != self.depth.shape[1:]:
            raise ValueError(f"Recording: images are {tuple(self.images.shape[1:])}, depth frames {tuple(self.depth.shape[1:])}")
        self.image_ts_host = np.ascontiguousarray(_host(image_ts), np.float64).reshape(-1)
        self.depth_ts_host = np.ascontiguousarray(_host(depth_ts), np.float64).reshape(-1)
        for name, ts, frames in (("image_ts", self.image_ts_host, self.images), ("depth_ts", self.depth_ts_host, self.depth)):
            if ts.shape[0] != frames.shape[0]:
                raise ValueError(f"Recording: {ts.shape[0]} {name} for {frames.shape[0]} frames")
        if self.images.shape[0] == 0 or self.depth.shape[0] == 0:
            raise ValueError("Recording: no images or no depth frames")
        if np.isnan(self.depth_ts_host).any():
            raise ValueError("Recording: depth_ts contains a NaN")
        lo, hi = poses.range
        if (self.depth_ts_host < lo).any() or (self.depth_ts_host > hi).any():
            raise ValueError(f"Recording: a depth stamp lies outside the pose track's range [{lo}, {hi}]")
        k = np.asarray(_host(K), np.float32)
        if k.shape != (3, 3):
            raise ValueError(f"Recording: K must be 3x3, got shape {k.shape}")
        self.K = torch.from_numpy(np.ascontiguousarray(k)).to(self.device)
        for name, t in (("events", self.events.t), ("the pose track", poses.stamps)):
            if t.device != self.K.device:
                raise ValueError(f"Recording: {name} lie on {t.device}, the recording on {self.K.device}")
        self.depth_ts = torch.from_numpy(self.depth_ts_host).to(self.device)
        # the pairing: one launch, and the one read-back of the construction (the windows are searched on the host)
        self.image_index = nearest_index(self.image_ts_host, self.depth_ts, device=self.device)
        self.paired_image_ts = self.image_ts_host[self.image_index.cpu().numpy()]
        self._poses_at_depth = None

    def _frames(self, a, dtype, what):
        t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dim() != 3:
            raise ValueError(f"Recording: {what} must be [F,H,W], got shape {tuple(t.shape)}")
        if t.dtype != dtype:
            raise ValueError(f"Recording: {what} must be {dtype}, got {t.dtype}")
        return t.to(self.device).contiguous()

    def __len__(self):
        """the number of depth frames: what a view index counts"""
        return int(self.depth.shape[0])

    def poses_at_depth(self):
        """[Fd,4,4] float32 T_j_W at every depth stamp (MVSEC.py:795), interpolated once and kept"""
        if self._poses_at_depth is None:
            self._poses_at_depth = self.poses.interpolate(self.depth_ts, dtype=torch.float32, inverse=True)
        return self._poses_at_depth

    def _pairs(self, pairs):
        p = np.asarray(_host(pairs))
        if p.size and not np.issubdtype(p.dtype, np.integer):
            raise ValueError(f"Recording: index pairs must be integers, got {p.dtype}")
        if p.ndim != 2 or p.shape[1] != 2:
            if p.size:
                raise ValueError(f"Recording: index pairs must be [P,2], got shape {p.shape}")
            p = p.reshape(0, 2)
        p = p.astype(np.int64)
        if p.size and (p.min() < 0 or p.max() >= len(self)):
            raise IndexError(f"Recording: an index outside [0, {len(self)})")
        return p

    def select_pairs(self, indices, **kw):
        """datasets.pairs.select_pairs on this recording's depth frames with poses_at_depth(); keywords are passed on"""
        return _pairs.select_pairs(self.depth, self.K, self.poses_at_depth(), self._pairs(indices), device=self.device, **kw)

    @torch.no_grad()
    def pair_batches(self, pairs, batch=32, events_dt=0.4):
        """The items of DifferentTimeEvaluator.run for the index pairs [P,2] (view 0, view 1; indices of depth frames), `batch` at a
        time, the last batch shorter (MVSECDataset_RPE_VAL.__getitem__, MVSEC.py:1035-1087, as test_events-image_different_time.py:179-184
        feeds it):

            (events.windows(paired_image_ts[i0], events_dt),   the events of view 0: the window ending at its image's stamp
             images[image_index[i1]][:, None].float(),          the image of view 1, values 0..255, [B,1,H,W]
             None,
             (K0, K1, T_0to1),                                  [B,3,3], [B,3,3], [B,4,4] float32
             (depth[i0], depth[i1]))                            [B,H,W] float32 each

        events_dt: the window length in seconds (the reference's configs: 0.4 for MVSEC, 0.04 for EC).  Every T_0to1 comes from one
        PoseTrack.relative call before the first batch; a batch itself reads nothing back from the device.
        IndexError: an index outside [0, Fd); ValueError: pairs that are not [P,2] integers, batch < 1."""
        p = self._pairs(pairs)
        batch = int(batch)
        if batch < 1:
            raise ValueError(f"Recording: batch must be at least 1, got {batch}")
        idx = torch.from_numpy(p).to(self.device)
        i0, i1 = idx[:, 0].contiguous(), idx[:, 1].contiguous()
        T01, _ = self.poses.relative(self.depth_ts[i0], self.depth_ts[i1])
        for s in range(0, len(p), batch):
            e = min(s + batch, len(p))
            K = self.K.expand(e - s, 3, 3).contiguous()
            yield (self.events.windows(self.paired_image_ts[p[s:e, 0]], events_dt),
                   self.images[self.image_index[i1[s:e]]][:, None].float(),
                   None,
                   (K, K, T01[s:e]),
                   (self.depth[i0[s:e]], self.depth[i1[s:e]]))
