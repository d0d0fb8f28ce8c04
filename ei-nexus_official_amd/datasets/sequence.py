"""A sequence's events on the device, and windows into them.

The reference's datasets keep ONE long, time-sorted event stream per sequence and cut a window out of it for every frame
(MVSECDataset.get_events_at_timestamp, datasets/MVSEC.py:723-758; ECDataset.get_events_at_timestamp, datasets/EC.py:253-262):

    index0 = np.searchsorted(t, timestamp - events_dt, side="left")
    index1 = np.searchsorted(t, timestamp, side="right")

`EventSequence` uploads such a stream once; `EventSequence.windows` applies that rule on the host (two numpy calls) and gives an
`EventWindows`, which every representation function and both evaluators take in place of a list of per-sample event dicts: the
windowed ops of include/einx.h then read the resident arrays at begin[b] .. end[b] - 1, with no packing and no upload per batch."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .. import _native as N
from .._lib import check

FIELDS = (("x", torch.float32), ("y", torch.float32), ("t", torch.float64), ("p", torch.float32))

# element types einx_events_pack converts from (include/einx.h: EINX_EV_*); anything else goes through float64 first
EV_TYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int64): 2, np.dtype(np.int32): 3, np.dtype(np.int16): 4,
            np.dtype(np.uint16): 5, np.dtype(np.int8): 6, np.dtype(np.uint8): 7, np.dtype(np.uint32): 8, np.dtype(np.uint64): 9,
            np.dtype(np.bool_): 7}


def event_arrays(ev, keep, what="events"):
    """one dict {"x","y","t","p"} of numpy arrays -> the _lib.EventArrays einx_events_pack reads; the arrays it points to (the
    caller's, or contiguous copies of them) are appended to `keep`, which must outlive the call"""
    fields = []
    for name in ("x", "y", "t", "p"):
        a = np.asarray(ev[name])
        code = EV_TYPES.get(a.dtype)
        if code is None or not a.flags["C_CONTIGUOUS"]:
            a = np.ascontiguousarray(a, None if code is not None else np.float64)
            code = EV_TYPES[a.dtype]
        keep.append(a)
        fields.append((a.ctypes.data, code))
    ln = len(keep[-4])
    if not all(len(k) == ln for k in keep[-4:]):
        raise ValueError(f"{what}: x / y / t / p differ in length")
    return _lib.EventArrays(fields[0][0], fields[1][0], fields[2][0], fields[3][0], fields[0][1], fields[1][1], fields[2][1], fields[3][1], ln)


def _check_stamps(t):
    """the window search is only defined on sorted stamps"""
    if np.isnan(t).any():
        raise ValueError("EventSequence: t contains a NaN")
    if t.size > 1 and (t[1:] < t[:-1]).any():
        k = int(np.argmax(t[1:] < t[:-1]))
        raise ValueError(f"EventSequence: t is not non-decreasing (t[{k + 1}] < t[{k}])")


class EventSequence:
    """The events of a whole sequence, resident on `device`: x / y / p as fp32 and t as fp64, converted element by element as
    einx_events_pack converts a batch's slices (C casts), so that a window holds exactly the values the packed path would have
    uploaded for the same slice.  `t_host` is the float64 host copy the windows are searched in.  The device arrays are only ever
    read."""

    def __init__(self, events, device="cuda"):
        """events: the reference's dict {"x","y","t","p"} of numpy arrays for the whole sequence (left untouched; `events_list`
        of a window returns slices of it).  ValueError: arrays of different lengths, a NaN in t, a t that decreases somewhere."""
        lens = {name: len(np.asarray(events[name])) for name in ("x", "y", "t", "p")}
        if len(set(lens.values())) != 1:
            raise ValueError("EventSequence: x / y / t / p differ in length: " + ", ".join(f"{k}: {v}" for k, v in lens.items()))
        self.events = {name: np.asarray(events[name]) for name in ("x", "y", "t", "p")}
        self.device = torch.device(device)
        n = lens["t"]
        host = {name: torch.empty(n, dtype=dt) for name, dt in FIELDS}  # (pageable: one upload, of any length)
        if n > 0:
            keep = []
            arr = (_lib.EventArrays * 1)(event_arrays(self.events, keep, "EventSequence"))
            offs = np.zeros(2, np.int64)
            from .representations import EventStage
            check(N.lib().einx_events_pack(arr, 1, *(ctypes.c_void_p(host[name].data_ptr()) for name, _ in FIELDS),
                                           offs.ctypes.data_as(ctypes.c_void_p), EventStage.pack_threads()), "einx_events_pack")
        self.t_host = host["t"].numpy()
        _check_stamps(self.t_host)
        self.x, self.y, self.t, self.p = (host[name].to(self.device) for name, _ in FIELDS)  # the one upload (blocking)

    @classmethod
    def from_tensors(cls, x, y, t, p):
        """the same from four 1-D tensors that are already on the device (converted to fp32 / fp64 there when they are of
        another type); t is read back once for the search"""
        lens = {name: int(v.numel()) for name, v in (("x", x), ("y", y), ("t", t), ("p", p))}
        if len(set(lens.values())) != 1 or any(v.dim() != 1 for v in (x, y, t, p)):
            raise ValueError("EventSequence: x / y / t / p must be 1-D and of one length: " + ", ".join(f"{k}: {v}" for k, v in lens.items()))
        if len({v.device for v in (x, y, t, p)}) != 1:
            raise ValueError("EventSequence: x / y / t / p lie on different devices")
        x, y, t, p = (v.detach().to(dt).contiguous() for v, (_, dt) in zip((x, y, t, p), FIELDS))
        return cls._from_parts(x, y, t, p, t.cpu().numpy())  # (the read-back waits for the conversions above as well)

    @classmethod
    def _from_parts(cls, x, y, t, p, t_host, check=True):
        """a sequence around four contiguous device arrays of the right types and the host copy of their stamps, as they are (no
        conversion, no copy, no read-back); check=False: the caller vouches that the stamps are sorted (a subsequence of a
        sequence's)"""
        self = cls.__new__(cls)
        self.events = None
        self.device = t.device
        self.x, self.y, self.t, self.p = x, y, t, p
        self.t_host = t_host
        if check:
            _check_stamps(self.t_host)
        return self

    def __len__(self):
        return int(self.t_host.shape[0])

    def windows(self, timestamps, events_dt):
        """One window per timestamp: the events with timestamp - events_dt <= t <= timestamp, both sides inclusive (every event of a
        run of equal stamps on a boundary is in) -- the reference's two searchsorted calls, `timestamp - events_dt` evaluated in
        float64.  A negative events_dt gives empty windows, like the reference's slice with index0 > index1."""
        ts = np.atleast_1d(np.asarray(timestamps, np.float64))
        begin = np.searchsorted(self.t_host, ts - np.float64(events_dt), side="left")
        end = np.searchsorted(self.t_host, ts, side="right")
        return EventWindows(self, begin, np.maximum(end, begin))

    def rectified(self, map_x, map_y, rule):
        """this stream rectified on the device (datasets/rectify.py::rectify_events): a new, shorter EventSequence"""
        from .rectify import rectify_events
        return rectify_events(self, map_x, map_y, rule)

    def windows_from_ranges(self, begin, end):
        """windows by explicit event indices: sample b is the events begin[b] <= k < end[b]"""
        return EventWindows(self, begin, end)


class EventWindows:
    """B windows (begin[b], end[b]) into one EventSequence: what the representation functions and the evaluators take in place of a
    list of B event dicts.  Windows may overlap, repeat, leave gaps, lie in any order or be empty."""

    def __init__(self, sequence, begin, end):
        self.sequence = sequence
        self.begin = np.ascontiguousarray(np.atleast_1d(begin), np.int64)
        self.end = np.ascontiguousarray(np.atleast_1d(end), np.int64)
        if self.begin.ndim != 1 or self.begin.shape != self.end.shape:
            raise ValueError("EventWindows: begin and end must be 1-D and of one length")
        if ((self.begin < 0) | (self.end < self.begin) | (self.end > len(sequence))).any():
            raise ValueError(f"EventWindows: 0 <= begin <= end <= {len(sequence)} does not hold for every window")
        self.counts = self.end - self.begin
        self.total = int(self.counts.sum())

    def __len__(self):
        return int(self.begin.shape[0])

    def events_list(self):
        """the B dicts {"x","y","t","p"} of numpy arrays the reference would have built: slices (views) of the sequence's host
        arrays; of a sequence made from device tensors: of one read-back"""
        seq = self.sequence
        if seq.events is None:
            seq.events = {name: getattr(seq, name).cpu().numpy() for name, _ in FIELDS}
        return [{name: a[b0:b1] for name, a in seq.events.items()} for b0, b1 in zip(self.begin.tolist(), self.end.tolist())]

    def args(self):
        """(stream_len, begin_host, end_host) of the windowed ops' C signatures"""
        return len(self.sequence), self.begin.ctypes.data_as(ctypes.c_void_p), self.end.ctypes.data_as(ctypes.c_void_p)
