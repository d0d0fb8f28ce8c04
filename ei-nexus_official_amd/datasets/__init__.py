"""The reference's `datasets` package, as far as it runs on the device: the event representations (representations.py), a
sequence's resident events with the windows cut out of them (sequence.py) and the selection of validation pairs by covisibility
(pairs.py, imported as a submodule), the rectification of raw recordings that comes before all of them (rectify.py), a recording's
pose track (poses.py) and the recording itself with the pair batches an evaluator takes (recording.py, imported as a submodule),
and the perspective warp that makes the second view of a homographic pair (warp.py)."""
from .sequence import EventSequence, EventWindows  # noqa: F401
from .rectify import (fisheye_rectify_map, radtan_rectify_map, radtan_undistort_points_map, rectify_events, remap)  # noqa: F401
from .poses import PoseTrack, nearest_index  # noqa: F401
from .warp import invert_homography, warp_perspective  # noqa: F401
