"""The reference's `datasets` package, as far as it runs on the device: the event representations (representations.py), a
sequence's resident events with the windows cut out of them (sequence.py) and the selection of validation pairs by covisibility
(pairs.py, imported as a submodule), and the rectification of raw recordings that comes before all of them (rectify.py)."""
from .sequence import EventSequence, EventWindows  # noqa: F401
from .rectify import (fisheye_rectify_map, radtan_rectify_map, radtan_undistort_points_map, rectify_events, remap)  # noqa: F401
