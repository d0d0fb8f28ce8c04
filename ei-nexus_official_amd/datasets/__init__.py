"""The reference's `datasets` package, as far as it runs on the device: the event representations (representations.py), a
sequence's resident events with the windows cut out of them (sequence.py) and the selection of validation pairs by covisibility
(pairs.py, imported as a submodule)."""
from .sequence import EventSequence, EventWindows  # noqa: F401
