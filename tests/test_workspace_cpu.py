"""Every *_ws_bytes query against the value the parent commit's library returned for the same arguments.

The ops' workspace layouts moved onto one carve function each (csrc/einx_common.h: WsCarver), used from a null base by the size
query and from the caller's pointer by the call.  That must not change what a caller allocates: TABLE holds, per query and
argument tuple, what the library built from the parent commit returned (recorded once from that build, never from the code under
test).  Queries whose parent layout was a walk of 256-byte aligned regions must return exactly that; the three whose parent layout
had unaligned regions (GROWTH: query -> number of regions) may grow by the rounding of each region and by no more:
parent <= new < parent + 256 * regions.  Zero returns (bad shapes, head widths LightGlue refuses) stay zero.

No GPU: the queries, and einx_extractor_create, are host code.
"""
import ctypes
from importlib import import_module

import pytest

from helpers import load_pkg

pkg = load_pkg()
_lib = import_module(pkg.__name__ + "._lib")

# regions of the layouts that had unaligned ones at the parent commit
GROWTH = {
    "detect": 3,   # buf0, buf1, flags
    "events": 4,   # statistics, count image, min/max, offsets
    "extract": 7,  # buf0, buf1, head, second head, and the nested detector's three
}


def _conv(cin, cout, ks=3, relu=1, pool=0):
    # placeholder non-null weight pointers: nothing dereferences them before a launch
    return _lib.ConvDesc(0x1000, 0x1000, None, None, cin, cout, ks, relu, pool)


# (cell, backbone, detector head, descriptor head, nms radius, top_k): a SuperPoint-shaped network (1/8-resolution heads) and a
# SiLK-shaped one (full-resolution heads)
NETWORKS = {
    "cell8": (8, [_conv(1, 64), _conv(64, 64), _conv(64, 64, pool=1), _conv(64, 64), _conv(64, 128, pool=1), _conv(128, 128),
                  _conv(128, 128, pool=1), _conv(128, 128)],
              [_conv(128, 256), _conv(256, 65, ks=1, relu=0)], [_conv(128, 256), _conv(256, 256, ks=1, relu=0)], 4, 1024),
    "cell1": (1, [_conv(1, 64), _conv(64, 64), _conv(64, 128), _conv(128, 128)],
              [_conv(128, 128), _conv(128, 1, ks=1, relu=0)], [_conv(128, 128), _conv(128, 128, ks=1, relu=0)], 0, 512),
}
_handles = {}


def _handle(lib, name):
    if (id(lib), name) not in _handles:
        cell, bb, det, desc, radius, top_k = NETWORKS[name]
        arr = lambda layers: (_lib.ConvDesc * len(layers))(*layers)  # noqa: E731
        d = _lib.ExtractorDesc(ctypes.sizeof(_lib.ExtractorDesc), cell, len(bb), len(det), len(desc), arr(bb), arr(det), arr(desc), 1, 4, radius,
                               top_k, 1.0, 0, 1.0, 0.0, None)
        create = lib.einx_extractor_create
        create.restype, create.argtypes = _lib.SIGNATURES["einx_extractor_create"]
        h = create(ctypes.byref(d))
        assert h, name
        _handles[(id(lib), name)] = h
    return _handles[(id(lib), name)]


def query(lib, name, args):
    """one size query of `lib` (a ctypes library with einx.h's symbols)"""
    def fn(sym):
        f = getattr(lib, sym)
        f.restype, f.argtypes = _lib.SIGNATURES[sym]
        return f

    if name == "mnn":
        return fn("einx_mnn_ws_bytes")(*args)
    if name == "lg":
        return fn("einx_lg_ws_bytes")(*args)
    if name == "lg_heads":
        return fn("einx_lg_ws_bytes_heads")(*args)
    if name == "voxel":
        return fn("einx_voxel_ws_bytes")(*args)
    if name == "events":
        return fn("einx_events_ws_bytes")(*args)
    if name == "detect":  # (B, Hp, Wp, H, W, radius, top_k, cap, nms_iters)
        B, Hp, Wp, H, W, radius, top_k, cap, iters = args
        p = _lib.DetectParams(B, Hp, Wp, H, W, (Hp - H) // 2, (Wp - W) // 2, radius, top_k, 1.0, 0, cap, iters)
        return fn("einx_detect_ws_bytes")(ctypes.byref(p))
    if name == "metrics":  # (B, cap0, cap1)
        B, cap0, cap1 = args
        p = _lib.MetricParams(B, cap0, cap1, 256, 3, 260, 346, 260, 346, 1, 2, 2)
        return fn("einx_metrics_ws_bytes")(ctypes.byref(p))
    if name == "pose":  # (B, cap, max_iters)
        B, cap, iters = args
        p = _lib.PoseParams(ctypes.sizeof(_lib.PoseParams), B, cap, 2, 1, 1, iters, 1.0, 0.999, 0)
        return fn("einx_relative_pose_ws_bytes")(ctypes.byref(p))
    if name == "homography":  # (B, cap, max_iters, n_thr)
        B, cap, iters, n_thr = args
        p = _lib.HomographyParams(ctypes.sizeof(_lib.HomographyParams), B, cap, 2, 1, iters, n_thr, 3.0, 0.995)
        return fn("einx_homography_ws_bytes")(ctypes.byref(p))
    if name == "extract":  # (network, B, H, W, cap, nms_iters)
        return fn("einx_extract_ws_bytes")(_handle(lib, args[0]), *args[1:])
    raise KeyError(name)


# (query, arguments, what the parent commit's library returned)
TABLE = [
    ('mnn', (1, 1024, 1024), 434176),
    ('lg', (1, 1024, 1024, 256, 256), 18277632),
    ('lg_heads', (1, 1024, 1024, 256, 4, 256), 18277632),
    ('voxel', (1, 5, 260, 346, 60000), 2191104),
    ('events', (1, 260, 346), 360152),
    ('detect', (1, 264, 352, 260, 346, 4, 1024, 1024, 8), 743936),
    ('metrics', (1, 1024, 1024), 43520),
    ('pose', (1, 1024, 1000), 799744),
    ('homography', (1, 1024, 2000, 3), 152576),
    ('extract', ('cell8', 1, 260, 346, 1024, 8), 51297024),
    ('extract', ('cell1', 1, 260, 346, 512, 8), 115869440),
    ('mnn', (32, 1024, 1024), 13893632),
    ('lg', (32, 1024, 1024, 256, 256), 584844544),
    ('lg_heads', (32, 1024, 1024, 256, 4, 256), 584844544),
    ('voxel', (32, 5, 260, 346, 1920000), 70093312),
    ('events', (32, 260, 346), 11516680),
    ('detect', (32, 264, 352, 260, 346, 4, 1024, 1024, 8), 23790848),
    ('metrics', (32, 1024, 1024), 1378560),
    ('pose', (32, 1024, 1000), 25562880),
    ('homography', (32, 1024, 2000, 3), 4864512),
    ('extract', ('cell8', 32, 260, 346, 1024, 8), 1641481728),
    ('extract', ('cell1', 32, 260, 346, 512, 8), 3707792896),
    ('mnn', (64, 1024, 1024), 27787264),
    ('lg', (64, 1024, 1024, 256, 256), 1169688064),
    ('lg_heads', (64, 1024, 1024, 256, 4, 256), 1169688064),
    ('voxel', (64, 5, 260, 346, 3840000), 140186112),
    ('events', (64, 260, 346), 23033096),
    ('detect', (64, 264, 352, 260, 346, 4, 1024, 1024, 8), 47581440),
    ('metrics', (64, 1024, 1024), 2756864),
    ('pose', (64, 1024, 1000), 51125248),
    ('homography', (64, 1024, 2000, 3), 9728768),
    ('extract', ('cell8', 64, 260, 346, 1024, 8), 3282962944),
    ('extract', ('cell1', 64, 260, 346, 512, 8), 7415585280),
    ('voxel', (32, 5, 264, 352, 1920000), 70126848),
    ('events', (32, 264, 352), 11896584),
    ('mnn', (1, 37, 1000), 42752),
    ('mnn', (3, 1000, 37), 115200),
    ('mnn', (2, 100, 300), 44288),
    ('mnn', (5, 129, 63), 38144),
    ('mnn', (1, 1, 1), 2048),
    ('mnn', (7, 513, 511), 860672),
    ('lg_heads', (2, 100, 300, 256, 4, 256), 7015936),
    ('lg_heads', (1, 37, 37, 256, 4, 256), 650240),
    ('lg_heads', (3, 33, 33, 128, 4, 128), 872960),
    ('lg_heads', (1, 1, 1, 256, 4, 256), 21760),
    ('lg_heads', (5, 129, 63, 512, 8, 256), 16267776),
    ('lg_heads', (2, 65, 65, 96, 3, 96), 881920),
    ('lg_heads', (1, 1023, 1024, 256, 4, 256), 18268928),
    ('lg_heads', (4, 50, 50, 240, 4, 240), 3283712),
    ('lg_heads', (2, 100, 100, 256, 1, 256), 4120320),
    ('lg', (2, 100, 300, 256, 256), 7015936),
    ('lg', (1, 37, 37, 128, 128), 347136),
    ('lg', (3, 511, 511, 64, 64), 8230912),
    ('voxel', (1, 5, 260, 346, 0), 30976),
    ('voxel', (2, 5, 90, 122, 1), 9728),
    ('voxel', (3, 3, 17, 33, 12345), 448512),
    ('voxel', (1, 10, 480, 640, 999999), 36252160),
    ('voxel', (4, 1, 8, 8, 77), 7936),
    ('events', (1, 8, 8), 568),
    ('events', (3, 17, 33), 7140),
    ('events', (2, 90, 122), 88200),
    ('events', (5, 1, 1), 524),
    ('events', (7, 480, 640), 8602200),
    ('detect', (2, 96, 128, 90, 122, 4, 64, 64, 8), 197120),
    ('detect', (3, 17, 33, 17, 33, 0, 0, 561, 8), 13976),
    ('detect', (1, 8, 8, 8, 8, 0, 0, 64, 0), 1024),
    ('detect', (5, 90, 122, 90, 122, 2, 100, 100, 3), 439712),
    ('detect', (33, 24, 40, 17, 33, 4, 10, 10, 100), 267008),
    ('detect', (1, 9, 7, 9, 7, 1, 5, 5, 1), 1016),
    ('metrics', (1, 37, 1000), 23040),
    ('metrics', (3, 100, 300), 26880),
    ('metrics', (1, 1, 1), 2048),
    ('metrics', (5, 129, 63), 21760),
    ('pose', (3, 37, 100), 233984),
    ('pose', (1, 5, 1), 2560),
    ('pose', (5, 129, 333), 1295360),
    ('homography', (3, 37, 100, 1), 23296),
    ('homography', (1, 4, 1, 0), 768),
    ('homography', (5, 129, 333, 4), 127232),
    ('extract', ('cell8', 2, 90, 122, 64, 8), 13566720),
    ('extract', ('cell8', 1, 8, 8, 16, 0), 36096),
    ('extract', ('cell8', 3, 17, 33, 100, 3), 1590528),
    ('extract', ('cell8', 5, 264, 352, 1024, 32), 256482560),
    ('extract', ('cell1', 1, 64, 64, 512, 8), 7373568),
    ('extract', ('cell1', 2, 64, 64, 512, 8), 14746368),
    ('extract', ('cell1', 3, 64, 64, 512, 8), 15827712),
    ('extract', ('cell1', 1, 17, 33, 100, 4), 1010688),
    ('extract', ('cell1', 2, 90, 122, 64, 0), 28285440),
    ('mnn', (0, 1024, 1024), 0),
    ('mnn', (32, 0, 1024), 0),
    ('mnn', (32, 1024, -1), 0),
    ('lg', (32, 1024, 1024, 100, 100), 0),
    ('lg', (32, 1024, 1024, 0, 0), 0),
    ('lg', (0, 1024, 1024, 256, 256), 0),
    ('lg_heads', (32, 1024, 1024, 256, 3, 256), 0),
    ('lg_heads', (32, 1024, 1024, 256, 0, 256), 0),
    ('lg_heads', (32, 1024, 1024, 1028, 2, 256), 0),
    ('lg_heads', (32, 1024, 1024, 6, 1, 6), 0),
    ('lg_heads', (32, 0, 1024, 256, 4, 256), 0),
    ('voxel', (0, 5, 260, 346, 100), 0),
    ('voxel', (32, 0, 260, 346, 100), 0),
    ('voxel', (32, 5, 260, 346, -1), 0),
    ('events', (0, 260, 346), 0),
    ('events', (32, 260, 0), 0),
    ('metrics', (0, 1024, 1024), 0),
    ('pose', (0, 1024, 1000), 0),
    ('pose', (32, 1024, 0), 0),
    ('homography', (32, 0, 2000, 3), 0),
    ('extract', ('cell8', 0, 260, 346, 1024, 8), 0),
    ('extract', ('cell1', 32, 0, 346, 512, 8), 1536),
]


@pytest.mark.parametrize("name,args,parent", TABLE, ids=[f"{n}{a}".replace(" ", "").replace("'", "") for n, a, _ in TABLE])
def test_size_query_returns_what_the_parent_returned(name, args, parent):
    got = query(pkg.native.lib(), name, args)
    print(f"{name}{args}: parent {parent}, now {got} ({got - parent:+d})")
    if name in GROWTH and parent:
        assert parent <= got < parent + 256 * GROWTH[name]
    else:
        assert got == parent


def test_table_covers_every_query_and_its_zero_returns():
    names = {n for n, _, _ in TABLE}
    assert names == {"mnn", "lg", "lg_heads", "voxel", "events", "detect", "metrics", "pose", "homography", "extract"}
    for n in ("mnn", "lg", "lg_heads", "voxel", "events", "metrics", "extract"):
        assert any(p == 0 for m, _, p in TABLE if m == n), f"no zero return of {n} in the table"
