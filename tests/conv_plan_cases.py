"""The conv dispatcher's coverage table: at least one launch for every kernel instantiation einx_conv_block can select, with the
name einx_conv_plan / einx_conv_last_kernel report for it.  Not collected by pytest (no test_ prefix); used by
test_conv_plan_cpu.py (every case plans to its name; no name the dispatcher produces is missing here) and by
test_conv_gpu.py::test_every_conv_instantiation_bit_exact (each case bit-equal to the oracle, guard zones intact).

RULE: a new instantiation in csrc/conv.hip needs a row here.  The CPU sweep fails on a name without one.

Each case was found with einx_conv_plan (no launch) as the smallest launch that selects the kernel with the stated properties.
Per kernel the cases between them hold, where the dispatcher's conditions allow it:
  * a map that is no multiple of the tile in H and in W, and one that fits exactly;
  * 70 or 130 output channels (ragged, two or three channel tiles of 64);
  * an input-channel count with a partial last chunk (12, 20; 72 or 40 for the 32-channel chunks of the 1x1 kernels) and one with
    two full chunks.  For the generic 3x3 tiles: a thin case (cin <= 6, any size) and a multi-chunk case (cin >= 16) whose
    launch has >= 512 workgroups with every candidate tile, so that neither conv16 nor the latency picks take it;
  * a replicate-padding fold (h0, w0, Hs, Ws) = (1, 2, H - 3, W - 3): padding on all four sides.  conv16 refuses folds, which is
    how a folded case with cin % 8 == 0 reaches the latency picks;
  * BatchNorm (with one negative gain, set by the test) and ReLU on / off, spread over the rows.
What the conditions rule out: the conv16 kernels and the xtra variant need whole chunks (cin % 8 == 0, cin % 32 == 0); pooled maps
have even sizes, so conv16's 2-row tiles always fit in H.  The three-per-CU variants need >= 6144 workgroups: their exact-fit rows
are one whole 8x32 tile per image at B = 6144 with few output channels, which keeps them below the size limit.
Input plus output of a case stay below 64 MB."""

CONV_PLAN_CASES = [
    # B, cin, cout, H, W, ks, relu, bn, pool, fold (h0, w0, Hs, Ws) or None, expected name
    # conv16_1x1_kernel<1>: 1x1 small grids: 16-pixel runs, one N-tile per wave (cin % 32 == 0 only)
    (2, 64, 70, 5, 13, 1, True, True, False, None, "conv16_1x1_kernel<1>"),  # 65 pixels: ragged last run; two channel tiles, two chunks
    (1, 32, 7, 4, 8, 1, True, False, False, None, "conv16_1x1_kernel<1>"),  # two whole runs, one chunk
    # conv16_1x1_kernel<2>
    (2, 64, 70, 61, 67, 1, False, True, False, None, "conv16_1x1_kernel<2>"),  # ragged last 32-pixel run
    (1, 32, 1, 128, 128, 1, True, False, False, None, "conv16_1x1_kernel<2>"),  # 512 whole runs
    # conv16_1x1_kernel<4>
    (2, 64, 70, 97, 101, 1, True, True, False, None, "conv16_1x1_kernel<4>"),  # ragged last 64-pixel run
    (2, 32, 1, 128, 128, 1, False, False, False, None, "conv16_1x1_kernel<4>"),  # whole runs
    # conv16_kernel<false,8,1>: 3x3 small grids: 2 x 8 pixel tiles per N-tile (cin % 8 == 0, no fold)
    (2, 16, 70, 5, 13, 3, True, True, False, None, "conv16_kernel<false,8,1>"),  # odd H and W % 8 != 0; two channel tiles, two chunks
    (1, 8, 7, 4, 16, 3, True, False, False, None, "conv16_kernel<false,8,1>"),  # exact fit, one chunk
    # conv16_kernel<false,8,2>
    (1, 16, 70, 45, 181, 3, False, True, False, None, "conv16_kernel<false,8,2>"),  # odd H, W % 16 != 0
    (1, 8, 7, 128, 128, 3, True, False, False, None, "conv16_kernel<false,8,2>"),  # exact fit
    # conv16_kernel<false,8,4>
    (1, 16, 70, 257, 33, 3, True, True, False, None, "conv16_kernel<false,8,4>"),  # odd H, one pixel in the second 32-pixel tile
    (2, 8, 7, 128, 128, 3, False, False, False, None, "conv16_kernel<false,8,4>"),  # exact fit
    # conv16_kernel<true,8,1>: pooled (H, W even, so only W can leave a partial tile)
    (2, 16, 70, 6, 20, 3, True, True, True, None, "conv16_kernel<true,8,1>"),  # W % 8 != 0
    (1, 8, 7, 4, 16, 3, True, False, True, None, "conv16_kernel<true,8,1>"),  # exact fit
    # conv16_kernel<true,8,2>
    (2, 16, 70, 128, 18, 3, False, True, True, None, "conv16_kernel<true,8,2>"),  # W % 16 != 0
    (1, 8, 7, 128, 128, 3, True, False, True, None, "conv16_kernel<true,8,2>"),  # exact fit
    # conv16_kernel<true,8,4>
    (2, 16, 70, 128, 34, 3, True, True, True, None, "conv16_kernel<true,8,4>"),  # W % 32 != 0
    (2, 8, 7, 128, 128, 3, False, False, True, None, "conv16_kernel<true,8,4>"),  # exact fit
    # conv_block_kernel<1,1,128,1,4,2,1,32,false,xtra>: 1x1, 64 n + 1 output channels on n channel tiles (cin % 32 == 0 only)
    (32, 64, 65, 33, 44, 1, True, True, False, None, "conv_block_kernel<1,1,128,1,4,2,1,32,false,xtra>"),  # the detector head's layer: 1452 pixels, ragged last run, two chunks
    (2, 32, 129, 128, 128, 1, True, False, False, None, "conv_block_kernel<1,1,128,1,4,2,1,32,false,xtra>"),  # whole runs, 129 channels on two channel tiles
    # conv_block_kernel<1,1,128,1,4,2,1,32,false>: 1x1, 128-pixel runs
    (2, 72, 70, 9, 31, 1, False, True, False, None, "conv_block_kernel<1,1,128,1,4,2,1,32,false>"),  # 279 pixels; 72 channels: two chunks and a quarter; two channel tiles
    (4, 32, 7, 128, 128, 1, True, False, False, None, "conv_block_kernel<1,1,128,1,4,2,1,32,false>"),  # whole runs, one chunk, 512 workgroups
    # conv_block_kernel<1,1,256,1,4,2,2,32,false>: 1x1, 256-pixel runs (>= 1024 workgroups)
    (256, 40, 70, 16, 17, 1, True, True, False, None, "conv_block_kernel<1,1,256,1,4,2,2,32,false>"),  # 272 pixels: 16 in the second run; partial second chunk
    (16, 32, 7, 128, 128, 1, False, False, False, None, "conv_block_kernel<1,1,256,1,4,2,2,32,false>"),  # whole runs
    (256, 64, 70, 16, 17, 1, True, False, False, None, "conv_block_kernel<1,1,256,1,4,2,2,32,false>"),  # two full chunks
    # conv_block_kernel<3,8,32,2,4,1,2,2,false>: thin first layer, 1-2 input channels
    (1, 1, 70, 13, 45, 3, True, True, False, (1, 2, 10, 42), "conv_block_kernel<3,8,32,2,4,1,2,2,false>"),  # partial tiles on both edges, fold, two channel tiles
    (1, 2, 7, 16, 64, 3, True, False, False, None, "conv_block_kernel<3,8,32,2,4,1,2,2,false>"),  # exact fit, a whole channel pair
    # conv_block_kernel<3,8,32,2,4,1,2,6,false>: thin first layer, 3-6 input channels
    (1, 5, 70, 13, 45, 3, False, True, False, (1, 2, 10, 42), "conv_block_kernel<3,8,32,2,4,1,2,6,false>"),  # partial tiles on both edges, fold, half a channel pair
    (2, 3, 130, 24, 64, 3, True, False, False, None, "conv_block_kernel<3,8,32,2,4,1,2,6,false>"),  # exact fit, a pair and a half, three channel tiles
    (1, 6, 7, 16, 64, 3, True, True, False, None, "conv_block_kernel<3,8,32,2,4,1,2,6,false>"),  # exact fit, three whole pairs
    # conv_block_kernel<3,8,32,2,4,1,2,8,false>: generic 8x32 below the three-per-CU size, and the latency pick
    (64, 20, 70, 13, 45, 3, False, False, False, (1, 2, 10, 42), "conv_block_kernel<3,8,32,2,4,1,2,8,false>"),  # generic, 512 workgroups: partial tiles, fold, two chunks and a half
    (8, 16, 7, 128, 128, 3, True, True, False, None, "conv_block_kernel<3,8,32,2,4,1,2,8,false>"),  # generic, 512 workgroups: exact fit, two chunks
    (24, 20, 70, 13, 41, 3, True, False, False, (1, 2, 10, 38), "conv_block_kernel<3,8,32,2,4,1,2,8,false>"),  # latency pick: partial tiles, fold
    (24, 16, 7, 16, 96, 3, False, True, False, (1, 2, 13, 93), "conv_block_kernel<3,8,32,2,4,1,2,8,false>"),  # latency pick: exact fit, fold keeps it off conv16
    (24, 12, 70, 13, 41, 3, True, False, False, None, "conv_block_kernel<3,8,32,2,4,1,2,8,false>"),  # latency pick: no fold, a chunk and a half
    # conv_block_kernel<3,8,32,2,4,1,2,8,false> (3 per CU): >= 6144 workgroups
    (1536, 12, 7, 13, 41, 3, True, True, False, (1, 2, 10, 38), "conv_block_kernel<3,8,32,2,4,1,2,8,false> (3 per CU)"),  # partial tiles on both edges, fold, a chunk and a half
    (3072, 16, 7, 2, 33, 3, False, False, False, None, "conv_block_kernel<3,8,32,2,4,1,2,8,false> (3 per CU)"),  # two chunks
    (1536, 8, 70, 2, 33, 3, True, True, False, None, "conv_block_kernel<3,8,32,2,4,1,2,8,false> (3 per CU)"),  # two channel tiles
    (6144, 8, 3, 8, 32, 3, False, True, False, (1, 2, 5, 29), "conv_block_kernel<3,8,32,2,4,1,2,8,false> (3 per CU)"),  # exact fit, fold
    # conv_block_kernel<3,8,32,2,4,1,2,8,true>: generic pooled 8x32 (thin layers too) and the latency pick
    (1, 5, 70, 14, 42, 3, True, False, True, (1, 2, 11, 39), "conv_block_kernel<3,8,32,2,4,1,2,8,true>"),  # thin: partial tiles, fold
    (1, 3, 7, 16, 64, 3, False, True, True, None, "conv_block_kernel<3,8,32,2,4,1,2,8,true>"),  # thin: exact fit
    (64, 20, 70, 14, 42, 3, True, False, True, (1, 2, 11, 39), "conv_block_kernel<3,8,32,2,4,1,2,8,true>"),  # generic, 512 workgroups: partial tiles, fold
    (8, 16, 7, 128, 128, 3, True, True, True, None, "conv_block_kernel<3,8,32,2,4,1,2,8,true>"),  # generic, 512 workgroups: exact fit
    (8, 20, 70, 38, 66, 3, False, False, True, (1, 2, 35, 63), "conv_block_kernel<3,8,32,2,4,1,2,8,true>"),  # latency pick: partial tiles, fold
    (6, 16, 7, 88, 96, 3, True, True, True, (1, 2, 85, 93), "conv_block_kernel<3,8,32,2,4,1,2,8,true>"),  # latency pick: exact fit
    (12, 12, 70, 66, 18, 3, True, False, True, None, "conv_block_kernel<3,8,32,2,4,1,2,8,true>"),  # latency pick: no fold
    # conv_block_kernel<3,8,32,2,4,1,2,8,true> (3 per CU)
    (1536, 12, 7, 14, 42, 3, False, True, True, (1, 2, 11, 39), "conv_block_kernel<3,8,32,2,4,1,2,8,true> (3 per CU)"),  # partial tiles on both edges, fold, a chunk and a half
    (3072, 16, 7, 2, 34, 3, True, False, True, None, "conv_block_kernel<3,8,32,2,4,1,2,8,true> (3 per CU)"),  # two chunks
    (6144, 8, 7, 8, 32, 3, True, True, True, (1, 2, 5, 29), "conv_block_kernel<3,8,32,2,4,1,2,8,true> (3 per CU)"),  # exact fit, fold
    (1536, 8, 70, 2, 34, 3, False, False, True, None, "conv_block_kernel<3,8,32,2,4,1,2,8,true> (3 per CU)"),  # two channel tiles
    (768, 5, 70, 14, 42, 3, True, True, True, (1, 2, 11, 39), "conv_block_kernel<3,8,32,2,4,1,2,8,true> (3 per CU)"),  # thin layer
    # conv_block_kernel<3,12,16,2,2,1,3,8,false>: generic 12x16 and the latency pick
    (1, 5, 70, 17, 45, 3, True, False, False, (1, 2, 14, 42), "conv_block_kernel<3,12,16,2,2,1,3,8,false>"),  # thin: partial tiles, fold
    (1, 3, 7, 24, 48, 3, False, True, False, None, "conv_block_kernel<3,12,16,2,2,1,3,8,false>"),  # thin: exact fit
    (32, 20, 70, 25, 45, 3, True, False, False, (1, 2, 22, 42), "conv_block_kernel<3,12,16,2,2,1,3,8,false>"),  # generic, >= 512 workgroups: partial tiles, fold
    (24, 16, 7, 96, 48, 3, True, True, False, None, "conv_block_kernel<3,12,16,2,2,1,3,8,false>"),  # generic: exact fit
    (24, 20, 70, 13, 26, 3, False, False, False, (1, 2, 10, 23), "conv_block_kernel<3,12,16,2,2,1,3,8,false>"),  # latency pick: partial tiles, fold
    (32, 16, 7, 24, 32, 3, True, True, False, (1, 2, 21, 29), "conv_block_kernel<3,12,16,2,2,1,3,8,false>"),  # latency pick: exact fit
    (24, 12, 70, 13, 26, 3, True, False, False, None, "conv_block_kernel<3,12,16,2,2,1,3,8,false>"),  # latency pick: no fold
    # conv_block_kernel<3,12,16,2,2,1,3,8,true>
    (1, 5, 70, 34, 18, 3, False, True, True, (1, 2, 31, 15), "conv_block_kernel<3,12,16,2,2,1,3,8,true>"),  # thin: partial tiles, fold
    (1, 3, 7, 24, 48, 3, True, False, True, None, "conv_block_kernel<3,12,16,2,2,1,3,8,true>"),  # thin: exact fit
    (32, 20, 70, 34, 34, 3, True, True, True, (1, 2, 31, 31), "conv_block_kernel<3,12,16,2,2,1,3,8,true>"),  # generic: partial tiles, fold
    (24, 16, 7, 96, 48, 3, False, False, True, None, "conv_block_kernel<3,12,16,2,2,1,3,8,true>"),  # generic: exact fit
    (12, 20, 70, 42, 18, 3, True, True, True, (1, 2, 39, 15), "conv_block_kernel<3,12,16,2,2,1,3,8,true>"),  # latency pick: partial tiles, fold
    (48, 16, 7, 24, 32, 3, True, False, True, (1, 2, 21, 29), "conv_block_kernel<3,12,16,2,2,1,3,8,true>"),  # latency pick: exact fit
    (12, 12, 70, 42, 18, 3, False, True, True, None, "conv_block_kernel<3,12,16,2,2,1,3,8,true>"),  # latency pick: no fold
    # conv_block_kernel<3,22,8,2,2,1,3,8,false>: generic 22x8 (no latency pick has this tile)
    (1, 5, 70, 37, 23, 3, True, False, False, (1, 2, 34, 20), "conv_block_kernel<3,22,8,2,2,1,3,8,false>"),  # thin: partial tiles, fold
    (1, 6, 7, 44, 24, 3, True, True, False, None, "conv_block_kernel<3,22,8,2,2,1,3,8,false>"),  # thin: exact fit
    (32, 20, 70, 37, 33, 3, False, False, False, (1, 2, 34, 30), "conv_block_kernel<3,22,8,2,2,1,3,8,false>"),  # generic: partial tiles, fold
    (48, 16, 7, 88, 24, 3, True, True, False, None, "conv_block_kernel<3,22,8,2,2,1,3,8,false>"),  # generic: exact fit
    # conv_block_kernel<3,22,8,2,2,1,3,8,true>
    (1, 5, 70, 38, 18, 3, True, False, True, (1, 2, 35, 15), "conv_block_kernel<3,22,8,2,2,1,3,8,true>"),  # thin: partial tiles, fold
    (1, 6, 7, 44, 24, 3, False, True, True, None, "conv_block_kernel<3,22,8,2,2,1,3,8,true>"),  # thin: exact fit
    (32, 20, 70, 38, 34, 3, True, False, True, (1, 2, 35, 31), "conv_block_kernel<3,22,8,2,2,1,3,8,true>"),  # generic: partial tiles, fold
    (48, 16, 7, 88, 24, 3, True, True, True, None, "conv_block_kernel<3,22,8,2,2,1,3,8,true>"),  # generic: exact fit
    # conv_block_kernel<3,11,22,2,4,1,2,8,false>: generic 11x22 and the latency pick
    (32, 5, 70, 49, 33, 3, False, False, False, (1, 2, 46, 30), "conv_block_kernel<3,11,22,2,4,1,2,8,false>"),  # thin: partial tiles, fold
    (24, 3, 7, 88, 88, 3, True, True, False, None, "conv_block_kernel<3,11,22,2,4,1,2,8,false>"),  # thin: exact fit
    (32, 20, 70, 49, 33, 3, True, False, False, (1, 2, 46, 30), "conv_block_kernel<3,11,22,2,4,1,2,8,false>"),  # generic: partial tiles, fold
    (24, 16, 7, 88, 88, 3, False, True, False, None, "conv_block_kernel<3,11,22,2,4,1,2,8,false>"),  # generic: exact fit
    (24, 20, 70, 17, 41, 3, True, False, False, (1, 2, 14, 38), "conv_block_kernel<3,11,22,2,4,1,2,8,false>"),  # latency pick: partial tiles, fold
    (48, 16, 7, 22, 44, 3, True, True, False, (1, 2, 19, 41), "conv_block_kernel<3,11,22,2,4,1,2,8,false>"),  # latency pick: exact fit
    (24, 12, 70, 17, 41, 3, False, False, False, None, "conv_block_kernel<3,11,22,2,4,1,2,8,false>"),  # latency pick: no fold
    # conv_block_kernel<3,11,11,2,2,1,2,8,false>: generic 11x11 (launches of 512..639 workgroups, thin layers below) and the latency pick
    (1, 5, 70, 13, 17, 3, True, True, False, (1, 2, 10, 14), "conv_block_kernel<3,11,11,2,2,1,2,8,false>"),  # thin: partial tiles, fold
    (1, 3, 7, 22, 22, 3, True, False, False, None, "conv_block_kernel<3,11,11,2,2,1,2,8,false>"),  # thin: exact fit
    (128, 20, 70, 13, 17, 3, False, True, False, (1, 2, 10, 14), "conv_block_kernel<3,11,11,2,2,1,2,8,false>"),  # generic: partial tiles, fold
    (96, 16, 7, 33, 33, 3, True, False, False, None, "conv_block_kernel<3,11,11,2,2,1,2,8,false>"),  # generic: exact fit
    (24, 20, 70, 12, 12, 3, True, True, False, (1, 2, 9, 9), "conv_block_kernel<3,11,11,2,2,1,2,8,false>"),  # latency pick: one pixel past the tile in both directions, fold
    (32, 16, 7, 22, 22, 3, False, False, False, (1, 2, 19, 19), "conv_block_kernel<3,11,11,2,2,1,2,8,false>"),  # latency pick: exact fit
    (24, 12, 70, 12, 12, 3, True, True, False, None, "conv_block_kernel<3,11,11,2,2,1,2,8,false>"),  # latency pick: no fold
    # conv_block_kernel<3,11,5,2,2,1,1,8,false>: latency pick only
    (1, 20, 70, 12, 6, 3, True, False, False, (1, 2, 9, 3), "conv_block_kernel<3,11,5,2,2,1,1,8,false>"),  # one pixel past the tile in both directions, fold
    (1, 16, 7, 22, 10, 3, False, True, False, (1, 2, 19, 7), "conv_block_kernel<3,11,5,2,2,1,1,8,false>"),  # exact fit
    (2, 12, 70, 13, 7, 3, True, False, False, None, "conv_block_kernel<3,11,5,2,2,1,1,8,false>"),  # no fold
    # conv_block_kernel<3,8,16,2,2,1,2,8,true>: latency pick only
    (24, 20, 70, 10, 18, 3, True, True, True, (1, 2, 7, 15), "conv_block_kernel<3,8,16,2,2,1,2,8,true>"),  # partial tiles, fold
    (6, 16, 7, 88, 32, 3, False, False, True, (1, 2, 85, 29), "conv_block_kernel<3,8,16,2,2,1,2,8,true>"),  # exact fit
    (24, 12, 70, 10, 18, 3, True, True, True, None, "conv_block_kernel<3,8,16,2,2,1,2,8,true>"),  # no fold
    # conv_block_kernel<3,4,16,2,2,1,1,8,true>: latency pick only
    (1, 20, 70, 6, 18, 3, True, False, True, (1, 2, 3, 15), "conv_block_kernel<3,4,16,2,2,1,1,8,true>"),  # partial tiles, fold
    (1, 16, 7, 8, 32, 3, False, True, True, (1, 2, 5, 29), "conv_block_kernel<3,4,16,2,2,1,1,8,true>"),  # exact fit
    (2, 12, 70, 6, 20, 3, True, False, True, None, "conv_block_kernel<3,4,16,2,2,1,1,8,true>"),  # no fold
]

CONV_PLAN_NAMES = sorted({c[-1] for c in CONV_PLAN_CASES})


def case_id(c):
    return "x".join(str(v) for v in c[:6]) + ("p" if c[8] else "") + ("f" if c[9] else "")


def plan_args(c):
    """a table row -> the arguments of einx_conv_plan (cin, cout, ks, pool, B, Hs, Ws, h0, w0, H, W)"""
    B, cin, cout, H, W, ks, _relu, _bn, pool, fold = c[:10]
    h0, w0, Hs, Ws = fold if fold else (0, 0, H, W)
    return (cin, cout, ks, int(pool), B, Hs, Ws, h0, w0, H, W)


def plan_name(lib, *args):
    """einx_conv_plan as a str (None for arguments einx_conv_block refuses)"""
    r = lib.einx_conv_plan(*[int(a) for a in args])
    return None if r is None else r.decode()
