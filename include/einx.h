/* einx.h -- C ABI of libeinx_hip.so: the MI355X (gfx950) native implementation of the
 * EI-Nexus event<->image feature extraction + matching hot path.
 *
 * The reference (ZhonghuaYi/EI-Nexus_official) is pure Python/PyTorch and owns no native
 * layer, so the "FFI" a maintainer would bind is the set of torch op groups its nn.Modules
 * dispatch.  Each entry point below names the reference code it replaces (file:line relative
 * to the reference root).  Conventions:
 *   - plain pointers + sizes; every pointer is DEVICE memory unless it says "host";
 *   - tensors are dense, fp32, NCHW / row-major, exactly the reference's logical layouts;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue;
 *   - the caller makes the device of `stream` and of the buffers the current HIP device (hipSetDevice) before a call;
 *   - return 0 on success, negative on error (einx_last_error() gives the text);
 *   - no device-memory allocation inside: callers pass workspaces sized by the *_ws_bytes helpers.  Two documented pieces of
 *     library-owned state: (a) per device, two pools of EINX_FORK_STREAM_POOL side streams and EINX_FORK_STREAMS_MAX slots of two
 *     events each, created at the first use on that device and never destroyed; a slot lends a (caller stream, lane) the pool
 *     stream that runs beside it (see einx_fork_stream_prepare), shared by every handle of the process; (b) einx_voxel_grid /
 *     einx_events_mask keep a few hundred bytes of pinned staging per host thread for the host offsets array;
 *   - einx_build_flags() tells a shipped library from a timing-only experiment build (see below).
 * No torch types cross this boundary.  INTEGRATION.md shows the ctypes binding.
 */
#ifndef EINX_H
#define EINX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EINX_OK 0
#define EINX_ERR_ARG (-1)
#define EINX_ERR_LAUNCH (-2)
#define EINX_ERR_NO_DEVICE (-3)

/* ABI revision of this header.  The public structs change layout between revisions (6: struct_size members, the weight watch out
 * of einx_extract_out, einx_lg_layer::Wqk_v); a host compares einx_abi_version() with the EINX_ABI_VERSION it was compiled
 * against before anything else, and every struct that is read by the library starts with `struct_size` = sizeof(the struct),
 * which the library checks (EINX_ERR_ARG on a mismatch instead of reading garbage from a shorter / longer struct). */
#define EINX_ABI_VERSION 6
int einx_abi_version(void);
const char* einx_version(void);
const char* einx_last_error(void);
/* Compile-time switches of this binary as a space-separated string ("" for the shipped build).  Experiment builds
 * (tools/build_variant.sh) that drop work to time what is left produce WRONG results; every such switch only takes effect
 * under -DEINX_TIMING_ONLY_BUILD, which this string then reports as "timing-only" -- the Python package refuses to load such
 * a library unless EINX_ALLOW_TIMING_ONLY=1. */
const char* einx_build_flags(void);
/* number of visible HIP devices (0 without a GPU); never initialises a context beyond that */
int einx_device_count(void);

/* Content watch of a module's weights (the reference's nn.Modules see an in-place edit through `p.data` at the next forward,
 * torch/nn/modules/module.py semantics; here weights are repacked / folded at load time).  table: device [n][2] int64 =
 * (device pointer, number of 32-bit words) per row.  Every word of a row is hashed (position-dependent, order-independent sum:
 * any edit of any word changes the hash) by ONE 64-lane wave, so callers cut large tensors into rows of
 * EINX_WATCH_CHUNK_WORDS words (any row length works; short rows keep a row's loads in flight together).
 * ref == stale == NULL: store the hashes in hash[n]; otherwise hash[n] is scratch and *stale (device int32) is OR-ed with 1
 * when any row's hash differs from ref. */
#define EINX_WATCH_CHUNK_WORDS 4096
int einx_params_hash(const int64_t* table, int n, uint64_t* hash, const uint64_t* ref, int32_t* stale, void* stream);

/* The numeric contract on the device (test aid): y[i] = f(x[i]) for the functions of include/einx_math.h as compiled for gfx950
 * (fn: 0 exp, 1 log, 2 sin, 3 cos, 4 erf, 5 sigmoid, 6 logsigmoid, 7 gelu, 8 acos -- what torch.exp / log / sin / cos / erf /
 * sigmoid / F.logsigmoid / F.gelu / acos compute in the reference's modules).  The oracle compiles the same header with gcc;
 * tests hold the two bit-equal and the header within 2 ulp of float64 libm. */
int einx_math_eval(int fn, const float* x, long long n, float* y, void* stream);

/* Do two streams of the current device run side by side (no reference counterpart: the reference has one stream)?  HIP deals
 * streams onto a few hardware queues; two that share one serialise, and which share depends on everything the process created
 * before (a process group's streams, a loader's copy streams).  Holds one wave spinning for spin_us (1..5000) on each stream
 * between a common start and end and returns the elapsed time in *elapsed_us: about spin_us when they overlap, about twice that
 * when they do not (or when a == b).  Synchronises with both streams; not capturable.  The library uses it to choose its side
 * streams (einx_fork_stream_prepare). */
int einx_stream_overlap_us(void* stream_a, void* stream_b, int spin_us, float* elapsed_us);

/* Measurement aid (no reference counterpart; the reference's scripts time with wall clocks around
 * whole forwards, test_events-image_same-time.py:196-208): while enabled, every kernel launch of
 * this library is bracketed by HIP events recorded on the launch stream.  einx_profile_report
 * waits for them and writes one text line per kernel class, "name calls total_ms\n", into `buf`
 * (host memory).  einx_profile_enable(0|1) also clears the collected records.  While enabled einx_extract keeps its two head
 * branches in line (no fork), so that every number is a kernel alone on the chip. */
int einx_profile_enable(int on);
int einx_profile_report(char* buf, size_t cap);

/* ------------------------------------------------------------------------------------------
 * Convolution blocks  (K1/K2 of SURVEY.md 2.3)
 * replaces: nn.Conv2d(3x3,pad 1 | 1x1) + ReLU + BatchNorm2d(eval) + MaxPool2d(2,2)
 *   core/modules/net/vgg.py:34-38, core/modules/net/backbone.py:105-128,
 *   core/modules/net/detector_head.py:42-48, core/modules/net/descriptor_head.py:40-43,
 *   core/modules/image_extractors/superpoint_extractor.py:388-406,
 *   core/modules/image_extractors/silk/backbones/superpoint/vgg.py:284-290
 * and Padder.pad (replicate) folded into the first layer's addressing
 *   core/modules/utils/util.py:17-32.
 * ---------------------------------------------------------------------------------------- */

/* floats needed for the kernel-native weight image of one conv (k-major, cout padded to 64) */
size_t einx_conv_weight_elems(int cin, int cout, int ks);
/* OIHW fp32 -> kernel-native [K][CoutPad], K ordered (ci>>1, tap, ci&1); runs on `stream` */
int einx_conv_repack(const float* w_oihw, int cin, int cout, int ks, float* w_native, void* stream);

/* BatchNorm2d(eval) running statistics -> (scale, shift): scale = gamma/sqrt(var+eps),
 * shift = beta - mean*scale (torch.nn.BatchNorm2d in eval mode; core/modules/net/vgg.py:37) */
int einx_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int n, float* scale,
                 float* shift, void* stream);

typedef struct einx_conv_desc {
  const float* w_native; /* from einx_conv_repack */
  const float* bias;     /* [cout] or NULL */
  const float* scale;    /* [cout] BN(eval) gamma/sqrt(var+eps), or NULL (no BN) */
  const float* shift;    /* [cout] beta - mean*scale, or NULL */
  int32_t cin, cout, ks; /* ks in {1,3}; padding ks/2, stride 1 */
  int32_t relu;          /* apply ReLU after bias (before BN, as the reference orders it) */
  int32_t pool;          /* fuse MaxPool2d(2,2) after BN (H, W must be even) */
} einx_conv_desc;

/* in:  [B,cin,Hs,Ws] source tensor.  The layer sees a logical [B,cin,H,W] input where
 *      logical (y,x) = source (clamp(y-h0,0,Hs-1), clamp(x-w0,0,Ws-1))  (replicate padding);
 *      pass Hs=H, Ws=W, h0=w0=0 for an ordinary layer.
 * out: [B,cout,H,W] or [B,cout,H/2,W/2] when pool. */
int einx_conv_block(const float* in, int B, int Hs, int Ws, int h0, int w0, int H, int W, const einx_conv_desc* d, float* out,
                    void* stream);

/* The first two layers of a network with a thin first layer as ONE launch (round 6): SuperPointv1's conv1a (1 -> 64, 3x3, ReLU) and conv1b
 * (64 -> 64, 3x3, ReLU, MaxPool 2x2), superpoint_extractor.py:388-390 -- the first layer's output (761 MB at B = 32) is
 * recomputed per tile on the matrix cores and never touches HBM.  Bit-identical to einx_conv_block(d0) followed by
 * einx_conv_block(d1).  in / Hs / Ws / h0 / w0 / H / W: as einx_conv_block for the FIRST layer; out: the second layer's output.
 * einx_conv_first_two_fused_ok: 1 when the pair of layers and the launch size are what the kernel covers AND the one launch is the
 * faster form (64-channel 3x3 layers on ONE input channel, a launch of at least eight rounds of workgroups) -- what einx_extract
 * uses; 2 when the kernel covers the pair but the two launches are faster (5 input channels: the event voxel grid of the bench shape;
 * einx_conv_first_two_fused still takes it); 0 otherwise: run the two layers one by one. */
int einx_conv_first_two_fused_ok(const einx_conv_desc* d0, const einx_conv_desc* d1, int B, int H, int W);
int einx_conv_first_two_fused(const float* in, int B, int Hs, int Ws, int h0, int w0, int H, int W, const einx_conv_desc* d0,
                              const einx_conv_desc* d1, float* out, void* stream);

/* name of the kernel instantiation the calling thread's last einx_conv_block launched, e.g.
 * "conv_block_kernel<3,8,32,2,4,1,2,8,true,true>" (tile shape, wave layout, chunk, pool, reload path): provenance for
 * profiles and bench lines, so that a reported kernel name cannot go stale against the dispatcher */
const char* einx_conv_last_kernel(void);

/* name of the instantiation einx_conv_block WOULD launch for a layer (cin, cout, ks, pool) and a call (B, Hs, Ws, h0, w0, H, W):
 * the dispatcher's own selection code without the launch, the same strings as einx_conv_last_kernel.  Host only: no device
 * pointer, no HIP call, usable without a GPU (the tests' coverage table of instantiations is checked with it).  NULL for
 * arguments einx_conv_block refuses.  The string belongs to the calling thread and holds until its next call.
 * (einx_conv_first_two_fused_ok stays the query for the fused first pair.) */
const char* einx_conv_plan(int cin, int cout, int ks, int pool, int B, int Hs, int Ws, int h0, int w0, int H, int W);

/* Opt-in binary16 convolutions on v_mfma_f32_32x32x16_f16 (no reference counterpart beyond its autocast training).
 * The same block as einx_conv_block for layers with cin % 8 == 0 and no padding fold, under another arithmetic contract: every input
 * activation and every weight element is rounded to IEEE binary16 (nearest even, overflow to infinity: tensor.half()), the products
 * are exact in fp32 and summed in fp32 in an unspecified order, and bias / ReLU / BN affine / 2x2 max are einx_conv_block's fp32
 * epilogue.  Input and output stay fp32 NCHW.  Results follow this contract, NOT the fp32 forward.
 * einx_conv_weight_elems_f16: binary16 elements (2 bytes each) of the weight image; 0 for arguments outside ks {1,3}, cin, cout > 0.
 * einx_conv_repack_f16: OIHW fp32 -> the image [cout tile of 64][chunk][64][tap][channels of the chunk], zero-filled past cin /
 * cout, each element rounded once; runs on `stream`. */
size_t einx_conv_weight_elems_f16(int cin, int cout, int ks);
int einx_conv_repack_f16(const float* w_oihw, int cin, int cout, int ks, void* w_f16, void* stream);

typedef struct einx_conv_desc_f16 {
  size_t struct_size;    /* sizeof(einx_conv_desc_f16) of the caller's header (checked) */
  const void* w_f16;     /* from einx_conv_repack_f16 */
  const float* bias;     /* [cout] or NULL */
  const float* scale;    /* [cout] or NULL, as einx_conv_desc */
  const float* shift;    /* [cout] or NULL */
  int32_t cin, cout, ks; /* ks in {1,3}; cin % 8 == 0 */
  int32_t relu;
  int32_t pool;          /* 3x3 only; H, W must be even */
} einx_conv_desc_f16;

/* in [B,cin,H,W] -> out [B,cout,H,W] or [B,cout,H/2,W/2] when pool.  Refused by name (einx_last_error): cin % 8 != 0, ks outside
 * {1,3}, pooling with odd H or W (or on a 1x1 layer), null pointers, a wrong struct_size, tensors of 2^30 elements per image.
 * No allocation, no atomics, no host synchronisation: capturable. */
int einx_conv_block_f16(const float* in, int B, int H, int W, const einx_conv_desc_f16* d, float* out, void* stream);
/* the instantiation einx_conv_block_f16 WOULD launch / the calling thread's last call launched, e.g. "conv_f16_kernel<3,8,32,16,true>"
 * (KS, tile rows, tile columns, channels per LDS round, pool).  einx_conv_f16_plan is host only (usable without a GPU) and returns
 * NULL for what the entry refuses; these names never appear in einx_conv_plan. */
const char* einx_conv_f16_plan(int cin, int cout, int ks, int pool, int B, int H, int W);
const char* einx_conv_f16_last_kernel(void);

/* x /= divisor in place (SuperPointv1.forward `image /= 255.0`, superpoint_extractor.py:372) */
int einx_div_inplace(float* x, size_t n, float divisor, void* stream);

/* SuperPointv1.forward's input handling for RGB and / or non-contiguous images (superpoint_extractor.py:372-376):
 *   image /= divisor in place on the caller's [B,C,H,W] tensor THROUGH ITS ELEMENT STRIDES (the caller sees the scaled tensor
 *   afterwards, as with the reference), and the network's contiguous [B,1,H,W] input written to `gray`:
 *   C == 1: the scaled value; C == 3: kornia.color.rgb_to_grayscale (kornia 0.7.1) = (0.299 r + 0.587 g) + 0.114 b in fp32,
 *   every product and sum rounded separately.  Overlapping strides (expanded tensors) are the caller's problem, as in torch. */
int einx_image_prepare(float* image, int B, int C, int H, int W, long long stride_b, long long stride_c, long long stride_h,
                       long long stride_w, float divisor, float* gray, void* stream);

/* ------------------------------------------------------------------------------------------
 * Detector head post-processing  (K3, K4, K5)
 * ---------------------------------------------------------------------------------------- */

/* logits_to_prob + depth_to_space + score[~dilate3x3(mask)] = 0 + remove_border_points
 *   core/modules/utils/detector_util.py:18-77,138-164,
 *   core/modules/event_extractors/EventExtractors.py:544-550,561-562
 * logits [B,C,hc,wc], C in {65,1}.  prob [B,C,hc,wc] (C==1: written with the mask/border zeros,
 * because the reference's score aliases probability there).  score [B,Hp,Wp], Hp=hc*cell.
 * mask: uint8 [B,H,W] (bool) or NULL; (h0,w0) = top/left padding of the padded map; dilate:
 * apply the 3x3 dilation (event extractors) or use the mask as is (image extractors).
 * The reference's Padder (core/modules/utils/util.py:17-32) pads a bool mask with zeros and a mask of any other dtype by
 * repeating its edge pixels.  einx_score_map is the bool rule; einx_score_map_pad takes the rule as `mask_pad`, for a host whose
 * bytes stand for the non-zero pixels of a mask that was not bool (the same call otherwise; EINX_ERR_ARG for another value). */
#define EINX_MASK_PAD_ZERO 0
#define EINX_MASK_PAD_REPLICATE 1
int einx_score_map(const float* logits, int B, int C, int hc, int wc, const uint8_t* mask, int H, int W, int h0, int w0,
                   int dilate, int border, float* prob, float* score, void* stream);
int einx_score_map_pad(const float* logits, int B, int C, int hc, int wc, const uint8_t* mask, int mask_pad, int H, int W, int h0,
                       int w0, int dilate, int border, float* prob, float* score, void* stream);

/* remove_border_points alone, in place on [B,Hp,Wp] (detector_util.py:138-164) */
int einx_remove_border(float* score, int B, int Hp, int Wp, int border, void* stream);

/* get_dense_positions (core/modules/utils/detector_util.py:504-519) for an unpadded score map
 * [B,1,H,W]: out [B,H*W,3] = (y+0.5, x+0.5, score) ("yx") or (x+0.5, y+0.5, score) ("xy") */
int einx_dense_positions(const float* score, int B, int H, int W, int ordering_xy, float* out, void* stream);

typedef struct einx_detect_params {
  int32_t B, Hp, Wp;     /* padded map */
  int32_t H, W, h0, w0;  /* unpadded size and top/left padding (Padder) */
  int32_t radius;        /* nms_radius (0 = no NMS) */
  int32_t top_k;         /* detection_top_k (0 = none) */
  float det_thr;         /* detection_threshold */
  int32_t ordering_xy;   /* 0: (y,x,p)  1: (x,y,p) */
  int32_t cap;           /* rows available per image in positions/indices */
  int32_t nms_iters;     /* suppression passes enqueued (>= 1); see not_converged */
} einx_detect_params;

size_t einx_detect_ws_bytes(const einx_detect_params* p);

/* prob_map_to_points_map (fast_nms fix-point + top-k quantile threshold) +
 * prob_map_to_positions_with_prob + Padder.unpad_positions + filter_sparse_feats
 *   core/modules/utils/detector_util.py:80-135,243-337,451-484, core/modules/utils/util.py:52-66,
 *   core/modules/event_extractors/EventExtractors.py:496-515
 * score     [B,Hp,Wp]  input (already masked / border-zeroed), not modified
 * nms_out   [B,H,W]    thresholded NMS map cropped to the unpadded window, or NULL
 * positions [B,cap,3]  (y+.5-h0, x+.5-w0, p) in raster order
 * indices   [B,cap]    int32 flat index y*Wp+x in the padded map
 * counts    [B]        int32 number of keypoints (may exceed cap: only cap rows are written)
 * thr       [B]        threshold used
 * not_converged [B]    int32, nonzero if the fix-point needed more than nms_iters passes (caller re-runs with more
 *                      passes).  Radius 4 (every shipped configuration) never raises it: images that are still changing
 *                      after the nms_iters wide passes are completed on the device by a per-image finisher
 *                      (nms4_finish_kernel), e.g. quantised maps that need 14-25 passes */
int einx_detect(const float* score, const einx_detect_params* p, void* ws, float* nms_out, float* positions, int32_t* indices,
                int32_t* counts, float* thr, int32_t* not_converged, void* stream);

/* ------------------------------------------------------------------------------------------
 * Descriptor heads post-processing  (K6, K10)
 * ---------------------------------------------------------------------------------------- */

/* sparsify_low_resolution_descriptors (bilinear=1; descriptor_util.py:74-128) or
 * sparsify_full_resolution_descriptors (bilinear=0; descriptor_util.py:50-71), then
 * F.normalize * scale.  raw [B,D,hc,wc], or with channels_last=1 (bilinear only) the [B,hc*wc,D]
 * copy written by einx_normalize_map; indices/counts from einx_detect; out [B,cap,D]. */
int einx_desc_sample(const float* raw, int B, int D, int hc, int wc, int Hp, int Wp, int bilinear, int channels_last,
                     const int32_t* indices, const int32_t* counts, int cap, float scale, float* out, void* stream);

/* sparsify_low_resolution_descriptors at GIVEN float positions (descriptor_util.py:74-128: grid_sample bilinear,
 * align_corners=False, zero padding outside the map, then F.normalize * scale) -- for projected, warped or refined points.
 * positions [B,cap,pos_stride >= 2] in the padded frame (pixel centres at .5), rows (y, x, ...) or with ordering_xy (x, y, ...);
 * counts [B] rows are read per image (clamped to cap); out [B,cap,D].  Any coordinate is accepted: the map coordinate is tested
 * as a float before it is converted, a position whose four taps lie outside the map (or a non-finite one) gives a zero row.  A
 * position (y + 0.5, x + 0.5) gives einx_desc_sample's row of index y * Wp + x bit for bit.  No workspace. */
int einx_desc_sample_pos(const float* raw, int B, int D, int hc, int wc, int Hp, int Wp, int channels_last, const float* positions,
                         int pos_stride, int ordering_xy, const int32_t* counts, int cap, float scale, float* out, void* stream);

/* Opt-in sub-pixel keypoints (a departure from the reference, whose keypoints are pixel centres).  For each of
 * the first counts[b] keypoints of einx_detect / einx_extract: (y, x) from indices; per axis, with c the score at the peak and
 * (l, r) its two neighbours along the axis on the padded score map [B,Hp,Wp], the offset is 0 when a neighbour is outside the map
 * or !(l < c && r < c), otherwise, in fp32 and in this order,
 *   a = l - c; b = r - c; den = a + b; num = l - r; delta = (0.5f * num) / den      (IEEE division)
 * clamped to +-(0.5 - 2^-10), which keeps floor() of the refined position on the detected pixel for map sides <= 8192 (larger
 * maps are refused).  positions [B,cap,3]: columns 0 and 1 become ((y + 0.5f + dy) - h0, (x + 0.5f + dx) - w0) in the ordering;
 * column 2 (the score at the integer peak) and indices are not touched.
 * bilinear = 1 (cell-8 networks): the keypoint's row of sparse_desc [B,cap,D] is resampled at the refined position, from raw
 * [B,D,hc,wc] or with channels_last = 1 its [B,hc*wc,D] copy, like einx_desc_sample_pos; with both offsets 0 the row equals
 * einx_desc_sample's bit for bit.  bilinear = 0 (cell-1 networks): positions only; raw, D, hc, wc, scale are ignored and
 * sparse_desc may be NULL.  One launch, no workspace, no host synchronisation: capturable. */
int einx_refine_keypoints(const float* score, int B, int Hp, int Wp, int H, int W, int h0, int w0, int ordering_xy,
                          const int32_t* indices, const int32_t* counts, int cap, float* positions, const float* raw, int D, int hc,
                          int wc, int bilinear, int channels_last, float scale, float* sparse_desc, void* stream);

/* normalize_descriptors over channels of a dense map (descriptor_util.py:21-28). raw/out [B,D,P].
 * raw_cl: optional [B,P,D] channels-last copy of `raw` (un-normalised) for einx_desc_sample, or NULL. */
int einx_normalize_map(const float* raw, int B, int D, int P, float scale, float* out, float* raw_cl, void* stream);

/* F.normalize(x, dim=1) * scale on a row-major [R,C] matrix: the random padding descriptors of the
 * trainable matcher branch (core/modules/Matchers.py:114-131) */
int einx_normalize_rows(const float* x, int R, int C, float scale, float* out, void* stream);

/* random padding keypoints of the same branch (Matchers.py:80-91): u [R,2] uniform draws ->
 * out [R,3] = (u0*size0, u1*size1, 0) */
int einx_random_positions(const float* u, int R, float size0, float size1, float* out, void* stream);

/* upsample_descriptors: bilinear resize to (Hp,Wp) + normalize, written cropped to the
 * unpadded window [B,D,H,W] (descriptor_util.py:131-138 + Padder.unpad util.py:34-50).
 * ws: device scratch of at least einx_upsample_ws_bytes(B,H,W) bytes (the per-pixel norms between the two
 * kernels); required when W <= 384 and wc <= 63 (every shipped geometry), unused (may be NULL) otherwise. */
size_t einx_upsample_ws_bytes(int B, int H, int W);
int einx_upsample_normalize(const float* raw, int B, int D, int hc, int wc, int Hp, int Wp, int h0, int w0, int H, int W,
                            float scale, float* out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mutual-nearest-neighbour matcher  (K7)   core/modules/matchers/MNN.py:43-140
 * desc0 [B,cap0,D], desc1 [B,cap1,D]; n[b], m[b] device int32 counts (<= cap).
 * matches0 [B,cap0] int64 (-1 = none), matches1 [B,cap1]; scores fp32 0/1.
 * la: optional [B,cap0+1,cap1+1] log_assignment written at [b, :n+1, :m+1] with row pitch
 * (cap1+1), or NULL.  ws: einx_mnn_ws_bytes.
 * ---------------------------------------------------------------------------------------- */
size_t einx_mnn_ws_bytes(int B, int cap0, int cap1);
int einx_mnn(const float* desc0, const int32_t* n, int cap0, const float* desc1, const int32_t* m, int cap1, int B, int D,
             void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, void* stream);
/* einx_mnn followed by einx_gather_matches (below) with the mutual check and the matched-keypoint compaction as ONE launch
 * (MNN.py:98-129: the matches and the per-pair matched_kpts lists); same outputs as the two calls. */
int einx_mnn_gather(const float* desc0, const int32_t* n, int cap0, const float* desc1, const int32_t* m, int cap1, int B, int D,
                    void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, const float* kpts0,
                    const float* kpts1, int cols, float* mk0, float* mk1, int32_t* nmatch, void* stream);
/* the same with find_nn's optional thresholds (MNN.py:12-22): dist = 2*(1-sim) of the best / second-best
 * neighbour per row (per column for matches1); a match is kept when dist0 <= ratio_sq*dist1 (use_ratio) and
 * dist0 <= dist_sq (use_dist); the mutual check (:25-32) runs on the masked matches.  ratio_sq / dist_sq are the
 * squared thresholds rounded to fp32 (what torch computes for `tensor <= python_float`).  Rows / columns with a
 * single candidate have no second neighbour: the ratio test passes there (torch.topk(2) raises; the Python
 * wrapper raises the same error when it knows the counts). */
int einx_mnn_thresh(const float* desc0, const int32_t* n, int cap0, const float* desc1, const int32_t* m, int cap1, int B, int D,
                    int use_ratio, float ratio_sq, int use_dist, float dist_sq, void* ws, int64_t* matches0, int64_t* matches1,
                    float* scores0, float* scores1, float* la, void* stream);

/* similarity = einsum("bnd,bmd->bnm") (MNN.py:88), returned by the reference's un-frozen Matcher
 * branch (Matchers.py:204-222).  sim [B,cap0,cap1]; entries outside [n[b], m[b]] are zero. */
int einx_similarity(const float* desc0, const int32_t* n, int cap0, const float* desc1, const int32_t* m, int cap1, int B, int D,
                    float* sim, void* stream);

/* matched keypoint gather in ascending keypoint-0 order (MNN.py:119-129, lightglue.py:690-698)
 * kpts0 [B,cap0,3], kpts1 [B,cap1,3]; cols = 3 (MNN) or 2 (LightGlue);
 * out0/out1 [B,cap0,cols]; nmatch [B] int32. */
int einx_gather_matches(const float* kpts0, const float* kpts1, const int64_t* matches0, const int32_t* n, int cap0, int cap1,
                        int B, int cols, float* out0, float* out1, int32_t* nmatch, void* stream);

/* Packs the first counts[b] rows of two padded [B,cap,width] arrays (the matched keypoints of
 * einx_gather_matches) into two flat [sum(counts),width] arrays, pair after pair, so that the
 * per-pair lists the reference returns (Matchers.py:177-201) are views cut by one split call.
 * dst0/dst1 need room for B*cap rows. */
int einx_compact_rows(const float* src0, const float* src1, const int32_t* counts, int B, int cap, int width, float* dst0, float* dst1,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * LightGlue  (K8, K9)   core/modules/matchers/lightglue.py:522-716
 * ---------------------------------------------------------------------------------------- */
/* y[M,N] (+)= x[M,K] w[N,K]^T + bias[N]   (torch.nn.functional.linear; also used at load time to
 * fold LightGlue's out_proj / to_out into the following FFN Linear).  accumulate != 0: y += ... */
int einx_linear(const float* x, int M, int K, const float* w, const float* bias, int N, float* y, int accumulate, void* stream);

/* Wo / Wco may be NULL: the message projection has then been folded into sf0_w / cf0_w
 * (x' = ffn(cat[x, context]) with W0' = [W0a | W0b Wo], b0' = b0 + W0b bo). */
typedef struct einx_lg_layer {
  /* SelfBlock (:240-272) */
  const float *Wqkv, *bqkv, *Wo, *bo, *sf0_w, *sf0_b, *sln_g, *sln_b, *sf3_w, *sf3_b;
  /* CrossBlock (:275-330) */
  const float *Wqk, *bqk, *Wv, *bv, *Wco, *bco, *cf0_w, *cf0_b, *cln_g, *cln_b, *cf3_w, *cf3_b;
  /* optional (NULL: two launches): the rows of Wqk followed by the rows of Wv as ONE [2d, d] matrix, and [bqk | bv] -- to_qk and
   * to_v then run as one launch (d = 256 with 64-wide heads; same results) */
  const float *Wqk_v, *bqk_v;
  /* optional (NULL unless einx_lightglue_mp runs with EINX_LG_LIN_F16): the IEEE binary16 image (round to nearest even) of the nine
   * Linear weights above, same shapes, and of Wqk_v.  Wo / Wco must then be given (no fold): the weights are rounded as written. */
  const uint16_t *Wqkv_h, *Wo_h, *sf0_h, *sf3_h, *Wqk_h, *Wv_h, *Wco_h, *cf0_h, *cf3_h, *Wqk_v_h;
} einx_lg_layer;

typedef struct einx_lg_weights {
  size_t struct_size; /* sizeof(einx_lg_weights) of the caller's header (checked) */
  size_t layer_size;  /* sizeof(einx_lg_layer): the stride of `layers` (checked) */
  const float* in_w; /* input_proj [d,input_dim] or NULL (Identity) */
  const float* in_b;
  const float* Wr;   /* posenc.Wr [head_dim/2,2] */
  const float* proj_w; /* log_assignment[last].final_proj [d,d] */
  const float* proj_b;
  const float* match_w; /* log_assignment[last].matchability [1,d] */
  const float* match_b;
  int32_t n_layers, heads, d, input_dim;
  float filter_threshold;
  const einx_lg_layer* layers; /* host array of n_layers */
} einx_lg_weights;

/* normalize_keypoints (lightglue.py:137-148): kpts [rows,cols>=2] -> out [rows,out_cols>=2] with
 * out[:, :2] = (kpt - (h,w)/2) / (max(h,w)/2) and zeros in further columns.  The batched (B>1)
 * LightGlue call returns matched keypoints in these coordinates (lightglue.py:677-687). */
int einx_normalize_keypoints(const float* kpts, int rows, int cols, float h, float w, float* out, int out_cols, void* stream);

/* Model widths (lightglue.py:456-461): d = descriptor_dim = heads x head_dim, head_dim any multiple of 4 up to 256 (the attention
 * kernel is instantiated for 32 / 64 / 128 / 256; other widths run the next larger one on zero-padded heads; anything else is refused);
 * Wr is [head_dim/2, 2].  d = 256 with 4 heads of 64 -- every EI-Nexus configuration -- runs kernels instantiated for those widths.
 * einx_lg_ws_bytes assumes 64-wide heads (heads = d / 64); 0 = unsupported widths. */
size_t einx_lg_ws_bytes(int B, int cap0, int cap1, int d, int input_dim);
size_t einx_lg_ws_bytes_heads(int B, int cap0, int cap1, int d, int heads, int input_dim);
/* kpts [B,cap,3] (first two columns used), desc [B,cap,input_dim], counts device int32.
 * size0/size1: image sizes (H,W) used by normalize_keypoints (:137-148).
 * outputs as einx_mnn; scores are exp(max log-assignment) for mutual matches (:402-418);
 * ref0/ref1: optional ref_descriptors, or NULL.  ref_layers 0/1: [B,cap,d], the last layer
 * (eval, lightglue.py:626-629); ref_layers == n_layers: [B,n_layers,cap,d], every layer
 * (what the reference stacks when self.training, lightglue.py:626-629,709-710).
 * Schedule (same results either way): with cap0 == cap1 the two sides are stacked in the workspace and every layer is one
 * launch over 2B entries; grids of fewer than 256 128x128 tiles (up to 7 pairs) run their linears on 64x64 tiles.
 * ws: device scratch of einx_lg_ws_bytes_heads(B, cap0, cap1, d, heads, input_dim) bytes; rows of the outputs past an entry's
 * count are left unwritten. */
int einx_lightglue(const einx_lg_weights* w, const float* kpts0, const float* desc0, const int32_t* n, int cap0, const float* kpts1,
                   const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1, float w1, void* ws,
                   int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, float* ref0, float* ref1,
                   int ref_layers, void* stream);

/* Early stopping: per-pair adaptive depth.  LightGlue trains a token_confidence head per non-final layer and a
 * log_assignment head per layer so that an easy pair can leave after a few layers; the reference carries them and
 * `depth_confidence`, but its forward has the branch commented out (lightglue.py:606-636) and always runs every layer.  This
 * entry point runs the branch.  It is a departure from the reference's results and therefore something the caller opts into;
 * einx_lightglue is unchanged.
 * After layer i < n_layers - 1, for every pair still running: c = sigmoid(token_w . x + token_b) of its n + m rows in float32,
 * below = #{c < thr[i]}, thr[i] = float32(clip(0.8 + 0.1 exp(-4 i / n_layers), 0, 1)); the pair stops iff
 * 1.0f - float(below) / float(n + m) > depth_confidence.  A pair that stops after layer i has stop = i + 1: its rows are not
 * touched again, and its assignment comes from heads[i] (final_proj, matchability) applied to them.  A pair that never stops has
 * stop = n_layers and exactly einx_lightglue's outputs; a pair with n == 0 or m == 0 has stop = 0 and einx_lightglue's outputs.
 * Pairs are independent of each other.  ref0 / ref1 [B,cap,d] hold the descriptors the head read.
 * heads: HOST array of n_layers entries (token_* unused in the last); head_size = sizeof(einx_lg_head), checked.  w->proj_* /
 * w->match_* are not read.  stop: device int32 [B].  n, m are never written: the layers run on copies in the workspace.
 * One more launch per non-final layer (integer counting, no float atomics: deterministic), no host synchronisation, no
 * allocation: capturable.  ws: einx_lightglue_early_stop_ws_bytes(...) bytes (0 = unsupported widths, or more than 32 layers). */
typedef struct einx_lg_head {
  const float *proj_w, *proj_b;   /* log_assignment[i].final_proj [d,d], [d] */
  const float *match_w, *match_b; /* log_assignment[i].matchability [1,d], [1] */
  const float *token_w, *token_b; /* token_confidence[i].token[0] [1,d], [1]; NULL in the last entry */
} einx_lg_head;
size_t einx_lightglue_early_stop_ws_bytes(int B, int cap0, int cap1, int d, int heads, int input_dim, int n_layers);
int einx_lightglue_early_stop(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                              const float* kpts0, const float* desc0, const int32_t* n, int cap0, const float* kpts1,
                              const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1, float w1, void* ws,
                              int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, float* ref0,
                              float* ref1, int32_t* stop, void* stream);

/* Point pruning: per-pair, per-side adaptive width, with or without early stopping.  The reference carries
 * `width_confidence`, get_pruning_mask and pruning_min_kpts, but the branch that calls them is commented out (lightglue.py:608-617,
 * 637-652, 658-670).  This entry point runs it; einx_lightglue and einx_lightglue_early_stop are unchanged.
 * After layer i < n_layers - 1, for every pair still running (after that layer's stop decision when depth_confidence > 0), each
 * side with more than min_kpts rows keeps the rows with sigmoid(match_w . x + match_b) > float(1.0 - width_confidence) -- or, with
 * depth_confidence > 0 only, sigmoid(token_w . x + token_b) <= thr[i] -- compacted to the front in their order; prune[ind[kept]]
 * grows by one.  The stop ratio's denominator stays the caller's n + m.  A side left without rows finishes its pair: no matches,
 * and stop = i + 1 when depth_confidence > 0.  depth_confidence <= 0: no stop decision, the last head, token_* not read.
 * Outputs in ORIGINAL indexing: matches0/1, scores0/1 (pruned points: -1 / 0), prune0 [B,cap0] / prune1 [B,cap1] float32 (1 +
 * the steps survived; 0 in the padding).  kept0 [B,cap0] / kept1 [B,cap1] int64: the survivors' original indices in compacted
 * order, -1 behind them; live [2B] int32: survivors of side 0 (entries 0..B-1) and side 1 (B..2B-1).  ref0 / ref1 [B,cap,d]: the
 * survivors' rows in that order (rows past live are not written).  la must be NULL (no log_assignment).  stop: device int32 [B]
 * or NULL.  width_confidence in (0, 1].  No host synchronisation, no allocation, no atomics: deterministic and capturable.
 * ws: einx_lightglue_adaptive_ws_bytes(...) bytes (0 = unsupported widths, or more than 32 layers). */
size_t einx_lightglue_adaptive_ws_bytes(int B, int cap0, int cap1, int d, int heads, int input_dim, int n_layers);
int einx_lightglue_adaptive(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                            double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                            const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1,
                            float w1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la,
                            float* ref0, float* ref1, int32_t* stop, float* prune0, float* prune1, int64_t* kept0, int64_t* kept1,
                            int32_t* live, void* stream);

/* LightGlue's `flash: True` (lightglue.py:206-230, :293-314): the three runs above with every attention, self and
 * cross, in half precision on the matrix cores.  Per (pair, head): q, k, v are rounded to IEEE binary16 (round to nearest even,
 * overflow to infinity; q and k after the rotary step, the cross block's qk unscaled), softmax(q . k^T / sqrt(head_dim)) v is
 * accumulated in fp32 (probabilities rounded to binary16 before the second product), and the context is rounded to binary16 and
 * widened to fp32.  Projections, FFN, heads and every decision stay fp32.  The entries above are unchanged and never take this path.
 * The argument list is einx_lightglue_adaptive's plus ref_layers (as in einx_lightglue):
 *   width_confidence > 0: einx_lightglue_adaptive's run and rules (la NULL, ref_layers 0 / 1);
 *   else depth_confidence > 0: einx_lightglue_early_stop's (stop required, ref_layers 0 / 1; prune0 .. live unread);
 *   else: einx_lightglue's (heads, stop, prune0 .. live unread and may be NULL).
 * ws: einx_lightglue_flash_ws_bytes(...) bytes = einx_lightglue_adaptive_ws_bytes(...): the kernel needs no region of its own (for
 * a layer count that only the plain run takes, more than 32: einx_lg_ws_bytes_heads(...); 0 = unsupported widths). */
size_t einx_lightglue_flash_ws_bytes(int B, int cap0, int cap1, int d, int heads, int input_dim, int n_layers);
int einx_lightglue_flash(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                         double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                         const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1,
                         float w1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la,
                         float* ref0, float* ref1, int ref_layers, int32_t* stop, float* prune0, float* prune1, int64_t* kept0,
                         int64_t* kept1, int32_t* live, void* stream);

/* The attention of einx_lightglue_flash alone (a test hook).  Q / K / V: fp32 [B,cap,ld], head h in columns h dh .. (h + 1) dh - 1
 * (ld >= heads * dh, a multiple of 4; dh a multiple of 4, at most 256); O: fp32 [B,capq,heads * dh].  Entry b: its first
 * min(nq[b], capq) query rows over the first min(nk[bk], capk) keys of entry bk = (b + kv_shift) mod B; rows past nq[b], and every
 * row of an entry without queries or keys, are not written.  Every value written is binary16-representable. */
int einx_lg_attention_f16(const float* Q, const float* K, const float* V, float* O, const int32_t* nq, const int32_t* nk, int capq, int capk,
                          int B, int heads, int dh, int ld, int kv_shift, void* stream);

/* LightGlue's `mp: True` (lightglue.py:430; upstream's torch.autocast(enabled=conf.mp), which the reference's forward no longer
 * has): the runs above with the precision modes as bits of `mode`.
 *   EINX_LG_LIN_F16:  the nine nn.Linear of every transformer layer (SelfBlock Wqkv, out_proj, ffn.0, ffn.3; CrossBlock to_qk, to_v,
 *                     to_out, ffn.0, ffn.3) on the f16 matrix-core instruction: every input element and every weight element
 *                     rounded to IEEE binary16 (round to nearest even, overflow to infinity), exact products accumulated in fp32
 *                     in an unspecified order, fp32 bias added in fp32, fp32 result (NOT rounded to binary16).  Operands whose
 *                     rounded magnitude lies below 2^-14 are outside the contract.  Needs the *_h images of einx_lg_layer and
 *                     unfolded Wo / Wco.  input_proj, rotary, residual, LayerNorm, GELU, the heads and every decision stay fp32.
 *   EINX_LG_ATTN_F16: the attention of einx_lightglue_flash.
 * mode 0 = the fp32 entries, EINX_LG_ATTN_F16 alone = einx_lightglue_flash.  Single pairs run the wide f16 GEMM kernel (no
 * small-grid twin).  Arguments and rules otherwise as einx_lightglue_flash; ws: einx_lightglue_mp_ws_bytes(...) bytes (the same
 * carve).  No allocation, no atomics, no host synchronisation: capturable. */
#define EINX_LG_ATTN_F16 1
#define EINX_LG_LIN_F16 2
size_t einx_lightglue_mp_ws_bytes(int B, int cap0, int cap1, int d, int heads, int input_dim, int n_layers);
int einx_lightglue_mp(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                      double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                      const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1, float w1,
                      void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, float* ref0,
                      float* ref1, int ref_layers, int32_t* stop, float* prune0, float* prune1, int64_t* kept0, int64_t* kept1,
                      int32_t* live, int mode, void* stream);

/* The linear of EINX_LG_LIN_F16 alone (a test hook).  X: fp32 [B,cap,K], or with X2 the concatenation of X [B,cap,Ksplit] and X2
 * [B,cap,K - Ksplit] (Ksplit a multiple of 32); W16: binary16 [N,K]; bias fp32 [N]; Y fp32 rows of stride ldy >= N.  epi 0:
 * Y = RN16(X) W16^T + bias; epi 1: Y += the same (resid: NULL or Y, the residual is read in place; with epi 0 a non-NULL resid is refused).  The rotary
 * epilogues of the Wqkv projection are reached through a forward only.  Entry b: its first
 * min(cnt[b], cap) rows (cnt NULL: cap rows); rows past the count and columns past N are not written.  K a multiple of 4. */
int einx_lg_linear_f16(const float* X, const float* X2, int Ksplit, int K, const uint16_t* W16, const float* bias, int N, float* Y, int ldy,
                       const float* resid, const int32_t* cnt, int cap, int B, int epi, void* stream);

/* Assignment NLL of ONE MatchAssignment head (lightglue.py:66-133 NLLLoss / weight_loss, :751-769 LightGlue.loss in eval mode): the
 * sums behind nll_pos / nll_neg / row_norm, without a log_assignment matrix or any other B x n x m buffer.
 * proj_w [d,d], proj_b [d]: the head's final_proj; match_w [d], match_b [1]: its matchability; d a multiple of 4.
 * x0 [B,cap0,d], x1 [B,cap1,d]: the descriptors the head is applied to (ref_descriptors); n, m: device int32 counts, clamped to
 * [0, cap].  gt_matches0 [B,cap0], gt_matches1 [B,cap1] int64: -1 selects the dustbin entries (-2 and matches weigh nothing).
 * The positives come in ONE of two forms (the other NULL): pos0 [B,cap0] int32, the column of row i's positive or -1 (what
 * einx_gt_label writes), or a dense 0/1 byte matrix read at assignment[b*as_b + i*as_i + j*as_j] (strides in bytes = elements).
 * The two give the same bits when the matrix is the scatter of pos0.
 * out [B,8] float64 per pair: S_pos = sum w la[i,j], num_pos = sum w, S_neg0 = sum over gt_matches0 == -1 of la[i,m], num_neg0,
 * S_neg1 = sum over gt_matches1 == -1 of la[n,j], num_neg1, sum_i sum_{j<=m} exp(la[i,j]) (row_norm x n), n.  A pair with
 * n == 0 or m == 0 gets eight zeros.  Deterministic (no float atomics, fixed summation order), no host synchronisation, no
 * allocation: capturable.  ws: einx_lg_assign_nll_ws_bytes(B, cap0, cap1, d) bytes (0 = bad shape). */
size_t einx_lg_assign_nll_ws_bytes(int B, int cap0, int cap1, int d);
int einx_lg_assign_nll(const float* proj_w, const float* proj_b, const float* match_w, const float* match_b, int d, const float* x0,
                       const int32_t* n, int cap0, const float* x1, const int32_t* m, int cap1, int B, const int64_t* gt_matches0,
                       const int64_t* gt_matches1, const int32_t* pos0, const unsigned char* assignment, int64_t as_b, int64_t as_i,
                       int64_t as_j, void* ws, double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Event representation (the step before the path)
 * events of B samples are concatenated; offsets_host[B+1] (HOST array) delimits the samples.
 * x, y, p: float32 [N]; t: float64 [N] raw timestamps (normalised inside exactly like
 * datasets/representations.py:8-21).
 * ---------------------------------------------------------------------------------------- */
size_t einx_events_ws_bytes(int B, int H, int W);                                        /* workspace of einx_events_mask */
size_t einx_voxel_ws_bytes(int B, int bins, int H, int W, int64_t total_events);         /* workspace of einx_voxel_grid */
/* events_to_voxel_grid (datasets/representations.py:67-124): grid [B,bins,H,W].  Deterministic: per voxel the contributions
 * are added in the order of the reference's serial path (corner (dx,dy,dt) major, then event order, :94-114), so two calls give
 * the same bits and the un-normalised grid is bit-equal to a sequential restatement.  offsets_host[0] must be 0;
 * ws_bytes >= einx_voxel_ws_bytes(B, bins, H, W, offsets_host[B]) is checked. */
int einx_voxel_grid(const float* x, const float* y, const double* t, const float* p, const int64_t* offsets_host, int B, int bins, int H,
                    int W, int normalize, float* grid, void* ws, size_t ws_bytes, void* stream);
/* draw_events_accumulation_image(...) > 0 (datasets/visualize.py:23-50,
 * test_events-image_same-time.py:137): mask uint8 [B,H,W] */
int einx_events_mask(const float* x, const float* y, const int64_t* offsets_host, int B, int H, int W, void* ws, uint8_t* mask,
                     void* stream);

/* The other three values of the reference's `representation_type` (datasets/MVSEC.py:706-718, datasets/EC.py:236-248), DESIGN.md 8d.
 * Same packed inputs as einx_voxel_grid; out: [B,bins,H,W] fp32.  Common rules: tn = (t - t[first]) / ((t[last] - t[first]) + 1e-8)
 * in float64 per sample (representations.py:8-22); event k is in bin i iff tn >= i * dt && tn <= i * dt + dt (dt = 1.0 / nb, float64,
 * both sides inclusive: for non-decreasing t the reference's two searchsorted calls; for unsorted t this per-event predicate IS
 * the contract); xi = (int)x, yi = (int)y and an event outside the image is dropped (numpy would wrap a negative index or raise).
 * A sample without events gives zeros (distance map: 8192.0).  Integer atomics only: two calls give the same bits.  The calls
 * enqueue on `stream`, keep no library-owned state (the offsets travel as kernel arguments) and can be captured.
 * offsets_host[0] must be 0; ws_bytes >= einx_*_ws_bytes(B, bins, H, W, offsets_host[B]) is checked (EINX_ERR_ARG); the size
 * queries return 0 on a shape the op does not take. */
size_t einx_time_surface_ws_bytes(int B, int bins, int H, int W, int64_t total_events);
size_t einx_event_stack_ws_bytes(int B, int bins, int H, int W, int64_t total_events);
size_t einx_distance_map_ws_bytes(int B, int bins, int H, int W, int64_t total_events);
/* events_to_time_surface (datasets/representations.py:26-63): nb = bins / 2 (bins >= 2), channel c = 2 i + (int)p, where numpy's
 * rule wraps -bins <= c < 0 once (p = -1) and any other c outside [0, bins) is dropped; a cell holds (float)tn of the
 * highest-indexed event that hits it (numpy's "last one wins"), 0 where none does. */
int einx_time_surface(const float* x, const float* y, const double* t, const float* p, const int64_t* offsets_host, int B, int bins, int H,
                      int W, float* out, void* ws, size_t ws_bytes, void* stream);
/* events_to_event_stack (datasets/representations.py:178-212): nb = bins, cell[i, yi, xi] += 2 (int)p - 1, summed in int32 and
 * converted once: the reference's sequential float32 sum whenever every partial sum stays within +-2^24. */
int einx_event_stack(const float* x, const float* y, const double* t, const float* p, const int64_t* offsets_host, int B, int bins, int H,
                     int W, float* out, void* ws, size_t ws_bytes, void* stream);
/* events_to_distance_map (datasets/representations.py:216-248): nb = bins; per bin the 3x3-mask chamfer distance of every pixel
 * to the pixels hit by an event of the bin, in 16.16 fixed point with HV = 62587 (0.955), DIAG = 89738 (1.3693):
 * d = min over set pixels of HV (max(|dx|,|dy|) - min(|dx|,|dy|)) + DIAG min(|dx|,|dy|), out = (float)d / 65536; a bin without a
 * pixel gives 8192.0 everywhere.  The written algorithm, not bit parity with cv2.distanceTransform(..., DIST_L2, 3).
 * W <= 1024, H <= 4096. */
int einx_distance_map(const float* x, const float* y, const double* t, const float* p, const int64_t* offsets_host, int B, int bins, int H,
                      int W, float* out, void* ws, size_t ws_bytes, void* stream);
/* name of the instantiation einx_distance_map WOULD launch for [H,W] slices, e.g. "distance_map_kernel<8>" (pixels per lane, from
 * ceil(W / 64): 2, 4, 6, 8, 12 or 16): the op's own selection function without the launch, the names tools/kernel_resources.py
 * prints.  Host only: no HIP call, usable without a GPU (the tests' table of widths is checked with it).  NULL for a shape the op
 * refuses (W > 1024, H > 4096, H <= 0 or W <= 0).  The string is static. */
const char* einx_distance_map_plan(int H, int W);

/* Windowed forms of einx_voxel_grid and einx_events_mask: x / y / p (fp32) and t (fp64) are the device arrays of a
 * WHOLE sequence of stream_len events, uploaded once, and sample b is its events begin_host[b] <= k < end_host[b], in stream order
 * (HOST arrays, int64 [B]).  Windows may overlap, repeat, leave gaps, lie in any order or be empty.  Every rule of the packed op
 * holds for exactly those events as if they had been packed: the time normalisation from the window's own first and last stamp,
 * dropped out-of-image events, the voxel grid's summation order; an empty window gives zeros.  The results are bit-equal to the
 * packed op on the packed slices.
 * Checked (EINX_ERR_ARG): null pointers, the shapes the packed op refuses, 0 <= begin_host[b] <= end_host[b] <= stream_len, fewer
 * than 2^31 events in all windows together, ws_bytes >= the op's *_windows_ws_bytes(..., total_events = sum of end - begin) (which
 * return 0 on the shapes the packed queries refuse and are never smaller than them).
 * Launch properties of the packed op: no allocation, integer atomics only (two calls give the same bits), the stream arrays are
 * only read; begin / end are staged through the pinned ring of the packed forms (one small copy per call).
 * (einx_time_surface / einx_event_stack / einx_distance_map have no windowed form yet: DESIGN.md 8i.) */
size_t einx_events_windows_ws_bytes(int B, int H, int W);
size_t einx_voxel_windows_ws_bytes(int B, int bins, int H, int W, int64_t total_events);
int einx_voxel_grid_windows(const float* x, const float* y, const double* t, const float* p, int64_t stream_len, const int64_t* begin_host,
                            const int64_t* end_host, int B, int bins, int H, int W, int normalize, float* grid, void* ws, size_t ws_bytes,
                            void* stream);
int einx_events_mask_windows(const float* x, const float* y, int64_t stream_len, const int64_t* begin_host, const int64_t* end_host, int B,
                             int H, int W, void* ws, size_t ws_bytes, uint8_t* mask, void* stream);

/* Host-side helper (no kernel, no device access): concatenates the B per-sample event arrays of a batch into the flat
 * x / y / p (fp32) and t (fp64) HOST arrays einx_voxel_grid / einx_events_mask read after an upload, converting element types
 * (C casts: the rounding of numpy's astype), and writes offsets[B + 1].  `threads` host threads share the copy (page-locked
 * destinations make the upload one asynchronous copy per array).  Replaces the per-sample tensor building of
 * datasets/representations.py:67-80 + a Python host's np.concatenate passes. */
enum { EINX_EV_F32 = 0, EINX_EV_F64, EINX_EV_I64, EINX_EV_I32, EINX_EV_I16, EINX_EV_U16, EINX_EV_I8, EINX_EV_U8, EINX_EV_U32, EINX_EV_U64 };
typedef struct einx_event_arrays {
  const void *x, *y, *t, *p;                 /* host arrays of n elements each */
  int32_t x_type, y_type, t_type, p_type;    /* EINX_EV_* */
  int64_t n;
} einx_event_arrays;
int einx_events_pack(const einx_event_arrays* samples, int B, float* x, float* y, double* t, float* p, int64_t* offsets, int threads);

/* ------------------------------------------------------------------------------------------
 * Rectification of raw recordings (csrc/rectify.hip)
 * replaces: datasets/MVSEC_rectify.py (maps, frames, events), datasets/rectify_ec.py (frames, events)
 * All maps are [H,W] fp32 pairs (map_x, map_y) on the device, computed in float64 with every operation rounded as written and
 * stored as float32.  K = (fx, fy, cx, cy), R and P row-major 3x3 (the left 3x3 block of a 3x4 projection matrix), all HOST arrays
 * of doubles.  Every call enqueues on `stream`, allocates nothing, waits for nothing and can be captured; two calls give the same
 * bits.  EINX_ERR_ARG: null pointers, non-positive sizes, H * W >= 2^31, a singular P R, a short workspace.
 * ------------------------------------------------------------------------------------------ */
/* cv.fisheye.initUndistortRectifyMap(K, D, R, P, (W, H), CV_32FC1) (datasets/MVSEC_rectify.py:91-106): destination pixel (u, v) ->
 * source position.  iR = (P R)^-1 (host, double); (X, Y, Wd) = iR (u, v, 1), x = X / Wd, y = Y / Wd, r = sqrt(x x + y y),
 * th = atan(r), thd = th (1 + k1 th^2 + k2 th^4 + k3 th^6 + k4 th^8), s = thd / r (1 where r == 0),
 * map = (fx x s + cx, fy y s + cy); Wd <= 0 gives (-1, -1).  D = (k1, k2, k3, k4). */
int einx_rectify_map_fisheye(const double* K, const double* D, const double* R, const double* P, int H, int W, float* map_x, float* map_y,
                             void* stream);
/* cv.initUndistortRectifyMap(K, D, R, P, (W, H), CV_32FC1); cv.undistort(img, K, D) (datasets/rectify_ec.py:48-50) remaps with
 * the map of R = I, P = K.  x, y as above; r2 = x x + y y, kr = 1 + ((k3 r2 + k2) r2 + k1) r2,
 * xd = x kr + 2 p1 x y + p2 (r2 + 2 x x), yd = y kr + p1 (r2 + 2 y y) + 2 p2 x y, map = (fx xd + cx, fy yd + cy).
 * D = (k1, k2, p1, p2, k3): the order of EC's calib.txt. */
int einx_rectify_map_radtan(const double* K, const double* D, const double* R, const double* P, int H, int W, float* map_x, float* map_y,
                            void* stream);
/* cv.undistortPoints(pixels, K, D, P=P) for EVERY integer pixel of the sensor (datasets/rectify_ec.py:70-77): raw pixel (u, v) ->
 * its undistorted position, so that 10^8 events need one lookup each.  x0 = (u - cx) / fx, y0 = (v - cy) / fy; `iters` times
 * x = (x0 - dx(x, y)) / kr(x, y), y = (y0 - dy(x, y)) / kr(x, y) from (x0, y0), dx / dy the tangential terms above (5: the
 * reference call's default criteria); (X, Y, Wp) = P (x, y, 1), map = (X / Wp, Y / Wp).  round_out = 1 stores rint of the double
 * result (rectify_ec.py:78). */
int einx_undistort_points_map_radtan(const double* K, const double* D, const double* P, int H, int W, int iters, int round_out, float* map_x,
                                     float* map_y, void* stream);
/* cv.remap(frame, map_x, map_y, INTER_LINEAR) with BORDER_CONSTANT 0 for F frames in one launch (datasets/MVSEC_rectify.py:16-21;
 * with the radtan map: cv.undistort, datasets/rectify_ec.py:48-50).  src [F,Hs,Ws], dst [F,H,W], both uint8 or both fp32; maps [H,W].
 * x0 = floor(mx), fx = mx - x0 (y likewise), top = I00 + fx (I01 - I00), bot = I10 + fx (I11 - I10), v = top + fy (bot - top),
 * every operation rounded to fp32; a tap outside the source reads 0, a map entry that is not finite gives 0; uint8 output is
 * rint(v) clamped to 0..255.  Interpolates at the map's own coordinate (OpenCV quantises it to 1/32 px first: DESIGN.md 8q). */
enum { EINX_REMAP_U8 = 0, EINX_REMAP_F32 = 1 };
int einx_remap_bilinear(const void* src, int src_type, int F, int Hs, int Ws, const float* map_x, const float* map_y, int H, int W, void* dst,
                        void* stream);
/* The event pass of both scripts (datasets/MVSEC_rectify.py:23-45, datasets/rectify_ec.py:70-83 with the points map above): for
 * event k of the stream x / y / p (fp32), t (fp64) of N events, in order: ox = rint(x[k]), oy = rint(y[k]) (half to even,
 * np.round); an event with ox outside [0, W) or oy outside [0, H), or either not finite, is counted in out_counts[1] and dropped
 * (numpy raises for a coordinate >= W and wraps a negative one); otherwise x' = map_x[oy, ox], y' = map_y[oy, ox] and the event is
 * kept iff 0 <= x' < x_hi and 0 <= y' < y_hi (NaN fails): (W - 1, H - 1) is MVSEC's rule (:37-43), (W, H) EC's (:80-83).  The kept
 * events are written densely and in input order to out_* (sized N): x', y' the map's values, t and p copied, all bit for bit;
 * out_counts[0] = the number kept (device, int64 [2]).  A stable compaction: per-workgroup counts, a scan of the counts, a
 * ranked scatter; every offset is an integer sum, so two calls give the same bits.  N may exceed 2^31 (N = 0: only the counts
 * are written).  The workspace holds one int64 per einx_events_remap_chunk() events and per 1024 of those. */
size_t einx_events_remap_ws_bytes(int64_t N);
int einx_events_remap(const float* x, const float* y, const double* t, const float* p, int64_t N, const float* map_x, const float* map_y,
                      int H, int W, float x_hi, float y_hi, float* out_x, float* out_y, double* out_t, float* out_p, int64_t* out_counts,
                      void* ws, size_t ws_bytes, void* stream);
int einx_events_remap_chunk(void); /* events per workgroup of einx_events_remap (host only) */

/* ------------------------------------------------------------------------------------------
 * Perspective warp of a batch of images (csrc/warp.hip): view 1 of a homographic pair
 * The reference has the sampler of the homographies (core/geometry/homography.py) and nothing that warps an image with one.
 * src [B,C,Hs,Ws] -> dst [B,C,Hd,Wd], both uint8 or both fp32 (the src_type codes of einx_remap_bilinear), one matrix per sample:
 * Hinv double[B,9] row-major ON THE DEVICE, the destination -> source map (the caller inverts the homography once, in float64).
 * Pixel (r, c) sits at (x, y) = (c + 0.5, r + 0.5).  For every destination pixel, in float64 with every operation rounded as
 * written: X = (h0 x + h1 y) + h2, Y = (h3 x + h4 y) + h5, w = (h6 x + h7 y) + h8, qx = X / w, qy = Y / w.  The pixel is VALID iff
 * w is finite and > 0, 0.5 <= qx <= Ws - 0.5 and 0.5 <= qy <= Hs - 0.5: all four taps lie inside the source.  An invalid pixel is 0
 * in every channel and in `valid`; there is no border blending.  A valid one samples the source at index coordinates
 * (sx, sy) = (qx - 0.5, qy - 0.5):
 *   EINX_WARP_BILINEAR: x0 = floor(sx), fx = (float)(sx - x0), gx = 1 - fx (y likewise), w00 = gx gy, w01 = fx gy, w10 = gx fy,
 *     w11 = fx fy, v = ((w00 I00 + w01 I01) + w10 I10) + w11 I11, all fp32; a tap at x0 + 1 == Ws or y0 + 1 == Hs (weight 0) reads
 *     as 0; NaN in any other tap propagates; uint8 output is rint(v) (half to even) clamped to 0..255.
 *   EINX_WARP_NEAREST: the source pixel (rint(sy), rint(sx)), half to even, copied bit for bit: what a mask needs.
 * valid: uint8 [B,Hd,Wd] or NULL.  Enqueues on `stream`, takes no workspace, allocates nothing, waits for nothing and can be
 * captured; no atomics: two calls give the same bits.  EINX_ERR_ARG: a negative size, an unknown src_type or mode, a null pointer
 * that would be read or written.  B, Hd or Wd == 0 (or C == 0 without `valid`) succeeds and launches nothing; Hs or Ws == 0
 * makes every pixel invalid.
 * ------------------------------------------------------------------------------------------ */
enum { EINX_WARP_BILINEAR = 0, EINX_WARP_NEAREST = 1 };
int einx_warp_perspective(const void* src, int src_type, int B, int C, int Hs, int Ws, const double* Hinv, int Hd, int Wd, int mode, void* dst,
                          uint8_t* valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pose tracks and the depth / image pairing of a recording (csrc/posetrack.hip)
 * replaces: datasets/Interpolator.py (PoseInterpolator), datasets/MVSEC.py:818-830 (get_relative_pose), :362-369 (nearest pairing)
 * A track is N >= 2 knots on the device: stamps double[N] strictly increasing (epoch seconds: float32 cannot hold them),
 * translations double[N,3] and UNIT quaternions double[N,4] as (x, y, z, w) of the poses T_W_j.  All arithmetic is float64 with
 * every operation rounded as written.  Every call enqueues on `stream`, takes no workspace, waits for nothing and can be captured;
 * two calls give the same bits.  EINX_ERR_ARG: null pointers, N < 2, negative counts, an unknown out_type, F <= 0.
 * ------------------------------------------------------------------------------------------ */
/* PoseInterpolator.interpolate (datasets/Interpolator.py:54-69) for Q queries double[Q], one thread each: out [Q,4,4] row-major of
 * out_type.  i = clamp(lower_bound(stamps, q) - 1, 0, N - 2), the interval of scipy's Slerp.__call__ and linear interp1d (a query
 * on a knot takes the interval on its left with alpha = 1, the first knot i = 0 with alpha = 0); alpha = (q - t_i) / (t_i+1 - t_i);
 * translation (p_i+1 - p_i) / (t_i+1 - t_i) * (q - t_i) + p_i (interp1d's order, :45-47, :65-67); rotation by quaternion slerp on
 * the shorter arc (:50-52, :68): q_i+1 negated when the dot product d is negative, theta = atan2(|q_i+1 - d q_i|, d), weights
 * sin((1 - alpha) theta) / sin(theta) and sin(alpha theta) / sin(theta) (1 - alpha and alpha below 1e-12 rad), the result
 * renormalised.  inverse = 1 writes T_j_W = [R^T | -R^T p] in closed form (:69 calls np.linalg.inv), inverse = 0 T_W_j = [R | p].
 * A query outside [t_0, t_N-1] or NaN gives sixteen NaNs and adds one to *out_of_range (device int32, zeroed by the call); the
 * reference prints a line and interp1d raises. */
enum { EINX_POSE_F32 = 0, EINX_POSE_F64 = 1 };
int einx_pose_interp(const double* stamps, const double* trans, const double* quats, int N, const double* queries, int Q, int inverse,
                     int out_type, void* out, int32_t* out_of_range, void* stream);
/* MVSECDataset_RPE_VAL.__getitem__'s two get_relative_pose calls (datasets/MVSEC.py:1081-1085, :818-830) for P pairs of queries
 * q0[P], q1[P]: T_0to1 = T_1_W T_W_0 and T_1to0 = T_0_W T_W_1, both [P,4,4] fp32.  The two interpolations above, the closed-form
 * rigid inverse and the products are float64, cast ONCE (the rule of datasets/pairs.py::relative_transforms).  The reference casts
 * each interpolated pose to float32 first and then forms pose1 @ np.linalg.inv(pose0) in float32: the two can differ in the last
 * float32 bit.  A pair with a query outside the track has NaN in both matrices; *out_of_range counts such QUERIES. */
int einx_pose_relative(const double* stamps, const double* trans, const double* quats, int N, const double* q0, const double* q1, int P,
                       float* T_0to1, float* T_1to0, int32_t* out_of_range, void* stream);
/* np.abs(np.subtract.outer(stamps, queries)).argmin(axis=0) (datasets/MVSEC.py:364-366) for sorted stamps double[F] (non-decreasing,
 * duplicates allowed) without the F x Q matrix: out[k] int64 = the FIRST index i whose fabs(stamps[i] - queries[k]), evaluated in
 * float64, is minimal.  Two binary searches per query: for the first stamp that is not below the query, and -- when the minimum
 * lies left of it -- for the first stamp with that rounded distance (equal stamps, or different stamps that tie after rounding).
 * A tie between the stamp below and the stamp above gives the lower index.  A NaN query gives 0, as argmin of an all-NaN column. */
int einx_nearest_stamp(const double* stamps, int64_t F, const double* queries, int64_t Q, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Handle-level extractor: ONE call enqueues a whole network (SURVEY.md 8b's coarse ABI)
 * replaces: VGGExtractor.forward / VGGExtractorNP.forward
 *             core/modules/event_extractors/EventExtractors.py:517-624, :331-434
 *           SuperPointv1.forward  core/modules/image_extractors/superpoint_extractor.py:345-480
 *           SiLKModel.forward     core/modules/image_extractors/silk_extractor.py:177-257
 * up to (not including) the Python output dict.  The handle owns copies of the layer descriptors only;
 * weights stay in caller-owned device memory (einx_conv_repack / einx_bn_fold images).  einx_extract makes no
 * allocation and no host synchronisation; it is bit-identical to the same sequence of op-level calls.
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_extractor einx_extractor; /* opaque */

typedef struct einx_extractor_desc {
  size_t struct_size;  /* sizeof(einx_extractor_desc) of the caller's header (checked by einx_extractor_create) */
  int32_t cell;        /* 8: SuperPoint-shaped (65-channel detector head, coarse descriptors); 1: SiLK-shaped */
  int32_t n_backbone, n_det, n_desc;
  const einx_conv_desc* backbone; /* host arrays, copied by einx_extractor_create */
  const einx_conv_desc* det_head;
  const einx_conv_desc* desc_head;
  int32_t dilate_mask; /* event extractors dilate the events mask 3x3 (EventExtractors.py:544-550) */
  int32_t border;      /* remove_borders */
  int32_t nms_radius;
  int32_t top_k;       /* detection_top_k (0 = none) */
  float det_thr;       /* detection_threshold */
  int32_t ordering_xy; /* 0: (y,x,p)  1: (x,y,p) */
  float desc_scale;    /* descriptor_scale_factor */
  float input_div;     /* SuperPointv1 scales its input in place (`image /= 255.0`, superpoint_extractor.py:372); 0 = off */
  /* optional (NULL = off): det_head[0] and desc_head[0] -- two 3x3 layers that read the same backbone features -- as ONE layer whose
   * output channels are det_head[0]'s followed by desc_head[0]'s (weights / bias / BatchNorm concatenated by the caller).  Used for
   * single images (B == 1, two-layer heads): one launch instead of two on the latency-bound chain of a single-pair forward; every
   * output channel is the same k-ordered chain, so results are bit-identical.  Larger batches keep the two launches. */
  const einx_conv_desc* merged_head0;
} einx_extractor_desc;

typedef struct einx_extract_shapes_t {
  int32_t Hp, Wp, h0, w0; /* padded size and top/left padding (Padder, utils/util.py:6-15) */
  int32_t hc, wc;         /* head resolution (Hp/cell, Wp/cell) */
  int32_t feat_channels, det_channels, desc_dim;
  int32_t cap;            /* keypoint rows per image the detector can emit (top-k quantile arithmetic) */
} einx_extract_shapes_t;

typedef struct einx_extract_out {
  float* feats;     /* [B,feat_channels,hc,wc]   backbone_feats */
  float* logits;    /* [B,det_channels,hc,wc] */
  float* raw;       /* [B,desc_dim,hc,wc]        raw_descriptors */
  float* prob;      /* [B,det_channels,hc,wc]    probability */
  float* score;     /* [B,1,Hp,Wp]               padded score map (masked, border-zeroed) */
  float* coarse;    /* [B,desc_dim,hc,wc]        coarse_descriptors (cell 8) or NULL */
  float* raw_cl;    /* [B,hc*wc,desc_dim]        channels-last raw copy for the sparse sampler (cell 8) or NULL */
  float* nms;       /* [B,H,W]                   thresholded NMS map, cropped, or NULL */
  float* positions; /* [B,cap,3] */
  int32_t* indices; /* [B,cap] */
  int32_t* counts;  /* [B] */
  float* thr;       /* [B] */
  int32_t* not_converged; /* [B] 1: the NMS fix-point of this image needs more passes than were enqueued (see einx_detect) */
  float* sparse_desc;     /* [B,cap,desc_dim] */
  int32_t cap;
  float* score_crop;      /* optional (NULL: off): [B,1,H,W] the un-padded score map of the output dict (Padder.unpad, utils/util.py:42-50),
                             written by the score kernel instead of by a crop + clone afterwards */
} einx_extract_out;

/* Optional content watch of a network's weights riding on an einx_extract_watch call (what einx_params_hash does as a launch
 * of its own): the rows of `table` are hashed by spare workgroups of the call's last kernel and compared with `ref`; a
 * difference ORs 1 into *stale.  The library never clears *stale: it belongs to whoever recorded `ref` (a stale watch stays
 * stale until its owner re-records the hashes and zeroes the word).  A torch-free host that never edits weights behind the
 * library's back has no use for it and calls einx_extract. */
typedef struct einx_weight_watch {
  size_t struct_size;     /* sizeof(einx_weight_watch) */
  int32_t n;              /* rows (0: off) */
  const int64_t* table;   /* device [n][2]: (pointer, number of 32-bit words) per row, as einx_params_hash */
  const uint64_t* ref;    /* device [n] hashes stored when the native weight images were built */
  uint64_t* scratch;      /* device [n] */
  int32_t* stale;         /* device int32, OR-ed with 1 on a mismatch */
} einx_weight_watch;

einx_extractor* einx_extractor_create(const einx_extractor_desc* d); /* NULL on error (einx_last_error) */
void einx_extractor_destroy(einx_extractor* e);
/* Opt-in binary16 convolutions for a handle (einx_conv_block_f16's contract).  backbone / det_head / desc_head: host
 * arrays of n_backbone / n_det / n_desc POINTERS, parallel to the layer arrays einx_extractor_create copied (the descriptors are
 * copied here too); a NULL entry or a NULL array leaves that layer on einx_conv_block, all NULL restores the fp32 forward.  Each
 * descriptor must describe its layer (cin, cout, ks, relu, pool) and have cin % 8 == 0.  einx_extract / einx_extract_watch then run
 * a layer through einx_conv_block_f16 exactly when an image is set for it and einx_conv_f16_plan covers the call; the first layer
 * (replicate-pad fold) never is, and a second layer with an image set runs as a launch of its own instead of inside the fused first
 * pair.  Streams, workspace (einx_extract_ws_bytes) and every other launch are unchanged.  Not to be called while another thread
 * runs einx_extract on the handle. */
int einx_extractor_set_conv_f16(einx_extractor* e, const einx_conv_desc_f16* const* backbone, const einx_conv_desc_f16* const* det_head,
                                const einx_conv_desc_f16* const* desc_head, const einx_conv_desc_f16* merged_head0);
/* Side streams (no reference counterpart).  einx_extract forks onto a side stream of its caller's stream; a host that runs two
 * extractors on two streams wants the second beside the first.  HIP deals streams onto a few hardware queues, and a side stream
 * on its caller's queue serialises the fork (single pair: 0.77 -> 1.06 ms).  So, per device, the library keeps EINX_FORK_STREAMS_MAX
 * slots of two events and, per lane, EINX_FORK_STREAM_POOL streams (created at the first use, never destroyed).  A slot is keyed
 * on (caller stream, lane) -- lane 0: einx_extract's fork, lane 1: einx_side_stream -- and lent the stream of its lane's pool that
 * a probe (einx_stream_overlap_us) finds beside the caller, the `beside` streams and the streams of the two most recently used
 * other slots of the device.  A new key takes a free slot or the least recently used one that no call holds (with none left,
 * einx_extract runs its branches in line, the same bits, and the calls below fail).  The probe synchronises with the caller's
 * stream (a few hundred microseconds per pool stream tried, once per key; skipped while it is capturing); probes of one device
 * take turns, nothing else waits for them.
 * einx_fork_stream_prepare[_beside]: choose the lane-0 side of `stream` NOW instead of at the first einx_extract that forks on it,
 * staying clear of up to 8 `beside` streams (the other extractor's stream and its side stream); no effect when it has one.
 * einx_side_stream: the side stream of `stream` in `lane` (0 or 1), lent for the life of the process; NULL on error.
 * einx_fork_stream_release un-keys the slots of `stream` (a host that destroys a stream it has made calls on; optional).
 * einx_fork_stream_count: keyed slots, all devices; einx_fork_stream_of: the lane-0 side stream, NULL when none (diagnostics). */
#define EINX_FORK_STREAMS_MAX 16
#define EINX_FORK_STREAM_POOL 8
int einx_fork_stream_prepare(void* stream);
int einx_fork_stream_prepare_beside(void* stream, void* const* beside, int n_beside);
void* einx_side_stream(void* stream, int lane, void* const* beside, int n_beside);
int einx_fork_stream_release(void* stream);
int einx_fork_stream_count(void);
void* einx_fork_stream_of(void* stream);
int einx_extract_shapes(const einx_extractor* e, int H, int W, einx_extract_shapes_t* shapes);
/* nms_iters: NMS pass budget per call (see einx_detect); <= 0 selects the default (8) in BOTH functions below.  The
 * workspace size depends on it (B x nms_iters convergence flags), so query and call must pass the same value. */
size_t einx_extract_ws_bytes(const einx_extractor* e, int B, int H, int W, int cap, int nms_iters);
/* in [B,cin,H,W] (modified in place only when input_div is set); mask [B,1,H,W] uint8 or NULL;
 * ws: device scratch, ws_bytes >= einx_extract_ws_bytes(e, B, H, W, out->cap, nms_iters) (checked).
 * Networks with 1/8-resolution heads (cell == 8; full-resolution networks while B x head pixels <= 8192) enqueue the descriptor
 * branch on a library-owned side stream between a fork and a join event of `stream`; every return path has `stream` wait for the
 * join.  The side stream is chosen on the FIRST such call for a (device, stream) pair (or by einx_fork_stream_prepare), shared by
 * every handle of the process -- so make one un-captured call (or the prepare call) per stream before capturing einx_extract into
 * a hipGraph (the probe is not capturable).  While `stream` is being captured the branches are enqueued in line (no fork: a fork
 * nested in a caller's own fork / join makes hipStreamEndCapture of ROCm 7.2 crash).  Calls that fork from one stream are
 * serialised on a mutex. */
int einx_extract(const einx_extractor* e, float* in, const uint8_t* mask, int B, int H, int W, int nms_iters, void* ws,
                 size_t ws_bytes, const einx_extract_out* out, void* stream);
/* the same call with the weight watch riding on it (watch == NULL or watch->n == 0: exactly einx_extract) */
int einx_extract_watch(const einx_extractor* e, float* in, const uint8_t* mask, int B, int H, int W, int nms_iters, void* ws,
                       size_t ws_bytes, const einx_extract_out* out, const einx_weight_watch* watch, void* stream);
/* the same call with the padding rule of the mask (EINX_MASK_PAD_*, see einx_score_map_pad); the two calls above pad with zeros */
int einx_extract_pad(const einx_extractor* e, float* in, const uint8_t* mask, int mask_pad, int B, int H, int W, int nms_iters, void* ws,
                     size_t ws_bytes, const einx_extract_out* out, const einx_weight_watch* watch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics of the reference's test harness (the step after the path)
 *   MatchingRatio            core/metrics/matching_metrics.py:30-51
 *   MeanMatchingAccuracy@t   core/metrics/matching_metrics.py:84-156   (points ordering "yx")
 *   ValidDescriptorsDistance core/metrics/keypoints_metrics.py:160-290 (repeat./distance/angle @t)
 * Inputs are the device-side batch results of the path: keypoints [B,cap,3], descriptors
 * [B,cap,D], counts, matched keypoints [B,cap0,cols] + nmatch (einx_gather_matches), optional
 * homography [B,9] (NULL = identity, as test_events-image_same-time.py:146 uses).
 * out: [B, 1 + n_mma + 3*n_vdd] float64 = MR, MMA@t..., (Repeatability, ValidDistance, Angle)@t...
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_metric_params {
  int32_t B, cap0, cap1, D, cols;
  int32_t H0, W0, H1, W1; /* img1_shape, img2_shape */
  int32_t kp_yx;          /* 1: keypoints are (y,x,..) (the extractors' "yx" ordering) */
  int32_t n_mma, n_vdd;
  float mma_thr[4];
  float vdd_thr[4];
  int32_t rep_nan_if_empty; /* 1: Repeatability@t = NaN when NEITHER image keeps a keypoint after the visibility filter
                               (class Repeatability emits no entry then, keypoints_metrics.py:126-128; VDD reports 0) */
} einx_metric_params;
size_t einx_metrics_ws_bytes(const einx_metric_params* p);
int einx_pair_metrics(const einx_metric_params* p, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                      const int32_t* n, const int32_t* m, const float* mk0, const float* mk1, const int32_t* nmatch,
                      const float* homography, void* ws, double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same metrics for a pair related by depth + motion instead of a homography (csrc/metrics.hip): what
 * the different-time evaluation (test_events-image_different_time.py:187-264) can say about keypoints and matches under the
 * geometry it has.  The reference has no such metric; each part restates reference text:
 *   sample_depth, project (ccth= branch: the occlusion check)   core/geometry/depth.py:9-69
 *   pinhole cam2image                                           core/geometry/wrappers.py:337-385
 *   keep_true_points (inside the other IMAGE)                   core/metrics/util.py:43-70
 *   MeanMatchingAccuracy / ValidDescriptorsDistance rules       core/metrics/matching_metrics.py:84-156, keypoints_metrics.py:160-290
 *   sym_epipolar_distance_all (F = K1^-T [t]x R K0^-1)          core/geometry/epipolar.py:59-80, gt_generation.py:128-133
 * Inputs as einx_pair_metrics takes them, with depth0 [B,dH0,dW0] / depth1 [B,dH1,dW1] float32 (BOTH NULL or both given), K0 / K1
 * [B,9], T_0to1 [B,16] float32 and T_1to0 [B,16] or NULL ((R^T, -R^T t) of T_0to1, as 8e).  A keypoint of view 0 goes through
 * depth0 and T_0to1 into view 1 with 8e stage A's sampler and projection, bit for bit; it is kept when its depth is valid, it lies
 * in front of camera 1 (q.z > 1e-4) and 0 <= u < W1, 0 <= v < H1; view 1 likewise into image 0.  occlusion_th > 0 adds the
 * reference's circle-consistency test: the other map sampled at (u, v), back-projected with the inverse motion, must be valid, in
 * front and within occlusion_th PIXELS of the keypoint (squared on both sides; the reference compares the squared distance with
 * the unsquared ccth).
 * out: [B, 1 + n_mma + 1 + 3 n_vdd + n_epi] float64 =
 *   MR                                 as einx_pair_metrics
 *   MMA@t...                           #(judged and |proj(mk0) - mk1| <= t) / #judged, judged = valid and in front (and the occlusion
 *                                      test); a match whose true location left the image is wrong, not unjudged
 *   judged_ratio                       #judged / M
 *   (Repeatability, ValidDistance, Angle)@t...   einx_pair_metrics' rule on the projected / kept keypoints
 *   EPI@t...                           #(symmetric epipolar distance <= t) / M, the distance in double, pixels; needs no depth.  A
 *                                      pure rotation has F = 0: every match passes
 * Quotients of counts are float32 quotients.  A quotient with an empty denominator is NaN (nothing could be judged): MMA@t without
 * a judged match, judged_ratio / EPI@t for M == 0, the VDD triple when either view keeps no keypoint.  With the depth pointers
 * NULL everything but MR and EPI@t is NaN and nothing is sampled.  Workspace O(B (cap0 + cap1)), no N x M term; integer atomics
 * only: two runs give the same bits.  Nothing synchronises or allocates; the call can be captured.
 * EINX_ERR_ARG (and a workspace query of 0): wrong struct_size, more than 4 thresholds of a kind, cols outside {2, 3}, a
 * non-positive size; the call also refuses exactly one depth pointer.
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_pose_metric_params {
  size_t struct_size;         /* sizeof(einx_pose_metric_params) (checked) */
  int32_t B, cap0, cap1, D, cols;
  int32_t H0, W0, H1, W1;     /* image sizes: the bound of "inside the other image" */
  int32_t dH0, dW0, dH1, dW1; /* sizes of depth0 / depth1 (unused when they are NULL) */
  int32_t kp_yx;              /* 1: keypoints are (y,x,..) */
  int32_t n_mma, n_vdd, n_epi; /* thresholds of each kind (0..4) */
  float mma_thr[4];
  float vdd_thr[4];
  float epi_thr[4];
  float occlusion_th;         /* pixels; <= 0: no occlusion check */
} einx_pose_metric_params;
size_t einx_pair_metrics_pose_ws_bytes(const einx_pose_metric_params* p); /* 0 on refused parameters */
int einx_pair_metrics_pose(const einx_pose_metric_params* p, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                           const int32_t* n, const int32_t* m, const float* mk0, const float* mk1, const int32_t* nmatch,
                           const float* depth0, const float* depth1, const float* K0, const float* K1, const float* T_0to1,
                           const float* T_1to0, void* ws, double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Relative pose of the different-time evaluation (csrc/pose.hip)
 *   RelativePoseEstimation   core/metrics/matching_metrics.py:347-559 (cv2.findEssentialMat RANSAC + cv2.recoverPose)
 * B pairs of matched keypoints mk0 / mk1 [B,cap,cols] float32 + nmatch int32 [B] (einx_gather_matches' layout), K0 / K1
 * [B,3,3] (float32 or float64, k_f64), T_0to1 [B,4,4] float64 or NULL.  The written algorithm of DESIGN.md 8b, not bit parity
 * with OpenCV (its random draws and root order are not reproduced).  Outputs:
 *   R_out [B,9] / t_out [B,3] float64 (zeros without a pose), mask_out [B,cap] uint8 (the recoverPose mask),
 *   status [B] int32: >= 0 pose found, = 16 * RANSAC iteration + solution index of the chosen model (the solution index
 *     alone for exactly 5 matches); -1 fewer than 5 matches, -2 no essential matrix, -3 no point passes the cheirality test,
 *   rows_out [B,4] float64 or NULL: R_err, t_err, pose_err (degrees), inlier ratio -- update_one's values (inf, inf, inf, 0
 *     without a pose; NaN errors when T_0to1 is NULL).
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_pose_params {
  size_t struct_size; /* sizeof(einx_pose_params) (checked) */
  int32_t B, cap, cols;
  int32_t kp_yx;      /* 1: keypoints are (y,x,..) */
  int32_t k_f64;      /* 0: K0 / K1 float32, 1: float64 (numpy's dtype of the normalisation and the threshold) */
  int32_t max_iters;  /* RANSAC iterations (1000: findEssentialMat's maxIters) */
  double thresh;      /* pixels; divided by mean(K0[0,0], K1[1,1], K0[0,0], K1[1,1]) */
  double conf;        /* RANSAC confidence (0.999) */
  uint64_t seed;      /* counter-based generator key */
} einx_pose_params;
size_t einx_relative_pose_ws_bytes(const einx_pose_params* p);
int einx_relative_pose(const einx_pose_params* p, const float* mk0, const float* mk1, const int32_t* nmatch, const void* K0, const void* K1,
                       const double* T_0to1, void* ws, double* R_out, double* t_out, uint8_t* mask_out, int32_t* status, double* rows_out,
                       void* stream);
/* The minimal solver alone (test aid, like einx_math_eval): x1 / x2 [n,5,2] float64 normalised points; E_out [n,10,9] float64 gets
 * every real essential matrix of each problem ordered by ascending E[2,1] / E[2,2] (scaled to E[2,2] = 1), n_solutions [n] int32
 * their count (0 for a singular sample). */
int einx_essential_5pt(const double* x1, const double* x2, int n_problems, double* E_out, int32_t* n_solutions, void* stream);

/* ------------------------------------------------------------------------------------------
 * Refinement of the relative pose on its inliers (csrc/pose.hip)
 * einx_relative_pose returns the pose of one five-point sample, as cv2.findEssentialMat + cv2.recoverPose do.  This entry fits
 * that pose to the matches that agree with it: Levenberg-Marquardt on the signed Sampson distances over the five parameters of
 * E = [t]x R with |t| = 1, in `rounds` rounds that each re-select the Sampson inliers of the current E (8b's points, threshold and
 * float-rounded compare) and run at most `lm_iters` iterations on them; a round needs 6 inliers.  A written algorithm (DESIGN.md
 * 8w), not parity with a library: the reference uses recoverPose's result as it is.
 * Inputs: mk0 / mk1 / nmatch / K0 / K1 / T_0to1 as einx_relative_pose takes them, and its outputs for the same pairs: R_in [B,9],
 * t_in [B,3] float64, mask_in [B,cap] uint8, status_in [B] int32.  Outputs:
 *   R_out [B,9] / t_out [B,3] float64, mask_out [B,cap] uint8, rows_out [B,4] float64 or NULL (einx_relative_pose's four values of
 *     the returned pose).  The refined pose is returned iff a step was accepted and its Sampson inlier count is not below the
 *     input pose's; its mask is its Sampson inliers that pass recoverPose's cheirality test.  Otherwise the input pose and mask_in
 *     come back unchanged, so the option never lowers a pair's inlier count.  status_in < 0: zeros and the no-pose rows.
 *   info_out [B,4] int32: kept (1 the refined pose, 0 the input pose, -1 no pose), rounds run, steps accepted over all rounds,
 *     the size of the last round's set (0 when no round ran),
 *   cost_out [B,2] float64 or NULL: the mean squared residual over the last round's set before and after that round's iterations
 *     (NaN where no round ran).
 * Every sum runs in a fixed order: two runs give the same bits, and a pair's result depends neither on its slot nor on B.
 * Nothing allocates, synchronises or uses atomics; the call can be captured.
 * EINX_ERR_ARG (and a workspace query of 0): wrong struct_size, a non-positive size, cols outside {2, 3}, kp_yx / k_f64 outside
 * {0, 1}, rounds outside 1..4, lm_iters outside 1..50, a thresh that is not a positive number; the call also refuses a null
 * pointer other than T_0to1, rows_out and cost_out.
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_pose_refine_params {
  size_t struct_size; /* sizeof(einx_pose_refine_params) (checked) */
  int32_t B, cap, cols;
  int32_t kp_yx;      /* 1: keypoints are (y,x,..) */
  int32_t k_f64;      /* 0: K0 / K1 float32, 1: float64 (as einx_pose_params) */
  int32_t rounds;     /* rounds of inlier selection + LM (1..4; 2) */
  int32_t lm_iters;   /* LM iterations of a round at the most (1..50; 10) */
  double thresh;      /* pixels; the value einx_relative_pose ran with */
} einx_pose_refine_params;
size_t einx_relative_pose_refine_ws_bytes(const einx_pose_refine_params* p); /* 0 on refused parameters */
int einx_relative_pose_refine(const einx_pose_refine_params* p, const float* mk0, const float* mk1, const int32_t* nmatch, const void* K0,
                              const void* K1, const double* R_in, const double* t_in, const uint8_t* mask_in, const int32_t* status_in,
                              const double* T_0to1, void* ws, double* R_out, double* t_out, uint8_t* mask_out, double* rows_out,
                              int32_t* info_out, double* cost_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Homography of the same-time evaluation (csrc/homography.hip)
 *   HomographyEstimation   core/metrics/matching_metrics.py:188-345 (cv2.findHomography(RANSAC) with its defaults + the corner
 *                          distances of update_one, :232-297)
 * B pairs of matched keypoints mk0 / mk1 [B,cap,cols] float32 + nmatch int32 [B] (einx_gather_matches' layout), img_shape
 * [B,2] int32 (H, W) or NULL, H_true [B,9] float32 or NULL.  The written algorithm of DESIGN.md 8c, not bit parity with OpenCV
 * (its random draws are not reproduced).  Outputs:
 *   H_out [B,9] float64 (H[2,2] = 1; zeros without a homography), mask_out [B,cap] uint8 (the RANSAC mask, not re-evaluated
 *     after the refit and the polish),
 *   status [B] int32: >= 0 the chosen RANSAC iteration (0 for exactly 4 matches); -1 fewer than 4 matches, -2 no homography (no
 *     sample passed checkSubset and the fit, or the refit on the inliers failed),
 *   rows_out [B,n_thr+2] float64 or NULL: (mean corner distance <= he_thr[i]) for i < n_thr, the mean corner distance (float32
 *     arithmetic, as update_one), the inlier ratio -- 0.., inf, 0 without a homography; NaN ratios and error when img_shape or
 *     H_true is NULL.
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_homography_params {
  size_t struct_size; /* sizeof(einx_homography_params) (checked) */
  int32_t B, cap, cols;
  int32_t kp_yx;      /* 1: keypoints are (y,x,..) */
  int32_t max_iters;  /* RANSAC iterations (2000: findHomography's maxIters) */
  int32_t n_thr;      /* correctness thresholds in he_thr (0..4) */
  double thresh;      /* ransacReprojThreshold in pixels (3.0) */
  double conf;        /* RANSAC confidence (0.995) */
  float he_thr[4];    /* update_one's correctness_thresh */
  uint64_t seed;      /* counter-based generator key */
} einx_homography_params;
size_t einx_homography_ws_bytes(const einx_homography_params* p);
int einx_homography(const einx_homography_params* p, const float* mk0, const float* mk1, const int32_t* nmatch, const int32_t* img_shape,
                    const float* H_true, void* ws, double* H_out, uint8_t* mask_out, int32_t* status, double* rows_out, void* stream);
/* The fit alone (test aid, like einx_essential_5pt): x1 / x2 [n,n_points,2] float64 points (rounded to the float32 the estimator
 * stores); H_out [n,9] float64 gets the normalised DLT of each problem (H[2,2] = 1), ok [n] int32 is 0 where it has none. */
int einx_homography_dlt(const double* x1, const double* x2, int n_problems, int n_points, double* H_out, int32_t* ok, void* stream);

/* ------------------------------------------------------------------------------------------
 * Absolute (metric) pose from matches and the depth of view 0 (csrc/abs_pose.hip)
 * The reference estimates no metric pose; this is a written algorithm (perspective-three-point RANSAC, a Levenberg-Marquardt
 * refit on the inliers), not parity with OpenCV's solvePnPRansac.
 * B pairs of matched keypoints mk0 / mk1 [B,cap,cols] float32 + nmatch int32 [B] (einx_gather_matches' layout).  The depth of a
 * match of view 0 is sampled from depth0 [B,H,W] float32 with einx_gt_project's sampler, or given as d_in [B,cap] float32 +
 * valid_in [B,cap] uint8: exactly one of the two forms.  K0 / K1 [B,9] float32, T_0to1 [B,16] float64 or NULL.  A match is usable
 * when its depth is valid; everything runs over the nu usable matches of a pair.  Outputs:
 *   R_out [B,9], t_out [B,3] float64: x1 = R x0 + t in the depth map's unit (zeros without a pose),
 *   mask_out [B,cap] uint8: the RANSAC model's inliers at their match indices (not re-evaluated after the refit),
 *   status [B] int32: >= 0: 4 * iteration + solution of the chosen model; -1 fewer than 4 usable matches, -2 no model,
 *   rows_out [B,5] float64 or NULL: rotation error (degrees), |t - t_gt|, the angle between t and t_gt (degrees, folded to
 *     [0, 90], NaN for a zero t_gt), inliers / nu, nu / min(nmatch, cap) (NaN without matches) -- inf, inf, inf, 0 without a pose;
 *     the three errors are NaN when T_0to1 is NULL.
 * Nothing synchronises or allocates; the call can be captured.
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_abs_pose_params {
  size_t struct_size; /* sizeof(einx_abs_pose_params) (checked) */
  int32_t B, cap, cols;
  int32_t kp_yx;      /* 1: keypoints are (y,x,..) */
  int32_t H, W;       /* size of depth0 (unused with d_in / valid_in) */
  int32_t max_iters;  /* RANSAC iterations (100: solvePnPRansac's iterationsCount) */
  int32_t refine;     /* 1: the Levenberg-Marquardt refit on the inliers; 0: the RANSAC model itself */
  double thresh;      /* reprojection threshold in pixels of view 1 (8.0) */
  double conf;        /* RANSAC confidence (0.99) */
  uint64_t seed;      /* counter-based generator key */
} einx_abs_pose_params;
size_t einx_absolute_pose_ws_bytes(const einx_abs_pose_params* p); /* 0 on a bad shape */
int einx_absolute_pose(const einx_abs_pose_params* p, const float* mk0, const float* mk1, const int32_t* nmatch, const float* depth0,
                       const float* d_in, const uint8_t* valid_in, const float* K0, const float* K1, const double* T_0to1, void* ws,
                       double* R_out, double* t_out, uint8_t* mask_out, int32_t* status, double* rows_out, void* stream);
/* The minimal solver alone (test aid, like einx_essential_5pt): X [n,3,3] float64 points, f [n,3,3] float64 unit bearings;
 * R_out [n,4,9] / t_out [n,4,3] float64 get every pose with s_i f_i = R X_i + t, s_i > 0, ordered by ascending s3 / s1 (zeros past
 * the count), n_solutions [n] int32 their count (0 for a degenerate sample). */
int einx_p3p(const double* X, const double* f, int n, double* R_out, double* t_out, int32_t* n_solutions, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ground-truth matches and the matcher's precision / recall (csrc/gt_matches.hip)
 *   gt_matches_from_pose_depth / gt_matches_from_homography   core/geometry/gt_generation.py:15-224
 *   sample_depth, project (ccth=None)                         core/geometry/depth.py:9-60
 *   matcher_metrics                                           core/modules/matchers/lightglue.py:17-63
 * Per side: keypoints kp [B,cap,cols>=2] float32 + int32 counts n / m [B] (the PairBatch layout), depth [B,H,W] float32 with its
 * own H, W, K [B,3,3] and T [B,4,4] float32.  T_1to0 may be NULL: the kernel then uses (R^T, -R^T t) of T_0to1.  With the four
 * dk*_in / vk*_in arrays (depths [B,cap] float32 and their validity uint8 per keypoint) the depth maps are not read (may be NULL).
 * Stage A (einx_gt_project, or einx_gt_warp with H [B,9] float32 for the homography form) writes dk [B,cap] sampled depths,
 * valid / vis [B,cap] uint8 and proj [B,cap,2] (x, y) projections into the other view (NaN where the depth is NaN); rows at or
 * beyond a pair's count get zeros.  Stage B (einx_gt_label, from given projections; vis* / valid* NULL = every point visible /
 * valid, the homography form) writes matches [B,cap] int64 (index, -1 unmatched, -2 ignore; -2 at or beyond the count, -1
 * everywhere below it when the pair has n == 0 or m == 0), scores [B,cap] float32 = (matches > -1), and pos0 [B,cap0] int32 (the
 * mutual positive of row i or -1: the dense `assignment` is its scatter; may be NULL).  No N x M intermediate, no atomics: bit-exact
 * given stage A's outputs, and two runs give the same bits.  einx_gt_matches = stage A (einx_gt_warp when p->homography) + B.
 * einx_match_pr: matcher_metrics per pair over its first n[b] rows, out [B,4] float64 = match_recall, match_precision, accuracy,
 * average_precision (NaN for n[b] == 0); matches0 / gt_matches0 [B,cap0] int64, scores0 [B,cap0] float32.
 * Nothing synchronises or allocates; every call can be captured.
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_gt_matches_params {
  size_t struct_size;     /* sizeof(einx_gt_matches_params) (checked) */
  int32_t B, cap0, cap1;
  int32_t cols0, cols1;   /* row width of kp0 / kp1 (>= 2) */
  int32_t kp_yx;          /* 1: keypoints are (y,x,..) */
  int32_t H0, W0, H1, W1; /* sizes of depth0 / depth1 (unused with precomputed depths and by the homography form) */
  int32_t homography;     /* einx_gt_matches: 0 pose form, 1 homography form */
  float pos_sq, neg_sq;   /* pos_th^2, neg_th^2 rounded to float32 (what torch compares a float32 tensor with) */
} einx_gt_matches_params;
size_t einx_gt_matches_ws_bytes(const einx_gt_matches_params* p); /* workspace of einx_gt_label / einx_gt_matches; 0 on a bad shape */
int einx_gt_project(const einx_gt_matches_params* p, const float* kp0, const float* kp1, const int32_t* n, const int32_t* m,
                    const float* depth0, const float* depth1, const float* K0, const float* K1, const float* T_0to1, const float* T_1to0,
                    const float* dk0_in, const float* dk1_in, const uint8_t* vk0_in, const uint8_t* vk1_in, float* dk0, float* dk1,
                    uint8_t* valid0, uint8_t* valid1, float* proj01, float* proj10, uint8_t* vis0, uint8_t* vis1, void* stream);
int einx_gt_warp(const einx_gt_matches_params* p, const float* kp0, const float* kp1, const int32_t* n, const int32_t* m, const float* H,
                 float* proj01, float* proj10, void* stream);
int einx_gt_label(const einx_gt_matches_params* p, const float* kp0, const float* kp1, const int32_t* n, const int32_t* m,
                  const float* proj01, const float* proj10, const uint8_t* vis0, const uint8_t* vis1, const uint8_t* valid0,
                  const uint8_t* valid1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, int32_t* pos0,
                  void* stream);
int einx_gt_matches(const einx_gt_matches_params* p, const float* kp0, const float* kp1, const int32_t* n, const int32_t* m,
                    const float* depth0, const float* depth1, const float* K0, const float* K1, const float* T_0to1, const float* T_1to0,
                    const float* dk0_in, const float* dk1_in, const uint8_t* vk0_in, const uint8_t* vk1_in, const float* H, void* ws,
                    float* dk0, float* dk1, uint8_t* valid0, uint8_t* valid1, float* proj01, float* proj10, uint8_t* vis0, uint8_t* vis1,
                    int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, int32_t* pos0, void* stream);
int einx_match_pr(const int64_t* matches0, const float* scores0, const int64_t* gt_matches0, const int32_t* n, int B, int cap0, double* out,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense-grid ground-truth matches and pair covisibility (csrc/gt_matches.hip)
 *   check_indices                                             datasets/generate_MVSEC_relative_pose_val.py:194-346
 * einx_gt_matches with BOTH keypoint sets the pixel grid of their depth map: keypoint i = y W + x is the pixel centre
 * (x + 0.5, y + 0.5), raster order, no keypoint arrays and no counts.  The outputs equal, bit for bit, what einx_gt_matches writes
 * for those keypoints (pose form), but stage B visits only the pixels of the other map within pos_th + 1 of a pixel's projection:
 * (2 pos_th + 3)^2 candidates per pixel instead of H W.
 * depth0 [F0,H0,W0], depth1 [F1,H1,W1] float32 frame stacks; idx0 / idx1 int32 [B] pick pair b's frames (clamped to [0, F) on the
 * device; NULL = frame b, which needs F >= B).  K0 / K1 [B,9], T_0to1 / T_1to0 [B,16] float32; T_1to0 may be NULL (inverted in the
 * kernel).  Outputs, each of which may be NULL: dk [B,H W] float32, valid / vis [B,H W] uint8, proj [B,H W,2] (x, y), matches
 * [B,H W] int64 (index into the other grid, -1 unmatched, -2 ignore), scores [B,H W] float32 = (matches > -1).  counts [B,4] int32
 * (required) = #(matches0 > -1), #(matches1 > -1), #visible0, #visible1: integer sums, the reference's valid_ratio is
 * counts[0] / min(counts[2], counts[3]).  pos_sq must be finite and > 0, neg_sq >= 0.  Workspace O(B (H0 W0 + H1 W1)), aligned to
 * 256 bytes.  Nothing synchronises or allocates; the call can be captured; two runs give the same bits.
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_gt_dense_params {
  size_t struct_size;     /* sizeof(einx_gt_dense_params) (checked) */
  int32_t B;              /* image pairs */
  int32_t F0, F1;         /* frames in depth0 / depth1 */
  int32_t H0, W0, H1, W1; /* map sizes: H W <= 2^24 per side */
  float pos_sq, neg_sq;   /* pos_th^2, neg_th^2 rounded to float32 */
} einx_gt_dense_params;
size_t einx_gt_dense_ws_bytes(const einx_gt_dense_params* p); /* 0 on a bad shape */
int einx_gt_dense(const einx_gt_dense_params* p, const float* depth0, const float* depth1, const int32_t* idx0, const int32_t* idx1,
                  const float* K0, const float* K1, const float* T_0to1, const float* T_1to0, void* ws, float* dk0, float* dk1,
                  uint8_t* valid0, uint8_t* valid1, float* proj01, float* proj10, uint8_t* vis0, uint8_t* vis1, int64_t* matches0,
                  int64_t* matches1, float* scores0, float* scores1, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * core.geometry.depth and core.geometry.epipolar on the device (csrc/geometry.hip)
 *   sample_fmap, sample_depth                                 core/geometry/depth.py:9-25
 *   project (ccth None or given)                              core/geometry/depth.py:37-69
 *   dense_warp_consistency                                    core/geometry/depth.py:72-89
 *   sym_epipolar_distance_all                                 core/geometry/epipolar.py:59-72
 *   Pose.transform, pinhole cam2image / image2cam             core/geometry/wrappers.py:186-193, :337-398
 * The sampler and the projection are those of einx_gt_project (csrc/gt_project.h): the same bits on the same inputs.  All tensors
 * float32 unless stated, K [B,9], T [B,16]; T is "this view -> the other" and may be NULL when T_other (the other view -> this one)
 * is given: the kernel then uses (R^T, -R^T t) of it.  Nothing synchronises or allocates, no workspace; every call can be captured;
 * two runs give the same bits.
 *
 * The cycle check (cc != 0; depth.py:62-69): the other view's depth map is sampled at the projection (or the caller supplies those
 * samples: dj_in / validj_in), the projection is taken back through the inverse of the FORWARD motion (T_itoj.inv(), not the
 * caller's pose of the other direction), and a point stays visible when that sample is valid, the way back ends in front of and
 * inside this view's camera (0 <= . <= 2c - 1) and dx^2 + dy^2 < cc_bound, strictly (NaN fails).  cc_bound is compared with the
 * SQUARED distance as given: the reference compares squared pixels with its unsquared ccth, so core.geometry.depth.project passes
 * ccth through, and callers that think in pixels pass th^2.  cc == 0 is "ccth=None": no magic value of the bound means "off".
 *
 * einx_geom_project: p->sides = 1 (one direction) or 2 (both, one launch).  Per side: kp [B,cap,cols>=2] ((y,x,..) when p->kp_yx),
 * count int32 [B] or NULL (= cap; rows at or beyond a count get zeros); the points' depths either given (d_in [B,cap] with valid_in
 * uint8) or sampled from this view's map depth [B,H,W]; with cc the other view's map depth_other [B,Ho,Wo] or dj_in / validj_in
 * [B,cap].  Outputs proj [B,cap,2] (x, y; NaN where the depth is) and visible [B,cap] uint8; d_out / valid_out [B,cap] (the depths
 * and validity used) may be NULL.
 * einx_geom_dense_warp: the keypoint of pixel i = y W + x of depth [B,H,W] is its centre (x + 0.5, y + 0.5), its depth the pixel's
 * own value (not a bilinear sample), valid = d > 0.  Outputs warp [B,H,W,2] (8-byte aligned) and visible [B,H,W] uint8 per side, and
 * counts int32 [B,sides,2] = #valid, #visible pixels: integer sums.
 * einx_geom_sample: fmap [B,C,H,W] at pts [B,N,2] (x, y) -> out [B,N,C]: einx_gt_project's depth sampler per channel (bilinear with
 * zero padding at x - 0.5; a hole under a tap of non-zero weight sends the sample to the nearest pixel, half to even; 0 outside the
 * map).  A hole is a NaN, or with depth_rule a value <= 0 or NaN (sample_depth on its NaN-masked map; a hole at the nearest pixel
 * then gives NaN); valid [B,N] uint8 = not NaN and > 0 may be given with depth_rule and C == 1, else NULL.
 * einx_epipolar_all: p0 [B,N,cols0], p1 [B,M,cols1] with 2 or 3 columns (2: w = 1), E [B,9] -> out [B,N,M].  Row line l = E p0
 * (l_i = (E[i,0] x + E[i,1] y) + E[i,2] w) and n0 = sqrt((l_0^2 + l_1^2) + eps), column c_k = (E[0,k] x' + E[1,k] y') + E[2,k] w' and
 * n1 = sqrt((c_0^2 + c_1^2) + eps), each once per point; entry s = |(x' l_0 + y' l_1) + w' l_2|, out = (s / n0 + s / n1) * 0.5.
 * N <= 2^21, M <= 2^24; N == 0 or M == 0 writes nothing.
 * ---------------------------------------------------------------------------------------- */
typedef struct einx_geom_side {
  const float* kp;           /* [B,cap,cols] */
  const int32_t* count;      /* [B] or NULL */
  const float* depth;        /* [B,H,W] this view's depth map, or NULL with d_in / valid_in */
  const float* d_in;         /* [B,cap] */
  const uint8_t* valid_in;   /* [B,cap] */
  const float* depth_other;  /* [B,Ho,Wo] the other view's depth map (cc), or NULL with dj_in / validj_in */
  const float* dj_in;        /* [B,cap] the other view's depth under each projection */
  const uint8_t* validj_in;  /* [B,cap] */
  const float *K, *K_other;  /* [B,9] */
  const float *T, *T_other;  /* [B,16]; one may be NULL */
  float* d_out;              /* [B,cap] or NULL */
  uint8_t* valid_out;        /* [B,cap] or NULL */
  float* proj;               /* [B,cap,2] */
  uint8_t* visible;          /* [B,cap] */
  int32_t cap, cols, H, W, Ho, Wo;
} einx_geom_side;
typedef struct einx_geom_project_params {
  size_t struct_size; /* sizeof(einx_geom_project_params) (checked) */
  int32_t B, sides;   /* sides: 1 or 2 */
  int32_t kp_yx;      /* 1: keypoints are (y,x,..) */
  int32_t cc;         /* 0: no cycle check (ccth=None) */
  float cc_bound;     /* compared with the squared cycle distance, strictly */
  einx_geom_side side[2];
} einx_geom_project_params;
int einx_geom_project(const einx_geom_project_params* p, void* stream);
typedef struct einx_geom_dense_side {
  const float* depth;        /* [B,H,W] */
  const float* depth_other;  /* [B,Ho,Wo] (cc) */
  const float *K, *K_other;  /* [B,9] */
  const float *T, *T_other;  /* [B,16]; one may be NULL */
  float* warp;               /* [B,H,W,2] */
  uint8_t* visible;          /* [B,H,W] */
  int32_t H, W, Ho, Wo;      /* H W <= 2^24 */
} einx_geom_dense_side;
typedef struct einx_geom_dense_params {
  size_t struct_size; /* sizeof(einx_geom_dense_params) (checked) */
  int32_t B, sides;
  int32_t cc;
  float cc_bound;
  int32_t* counts;    /* [B,sides,2] */
  einx_geom_dense_side side[2];
} einx_geom_dense_params;
int einx_geom_dense_warp(const einx_geom_dense_params* p, void* stream);
int einx_geom_sample(const float* fmap, int B, int C, int H, int W, const float* pts, int N, int depth_rule, float* out, uint8_t* valid,
                     void* stream);
int einx_epipolar_all(const float* p0, int cols0, const float* p1, int cols1, const float* E, int B, int N, int M, float eps, float* out,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Forward values of the extractor losses (csrc/loss.hip): validation under no_grad, no autograd.
 *   ScoreLoss, LogitsLoss, DescriptorsLoss (mse / mae / cosine_similarity), FeatureLoss      core/loss/extractor_loss.py:6-383
 * Every call writes out [B,2] float64 = one (sum, count) pair per image: the reference's (pooled) loss value is
 * weight * sum_b(sum) / sum_b(count), a per-pair value weight * sum_b / count_b (count 0 gives NaN, as the reference's 0 / 0).
 * Every term is added in float64; partial sums go through the caller's workspace and are added in a fixed order: no atomics,
 * bit-identical run to run.  Nothing synchronises or allocates; every call can be captured.  ws: aligned to 256 bytes.
 * Masks: mask_type EINX_MASK_NONE (mask NULL, every weight 1), EINX_MASK_U8 (non-zero = 1) or EINX_MASK_F32 (weights).
 *
 * einx_desc_loss: DescriptorsLoss on `normalized_descriptors` of two extractor outputs WITHOUT materialising the [B,D,H,W] maps.
 *   raw_a / raw_b [B,D,hc,wc] with their descriptor_scale_factor; Hp, Wp, h0, w0, H, W as einx_upsample_normalize; cell 8
 *   (bilinear upsample + normalise, cropped) or 1 (hc == Hp, wc == Wp: normalise, cropped); mask [B,H,W].  The elements a (of
 *   side a) and b formed in registers equal, bit for bit, what einx_upsample_normalize / einx_normalize_map would have stored.
 *   MAE: sum = sum w |a - b|, MSE: sum = sum w (a - b)^2 (difference and square rounded to float32, as torch does), count =
 *   D * sum w.  COS: sum = sum_pixels w dot / (max(|a|, 1e-8) max(|b|, 1e-8)) in float64, count = sum w (H * W without a mask);
 *   the module returns 1 - sum / count.  Geometries that einx_upsample_normalize gives to its band kernel (W > 384, wc > 63,
 *   unusual scales) materialise both maps in the workspace and reduce them with einx_map_loss's kernel: same result contract.
 * einx_map_loss: x, y [B,C,P] float32 (contiguous); mask [B,P] (broadcast over C; count = C * sum w) or, with mask_full, [B,C,P]
 *   (count = sum w).  SQ / ABS as above; BCE: x = probability, target t = (y > 0), term -(t max(log x, -100) +
 *   (1 - t) max(log(1 - x), -100)) with the logarithms in float64; COS: cosine over C per position ([B,P] mask only).
 * einx_logits_loss: LogitsLoss.  x, y [B,C,hc,wc], channels 0 .. cell^2 - 1 only; element (c, yc, xc) is pixel
 *   (cell yc + c / cell, cell xc + c % cell) (pixel_shuffle), kept inside the crop window [h0, h0 + H) x [w0, w0 + W)
 *   (Padder.unpad) and weighted by mask [B,H,W] at its cropped position; count = elements in the window, masked or not (the
 *   reference's mean).  Workspace: einx_map_loss_ws_bytes(B, hc * wc).
 * ---------------------------------------------------------------------------------------- */
enum { EINX_MASK_NONE = 0, EINX_MASK_U8 = 1, EINX_MASK_F32 = 2 };
enum { EINX_LOSS_MAE = 0, EINX_LOSS_MSE = 1, EINX_LOSS_COS = 2 };
enum { EINX_MAP_SQ = 0, EINX_MAP_ABS = 1, EINX_MAP_BCE = 2, EINX_MAP_COS = 3 };
size_t einx_desc_loss_ws_bytes(int B, int D, int hc, int wc, int Hp, int Wp, int h0, int w0, int H, int W, int cell); /* 0 on a bad shape */
int einx_desc_loss(const float* raw_a, float scale_a, const float* raw_b, float scale_b, int B, int D, int hc, int wc, int Hp, int Wp,
                   int h0, int w0, int H, int W, int cell, const void* mask, int mask_type, int mode, double* out, void* ws,
                   size_t ws_bytes, void* stream);
size_t einx_map_loss_ws_bytes(int B, int P);
int einx_map_loss(const float* x, const float* y, int B, int C, int P, const void* mask, int mask_type, int mask_full, int mode,
                  double* out, void* ws, size_t ws_bytes, void* stream);
int einx_logits_loss(const float* x, const float* y, int B, int C, int cell, int hc, int wc, int h0, int w0, int H, int W,
                     const void* mask, int mask_type, double* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EINX_H */
