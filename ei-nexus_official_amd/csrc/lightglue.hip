// lightglue.hip -- LightGlue inference on gfx950 (fp32 end to end, fp32 matrix cores; with the opt-in `flash: True` the attention
// alone runs in fp16 on the f16 matrix-core instruction: lg_attn_f16_kernel; with the opt-in `mp: True` the layers'
// linears run on it too, lg_gemm_kernel on the f16 tile engine of gemm_tile_f16.h).
//
// Per layer: SelfBlock (Wqkv GEMM -> rotary -> fused softmax(QK^T/8)V -> out_proj GEMM ->
// concat-free FFN GEMM -> LayerNorm+GELU -> FFN GEMM + residual) on both sides, then CrossBlock
// (to_qk / to_v GEMMs, two fused attentions sharing the 1/8 scale, to_out, same FFN).  After the
// last layer MatchAssignment: final_proj/d^(1/4), similarity tiles with double log-softmax +
// matchability (match_tiles.h), mutual filter.  Everything for a batch of pairs is enqueued on one
// stream with device-side keypoint counts; no host synchronisation.
//
// Attention is flash-style per (pair, head, 128 queries): S^T = K Q^T on the matrix cores with the
// query on the MFMA column so that (a) the online-softmax state (running max / sum) is per lane
// and (b) the probability registers are directly the B operand of the PV product O^T = V^T P^T --
// no LDS round trip for P.  K/V blocks of 64 keys are staged through LDS (K with an odd pitch).
//
// Replaces (reference file:line): core/modules/matchers/lightglue.py:137-148 (normalize_keypoints),
// :161-174 (posenc), :151-158 (rotary), :240-272 (SelfBlock), :275-330 (CrossBlock), :365-418
// (assignment + filter_matches), :522-716 (forward).
#include <stdlib.h>

#include <optional>
#include <type_traits>

#include "gemm_tile_f16.h"
#include "match_tiles.h"

using namespace einx_gemm;
using namespace einx_match;

namespace {

// The shipped configuration (every EI-Nexus YAML): descriptor_dim 256 = 4 heads x 64.  Its kernels are instantiated with these
// as compile-time constants; any other (heads, head_dim in {32, 64, 128}) configuration of lightglue.py:456-461 runs the same
// kernels with the widths taken from the arguments.
constexpr int D = 256;   // descriptor_dim
constexpr int DH = 64;   // head dim

__device__ __forceinline__ int crow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// one side of a batch of pairs: its inputs, and its buffers in the workspace
struct Side {
  const float* kpts;
  const float* desc;
  const int32_t* cnt;
  int cap;
  float *x, *enc, *q, *k, *v, *ctx, *msg, *h, *cert, *dust;
};

// the mode bits of einx_lightglue_mp (einx.h: EINX_LG_ATTN_F16, EINX_LG_LIN_F16)
enum { LG_ATTN_F16 = 1, LG_LIN_F16 = 2 };

// the model's widths and precision modes, as the launchers need them
struct Dims {
  int d, heads, dh;
  bool flash = false;  // LG_ATTN_F16: attention in fp16 on the matrix cores (conf.flash)
  bool lin16 = false;  // LG_LIN_F16: the layers' linears on the f16 tile engine (conf.mp)
  bool shipped() const { return d == D && dh == DH; }
};

}  // namespace

#include "lg_gemm.h"  // the batched Linear: args, tile engines, both kernels, the call record and its launcher
#include "lg_attn.h"  // the fused attention: args, three kernels, the call record and its launcher

namespace {

// ------------------------------------------------------------------------------------------
// positional encoding: enc[b][i][0..dh-1] = cos, [dh..2dh-1] = sin of Wr . normalised keypoint (Wr: [dh/2, 2]),
// each frequency repeated twice (repeat_interleave(2)).
// ------------------------------------------------------------------------------------------
__global__ void lg_posenc_kernel(const float* kpts, const int32_t* cnt, int cap, float s0, float s1, const float* Wr, float* enc, int dh) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int nf = dh >> 1;
  const int i = t / nf, f = t - i * nf;
  if (i >= n) return;
  const float sh0 = s0 / 2.0f, sh1 = s1 / 2.0f;
  const float sc = fmaxf(s0, s1) / 2.0f;
  const float* kp = kpts + ((size_t)b * cap + i) * 3;
  const float k0 = (kp[0] - sh0) / sc, k1 = (kp[1] - sh1) / sc;
  float p = fmaf(k0, Wr[f * 2 + 0], 0.0f);
  p = fmaf(k1, Wr[f * 2 + 1], p);
  float sn, cs;
  einx_sincosf(p, &sn, &cs);
  float* e = enc + ((size_t)b * cap + i) * (2 * dh);
  e[2 * f] = cs;
  e[2 * f + 1] = cs;
  e[dh + 2 * f] = sn;
  e[dh + 2 * f + 1] = sn;
}


// LayerNorm(512, eps 1e-5, biased variance) + exact GELU, in place; one wave per token
__global__ __launch_bounds__(256) void lg_ln_gelu_kernel(float* hbuf, const int32_t* cnt, int cap, const float* g, const float* be) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  float* row = hbuf + ((size_t)b * cap + i) * 512;
  float v[8], gv[8], bv[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) v[t] = row[lane + 64 * t];
  // gamma / beta are requested with the row: read next to the stores below they are one L2 round trip per element
  // (the compiler cannot move a load above a store through plain float pointers)
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    gv[t] = g[lane + 64 * t];
    bv[t] = be[lane + 64 * t];
  }
  float s = 0.0f;
#pragma unroll
  for (int t = 0; t < 8; ++t) s += v[t];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  const float mean = s / 512.0f;
  float q = 0.0f;
#pragma unroll
  for (int t = 0; t < 8; ++t) q = fmaf(v[t] - mean, v[t] - mean, q);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
  const float rstd = 1.0f / sqrtf(q / 512.0f + 1e-5f);
#pragma unroll
  for (int t = 0; t < 8; ++t) row[lane + 64 * t] = einx_geluf(fmaf((v[t] - mean) * rstd, gv[t], bv[t]));
}

// the same for any row width that is a multiple of 64 (configurations other than d = 256): lane partial sums over
// columns lane, lane + 64, ... ascending, then the same butterfly
__global__ __launch_bounds__(256) void lg_ln_gelu_any_kernel(float* hbuf, const int32_t* cnt, int cap, int width, const float* g, const float* be) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  float* row = hbuf + ((size_t)b * cap + i) * width;
  float s = 0.0f;
  for (int c = lane; c < width; c += 64) s += row[c];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  const float mean = s / (float)width;
  float q = 0.0f;
  for (int c = lane; c < width; c += 64) q = fmaf(row[c] - mean, row[c] - mean, q);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
  const float rstd = 1.0f / sqrtf(q / (float)width + 1e-5f);
  for (int c = lane; c < width; c += 64) row[c] = einx_geluf(fmaf((row[c] - mean) * rstd, g[c], be[c]));
}

// row . w by one wave: lane l adds the columns l, l + 64, ... in ascending order, then the xor butterfly; every lane gets the sum
__device__ __forceinline__ float wave_row_dot(const float* row, const float* w, int d, int lane) {
  float s = 0.0f;
  for (int c = lane; c < d; c += 64) s = fmaf(row[c], w[c], s);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// where a matchability head's weight and bias come from: the model's one head (w, b), or the head entry b's pair stopped at
// (heads[4 h + 2 / 3], see GemmArgs)
struct MatchHead {
  const float *w, *b;
};
__device__ __forceinline__ MatchHead match_head(int, const float* w, const float* bm) { return {w, bm}; }
__device__ __forceinline__ MatchHead match_head(int b, const float* const* heads, const int32_t* stop, int pairs, int nheads) {
  const int h = head_of(stop, pairs, nheads, b);
  return {heads[4 * h + 2], heads[4 * h + 3]};
}

// matchability logit z = x . w + b per token, plus logsigmoid(z) and logsigmoid(-z); Src...: the arguments of a match_head()
template <typename... Src>
__global__ __launch_bounds__(256) void lg_matchability_kernel(const float* x, const int32_t* cnt, int cap, int d, Src... src, float* cert, float* dust) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const MatchHead h = match_head(b, src...);
  const float s = wave_row_dot(x + ((size_t)b * cap + i) * d, h.w, d, lane);
  if (lane == 0) {
    const float z = s + h.b[0];
    cert[(size_t)b * cap + i] = einx_logsigmoidf(z);
    dust[(size_t)b * cap + i] = einx_logsigmoidf(-z);
  }
}

// ------------------------------------------------------------------------------------------
// Early stopping: the layers run on PRIVATE active counts; a pair that stops gets both of them zeroed, and every
// kernel above skips its rows from then on.
// ------------------------------------------------------------------------------------------
constexpr int LG_MAX_HEADS = 32;
struct HeadTable {
  const float* p[4 * LG_MAX_HEADS];  // per layer: final_proj w, b, matchability w, b
};

// the heads' pointers into device memory (the kernels pick an entry by stop[b]), the private counts, stop and the decision's counters
__global__ void lg_es_init_kernel(const HeadTable t, int nheads, const float** heads, const int32_t* n, const int32_t* m, int B, int cap0, int cap1,
                                  int32_t* cnt2, int32_t* act, int32_t* stop, int32_t* below, int32_t* done) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4 * nheads) heads[i] = t.p[i];
  if (i < 2 * B) {
    const int32_t v = i < B ? n[i] : m[i - B];
    cnt2[i] = v;
    act[i] = v;
  }
  if (i < B) {
    stop[i] = (min(n[i], cap0) > 0 && min(m[i], cap1) > 0) ? nheads : 0;
    below[i] = 0;
    done[i] = 0;
  }
}

// The launches behind a non-final layer (the stop decision, the pruning step) run over 2B entries: entry e < B is side 0 of pair
// e, entry e >= B side 1 of pair e - B.
struct Entry {
  bool side;
  int p, cap;
};
__device__ __forceinline__ Entry entry_of(int e, int B, int cap0, int cap1) {
  const bool side = e >= B;
  return {side, side ? e - B : e, side ? cap1 : cap0};
}

// ... and what their argument blocks share
struct TailArgs {
  float *x0, *x1;  // [B,cap0,d], [B,cap1,d] after the layer
  int32_t* act;    // [2B]: the layers' active counts
  int32_t* stop;
  int cap0, cap1, d, B, layer;
  const float *tw, *tb;  // token_confidence[layer].token[0], or null: no stop decision
  float thr;             // the layer's confidence threshold
};

struct StopArgs {
  TailArgs t;
  float depth;
  int32_t *below, *done;       // [B], zero between launches
  const int32_t *tot0, *tot1;  // null, or the caller's counts: the ratio's denominator when rows have been pruned
};

// One launch per non-final layer: a workgroup takes STOP_ROWS rows of an entry (a wave one row at a time: c = sigmoid(x . w + b),
// compared with the layer's threshold in float32).  The workgroups of a
// pair add their integer counts into below[pair] and take a ticket; the one that takes the last ticket has every count, applies
// r = 1 - below / (n + m) > depth_confidence, writes stop and zeroes the pair's active counts, and leaves the counters at zero.
// Integer sums only: the order in which the workgroups arrive does not matter.  Every workgroup with rows has read the counts
// before it takes its ticket, so none can meet the zeroed counts of its own launch; those without rows return either way.
constexpr int STOP_ROWS = 32;
__global__ __launch_bounds__(256) void lg_stop_kernel(const StopArgs a) {
  __shared__ int part[4];
  const TailArgs& t = a.t;
  const Entry en = entry_of(blockIdx.y, t.B, t.cap0, t.cap1);
  const int p = en.p;
  const int n = min(t.act[p], t.cap0), m = min(t.act[t.B + p], t.cap1);
  if (n <= 0 || m <= 0) return;  // stopped earlier, or an empty pair (stop = 0)
  const int rows = en.side ? m : n;
  const int r0 = (int)blockIdx.x * STOP_ROWS;
  if (r0 >= rows) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* x = (en.side ? t.x1 : t.x0) + (size_t)p * en.cap * t.d;
  const float b0 = t.tb[0];
  int below = 0;
  for (int k = 0; k < STOP_ROWS / 4; ++k) {
    const int i = r0 + wave * (STOP_ROWS / 4) + k;
    if (i >= rows) break;
    const float s = wave_row_dot(x + (size_t)i * t.d, t.tw, t.d, lane);
    below += einx_sigmoidf(s + b0) < t.thr ? 1 : 0;
  }
  if (lane == 0) part[wave] = below;
  __syncthreads();
  if (threadIdx.x != 0) return;
  atomicAdd(&a.below[p], part[0] + part[1] + part[2] + part[3]);
  __threadfence();
  const int expected = einx_cdiv(n, STOP_ROWS) + einx_cdiv(m, STOP_ROWS);
  if (atomicAdd(&a.done[p], 1) != expected - 1) return;
  __threadfence();
  const int total = atomicExch(&a.below[p], 0);
  atomicExch(&a.done[p], 0);
  const int den = a.tot0 ? min(a.tot0[p], t.cap0) + min(a.tot1[p], t.cap1) : n + m;  // the reference divides by the ORIGINAL m + n (:635)
  const float r = 1.0f - (float)total / (float)den;
  if (r > a.depth) {
    t.stop[p] = t.layer + 1;
    t.act[p] = 0;
    t.act[t.B + p] = 0;
  }
}

// ------------------------------------------------------------------------------------------
// Point pruning: per pair and side, rows whose matchability head calls them unmatchable leave the network.  The
// survivors are compacted to the front in their order, and the side's active count shrinks: every kernel above skips the rest.
// Per non-final layer, after the stop decision: lg_keep_kernel (the flags), lg_prune_scan_kernel (one workgroup per pair: new
// positions, ind, prune, the counts), lg_prune_gather_kernel (x and the rotary encoding into buffers that are free between
// layers) and lg_prune_copyback_kernel.  Launch boundaries are the only synchronisation; no float atomics, no atomics at all.
// ------------------------------------------------------------------------------------------
struct PruneArgs {
  TailArgs t;          // tw / tb null: no early stopping, no token term
  float *enc0, *enc1;  // [B,cap,2 dh]
  float *tx0, *tx1;    // where the gather puts x: the sides' ctx
  float *te0, *te1;    // ... and the encoding: the sides' h, rows packed at 2 dh floats from each entry's base
  int32_t *live, *prev;    // [2B] each: the surviving rows, the surviving rows before this layer's step
  int32_t *dst0, *dst1;    // [B,cap0], [B,cap1]: the keep flag, then the row's new position or -1
  int64_t *kept0, *kept1;  // ind: position -> original index; -1 past the live count
  float *prune0, *prune1;
  const int32_t *n, *m;  // the caller's counts
  int dh2, min_kpts, set_stop;
  const float *mw, *mb;  // log_assignment[layer].matchability
  float thr_w;
};

// ind = identity, prune = 1 for every original point (0 in the padding), live = prev = the clamped counts
__global__ void lg_prune_init_kernel(const PruneArgs a) {
  const int e = blockIdx.y;
  const Entry en = entry_of(e, a.t.B, a.t.cap0, a.t.cap1);
  const int p = en.p, cap = en.cap;
  const int cnt = max(0, min(en.side ? a.m[p] : a.n[p], cap));
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) {
    a.live[e] = cnt;
    a.prev[e] = cnt;
  }
  if (t >= cap) return;
  (en.side ? a.kept1 : a.kept0)[(size_t)p * cap + t] = t < cnt ? t : -1;
  (en.side ? a.prune1 : a.prune0)[(size_t)p * cap + t] = t < cnt ? 1.0f : 0.0f;
}

// keep = sigmoid(matchability(x)) > thr_w, or (early stopping on) sigmoid(token(x)) <= thr: the dot products in the order of
// lg_matchability_kernel, one wave per row; grid and entries as lg_stop_kernel.  Pairs that have stopped, and sides that do not
// pass the gate (rows > min_kpts), are left alone.
__global__ __launch_bounds__(256) void lg_keep_kernel(const PruneArgs a) {
  const TailArgs& t = a.t;
  const Entry en = entry_of(blockIdx.y, t.B, t.cap0, t.cap1);
  const int p = en.p, cap = en.cap;
  const int n = min(t.act[p], t.cap0), m = min(t.act[t.B + p], t.cap1);
  if (n <= 0 || m <= 0) return;
  const int rows = en.side ? m : n;
  if (rows <= a.min_kpts) return;
  const int r0 = (int)blockIdx.x * STOP_ROWS;
  if (r0 >= rows) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* x = (en.side ? t.x1 : t.x0) + (size_t)p * cap * t.d;
  int32_t* dst = (en.side ? a.dst1 : a.dst0) + (size_t)p * cap;
  for (int k = 0; k < STOP_ROWS / 4; ++k) {
    const int i = r0 + wave * (STOP_ROWS / 4) + k;
    if (i >= rows) break;
    const float* row = x + (size_t)i * t.d;
    bool keep = einx_sigmoidf(wave_row_dot(row, a.mw, t.d, lane) + a.mb[0]) > a.thr_w;
    if (t.tw) {  // low-confidence points are never pruned (lightglue.py:728-729)
      const float c = wave_row_dot(row, t.tw, t.d, lane);
      keep = keep || einx_sigmoidf(c + t.tb[0]) <= t.thr;
    }
    if (lane == 0) dst[i] = keep ? 1 : 0;
  }
}

// One workgroup per pair, its two sides one after the other: an exclusive scan of the flags in chunks of 256 rows gives every kept
// row its new position (stable).  ind is compacted in place -- a chunk is read by every thread before any of it is written, and
// a row only moves forward, into places the earlier chunks have left -- and prune[ind] grows by one for the rows that stay.  Then
// the counts: live = act = the rows kept; a side with no rows left finishes the pair (both active counts zero, stop = layer + 1
// when early stopping is on).  prev keeps what live was, so that the two launches behind this one know which sides moved.
__global__ __launch_bounds__(256) void lg_prune_scan_kernel(const PruneArgs a) {
  __shared__ int wsum[4];
  const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = min(a.t.act[p], a.t.cap0), m = min(a.t.act[a.t.B + p], a.t.cap1);
  if (tid == 0) {
    a.prev[p] = a.live[p];
    a.prev[a.t.B + p] = a.live[a.t.B + p];
  }
  if (n <= 0 || m <= 0) return;  // stopped, finished or empty (uniform over the workgroup)
  int newc[2] = {n, m};
  for (int side = 0; side < 2; ++side) {
    const int rows = side ? m : n, cap = side ? a.t.cap1 : a.t.cap0;
    if (rows <= a.min_kpts) continue;  // the gate: untouched at this layer, prune not incremented
    int32_t* dst = (side ? a.dst1 : a.dst0) + (size_t)p * cap;
    int64_t* kept = (side ? a.kept1 : a.kept0) + (size_t)p * cap;
    float* prune = (side ? a.prune1 : a.prune0) + (size_t)p * cap;
    int run = 0;
    for (int base = 0; base < rows; base += 256) {
      const int i = base + tid;
      const int flag = i < rows ? dst[i] : 0;
      const int64_t src = i < rows ? kept[i] : -1;
      const unsigned long long bal = __ballot(flag != 0);
      const int within = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wsum[wave] = __popcll(bal);
      __syncthreads();
      int off = run, total = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w < wave) off += wsum[w];
        total += wsum[w];
      }
      __syncthreads();
      if (i < rows) {
        dst[i] = flag ? off + within : -1;
        if (flag) {
          kept[off + within] = src;
          prune[src] += 1.0f;
        }
      }
      run += total;
    }
    __syncthreads();
    for (int i = run + tid; i < rows; i += 256) kept[i] = -1;
    newc[side] = run;
  }
  if (tid != 0) return;
  a.live[p] = newc[0];
  a.live[a.t.B + p] = newc[1];
  const bool finished = newc[0] == 0 || newc[1] == 0;
  a.t.act[p] = finished ? 0 : newc[0];
  a.t.act[a.t.B + p] = finished ? 0 : newc[1];
  if (finished && a.set_stop) a.t.stop[p] = a.t.layer + 1;
}

// the rows that stay, of the sides that lost rows at this layer: x -> tx, enc -> te at the new position; one wave per row
__global__ __launch_bounds__(256) void lg_prune_gather_kernel(const PruneArgs a) {
  const int e = blockIdx.y;
  const int old = a.prev[e];
  if (a.live[e] == old) return;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= old) return;
  const Entry en = entry_of(e, a.t.B, a.t.cap0, a.t.cap1);
  const bool side = en.side;
  const int p = en.p, cap = en.cap;
  const int j = (side ? a.dst1 : a.dst0)[(size_t)p * cap + i];
  if (j < 0) return;
  const int lane = threadIdx.x & 63;
  const size_t xb = (size_t)p * cap * a.t.d, eb = (size_t)p * cap * a.dh2;
  const float* xs = (side ? a.t.x1 : a.t.x0) + xb + (size_t)i * a.t.d;
  float* xd = (side ? a.tx1 : a.tx0) + xb + (size_t)j * a.t.d;
  for (int c = lane * 4; c < a.t.d; c += 256) *reinterpret_cast<f32x4*>(xd + c) = *reinterpret_cast<const f32x4*>(xs + c);
  const float* es = (side ? a.enc1 : a.enc0) + eb + (size_t)i * a.dh2;
  float* ed = (side ? a.te1 : a.te0) + (size_t)p * cap * 2 * a.t.d + (size_t)j * a.dh2;
  for (int c = lane * 4; c < a.dh2; c += 256) *reinterpret_cast<f32x4*>(ed + c) = *reinterpret_cast<const f32x4*>(es + c);
}

// ... and back: the first live rows of x and enc (16 bytes per thread; the x part, then the enc part of an entry)
__global__ __launch_bounds__(256) void lg_prune_copyback_kernel(const PruneArgs a) {
  const int e = blockIdx.y;
  const int nw = a.live[e];
  if (nw == a.prev[e]) return;
  const Entry en = entry_of(e, a.t.B, a.t.cap0, a.t.cap1);
  const bool side = en.side;
  const int p = en.p, cap = en.cap;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t xq = (size_t)cap * (a.t.d / 4), eq = (size_t)cap * (a.dh2 / 4);
  if (t < xq) {
    if (t >= (size_t)nw * (a.t.d / 4)) return;
    const size_t o = (size_t)p * cap * a.t.d + t * 4;
    *reinterpret_cast<f32x4*>((side ? a.t.x1 : a.t.x0) + o) = *reinterpret_cast<const f32x4*>((side ? a.tx1 : a.tx0) + o);
  } else if (t - xq < eq) {
    const size_t u = t - xq;
    if (u >= (size_t)nw * (a.dh2 / 4)) return;
    *reinterpret_cast<f32x4*>((side ? a.enc1 : a.enc0) + (size_t)p * cap * a.dh2 + u * 4) =
        *reinterpret_cast<const f32x4*>((side ? a.te1 : a.te0) + (size_t)p * cap * 2 * a.t.d + u * 4);
  }
}

// a packed arg-max key (pack_key, match_tiles.h) back into its index and its value
__device__ __forceinline__ int key_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)); }
__device__ __forceinline__ float key_value(unsigned long long k) { return einx_ordered_unkey((unsigned)(k >> 32)); }

// filter_matches (lightglue.py:402-418) from the packed arg-max keys of the assignment scores
__global__ void lg_finalize_kernel(const unsigned long long* rowkey, const unsigned long long* colkey, const int32_t* nn, const int32_t* mm,
                                   int cap0, int cap1, float th, int64_t* m0, int64_t* m1, float* s0, float* s1) {
  const int b = blockIdx.y;
  const int n = min(nn[b], cap0), m = min(mm[b], cap1);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long* rk = rowkey + (size_t)b * cap0;
  const unsigned long long* ck = colkey + (size_t)b * cap1;
  if (t < cap0) {
    int64_t r = -1;
    float sc = 0.0f;
    if (t < n && m > 0) {
      const int j = key_index(rk[t]);
      const bool mutual = key_index(ck[j]) == t;
      sc = mutual ? einx_expf(key_value(rk[t])) : 0.0f;
      if (mutual && sc > th) r = j;
    }
    m0[(size_t)b * cap0 + t] = r;
    s0[(size_t)b * cap0 + t] = sc;
  }
  if (t < cap1) {
    int64_t r = -1;
    float sc = 0.0f;
    if (t < m && n > 0) {
      const int i = key_index(ck[t]);
      const int back = key_index(rk[i]);
      const bool mutual1 = back == t;
      // mscores1 = mscores0[m1] where mutual1; mscores0[i] is non-zero only if i is mutual too,
      // which is the same condition (back == t  <=>  i's best is t and t's best is i)
      const float ms0 = mutual1 ? einx_expf(key_value(rk[i])) : 0.0f;
      sc = ms0;
      if (mutual1 && ms0 > th) r = i;
    }
    m1[(size_t)b * cap1 + t] = r;
    s1[(size_t)b * cap1 + t] = sc;
  }
}

// The same after point pruning: the keys are those of the LIVE rows, and the results go back to original indexing
// through ind (lightglue.py:659-667).  One workgroup per pair: every row gets -1 / 0 first, then the live rows scatter.
__global__ __launch_bounds__(256) void lg_finalize_scatter_kernel(const unsigned long long* rowkey, const unsigned long long* colkey, const int32_t* live,
                                                                  int B, const int64_t* kept0, const int64_t* kept1, int cap0, int cap1, float th,
                                                                  int64_t* m0, int64_t* m1, float* s0, float* s1) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(live[b], cap0), m = min(live[B + b], cap1);
  m0 += (size_t)b * cap0;
  s0 += (size_t)b * cap0;
  m1 += (size_t)b * cap1;
  s1 += (size_t)b * cap1;
  for (int t = tid; t < cap0; t += 256) {
    m0[t] = -1;
    s0[t] = 0.0f;
  }
  for (int t = tid; t < cap1; t += 256) {
    m1[t] = -1;
    s1[t] = 0.0f;
  }
  __syncthreads();
  if (n <= 0 || m <= 0) return;
  const unsigned long long* rk = rowkey + (size_t)b * cap0;
  const unsigned long long* ck = colkey + (size_t)b * cap1;
  const int64_t* i0 = kept0 + (size_t)b * cap0;
  const int64_t* i1 = kept1 + (size_t)b * cap1;
  for (int t = tid; t < n; t += 256) {
    const int j = key_index(rk[t]);
    const bool mutual = key_index(ck[j]) == t;
    const float sc = mutual ? einx_expf(key_value(rk[t])) : 0.0f;
    m0[i0[t]] = (mutual && sc > th) ? i1[j] : -1;
    s0[i0[t]] = sc;
  }
  for (int t = tid; t < m; t += 256) {
    const int i = key_index(ck[t]);
    const bool mutual1 = key_index(rk[i]) == t;
    const float ms0 = mutual1 ? einx_expf(key_value(rk[i])) : 0.0f;
    m1[i1[t]] = (mutual1 && ms0 > th) ? i0[i] : -1;
    s1[i1[t]] = ms0;
  }
}

// dst_bstride: elements between consecutive batches of dst (cap*width for a plain [B,cap,width] copy)
__global__ void lg_copy_rows_kernel(const float* src, float* dst, const int32_t* cnt, int cap, int width, size_t dst_bstride) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * width) return;
  dst[(size_t)b * dst_bstride + t] = src[(size_t)b * cap * width + t];
}

// normalize_keypoints (lightglue.py:137-148): (kpt - size/2) / (max(size)/2), first two columns
__global__ void lg_normalize_kpts_kernel(const float* kpts, int cols, size_t total, float s0, float s1, float* out, int out_cols) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const float sc = fmaxf(s0, s1) / 2.0f;
  out[t * out_cols + 0] = (kpts[t * cols + 0] - s0 / 2.0f) / sc;
  out[t * out_cols + 1] = (kpts[t * cols + 1] - s1 / 2.0f) / sc;
  for (int c = 2; c < out_cols; ++c) out[t * out_cols + c] = 0.0f;
}

// The three entries share one driver (lg_run): einx_lightglue, einx_lightglue_early_stop and
// einx_lightglue_adaptive (8j: point pruning, with or without the stop decision).  Each mode's workspace is the one before it
// plus a block of its own.
enum LgMode { LG_PLAIN = 0, LG_EARLY_STOP = 1, LG_ADAPTIVE = 2 };

struct LgShape {
  int B, cap0, cap1, d, dh, n_layers;  // d: descriptor_dim, dh: head dim
  // equal capacities (every shipped configuration): the two sides are stacked and every layer runs ONCE over 2B entries --
  // half the launches, and at small batch twice the workgroups per launch (a single pair: 8.0 -> see profiles/r03_notes.md)
  bool stacked() const { return cap0 == cap1; }
};

struct LgWs {
  Side s[2];
  int32_t* cnt2;  // the caller's counts of both sides as [2B] (written when stacked, or by the early-stop init)
  MnnArgs mnn;
  // early stopping
  const float** heads;          // [4 n_layers] device table
  int32_t *act, *below, *done;  // private active counts [2B]; the decision's counters [B] each
  // point pruning
  int32_t *dst0, *dst1;  // [B,cap0], [B,cap1]
  int32_t *prev, *stop;  // [2B]; [B], used when the caller passes no stop
};

// The workspace of all three entries (their size queries walk it from a null base).  Per side the buffers [tokens, d] (x, q, k,
// v, ctx, msg), [tokens, 2 dh] (enc), [tokens, 2 d] (h), [tokens] (cert, dust); then the stacked counts, the assignment stage's
// MNN workspace (match_tiles.h) and 1024 bytes of slack; then the early-stop block, then the pruning block, 256 bytes of slack
// each.  Stacked (equal capacities): every buffer is ONE array [2B, cap, width], side 0 = entries 0..B-1, side 1 = entries
// B..2B-1.  LightGlue applies the same weights to both sides, so every per-side launch becomes one launch over 2B entries (cross
// attention reaches the partner entry B entries on); s[0] / s[1] stay views of the halves.  The array lies in the two regions
// that its halves would take apart, side 1 directly behind side 0's last element: rounding each half up never gives less than the
// whole needs, so the size does not depend on `stacked`.
void carve(WsCarver& c, LgWs& w, LgMode mode, const LgShape& sh) {
  const size_t B = (size_t)sh.B, d = (size_t)sh.d;
  const struct {
    float* Side::*buf;
    size_t width;  // floats per token
  } bufs[] = {{&Side::x, d},   {&Side::enc, (size_t)2 * sh.dh}, {&Side::q, d},     {&Side::k, d},     {&Side::v, d},
              {&Side::ctx, d}, {&Side::msg, d},                 {&Side::h, 2 * d}, {&Side::cert, 1}, {&Side::dust, 1}};
  if (sh.stacked()) {
    for (const auto& b : bufs) {
      const size_t n = B * sh.cap0 * b.width;
      float* both = c.take<float>(n);
      c.take<float>(n);
      w.s[0].*b.buf = both;
      w.s[1].*b.buf = both ? both + n : nullptr;
    }
  } else {
    for (const auto& b : bufs) w.s[0].*b.buf = c.take<float>(B * sh.cap0 * b.width);
    for (const auto& b : bufs) w.s[1].*b.buf = c.take<float>(B * sh.cap1 * b.width);
  }
  w.cnt2 = c.take<int32_t>(2 * B);
  einx_match::carve(c, w.mnn, sh.B, sh.cap0, sh.cap1);
  c.slack(1024);
  if (mode == LG_PLAIN) return;
  w.heads = c.take<const float*>((size_t)4 * sh.n_layers);
  w.act = c.take<int32_t>(2 * B);
  w.below = c.take<int32_t>(B);
  w.done = c.take<int32_t>(B);
  c.slack(256);
  if (mode == LG_EARLY_STOP) return;
  w.dst0 = c.take<int32_t>(B * sh.cap0);
  w.dst1 = c.take<int32_t>(B * sh.cap1);
  w.prev = c.take<int32_t>(2 * B);
  w.stop = c.take<int32_t>(B);
  c.slack(256);
}

__global__ void lg_stack_counts_kernel(const int32_t* n, const int32_t* m, int B, int32_t* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 2 * B) out[t] = t < B ? n[t] : m[t - B];
}

// a layer's Linear: the call on the engine the mode asks for (W16, the fp16 image of c.W, is passed on only under LG_LIN_F16)
int linear(hipStream_t st, const Dims& dm, GemmCall c, const uint16_t* W16) {
  if (dm.lin16 && !W16) return -1;
  c.W16 = dm.lin16 ? W16 : nullptr;
  return launch_gemm(st, c);
}

// fused Wqkv projection + rotary split: X [B,cap,d] -> q, k (rotary applied), v, each [B,cap,d]
int gemm_qkv_rope(hipStream_t st, const Side& s, int B, const Dims& dm, const float* X, const float* Wqkv, const uint16_t* Wqkv16, const float* bqkv,
                  float* q, float* k, float* v) {
  const int d = dm.d;
  GemmCall c = gemm_call(dm.shipped() ? EPI_ROPE : EPI_ROPE_ANY, s, B, X, d, Wqkv, bqkv, 3 * d, nullptr);
  c.ldy = d;
  c.enc = s.enc;
  c.Yq = q, c.Yk = k, c.Yv = v;
  c.d = dm.d, c.dh = dm.dh;
  c.rope_tiles = 3 * einx_cdiv(d, BN) * einx_cdiv(s.cap, BM) * B;
  return linear(st, dm, c, Wqkv16);
}

// ffn(cat[x,msg]) + residual, in place on s.x
int ffn(hipStream_t st, const Side& s, int B, const Dims& dm, const float* msg, const float* w0, const uint16_t* w0h, const float* b0, const float* g,
        const float* be, const float* w3, const uint16_t* w3h, const float* b3) {
  const int d = dm.d;
  // (one fused launch for ffn.0 + LayerNorm + GELU was measured in round 3 and is slower: tools/experiments/lg_ffn0_ln_gelu_kernel.hip.txt)
  GemmCall up = gemm_call(EPI_BIAS, s, B, s.x, 2 * d, w0, b0, 2 * d, s.h);  // K = 2 d: columns 0 .. d - 1 from x, the rest from msg
  up.ldx = d, up.X2 = msg, up.ldx2 = d, up.Ksplit = d;
  if (linear(st, dm, up, w0h)) return -1;
  {
    EINX_PROF("lg_ln_gelu_kernel", st);
    const dim3 lg((unsigned)einx_cdiv(s.cap, 4), (unsigned)B);
    if (2 * d == 512) hipLaunchKernelGGL(lg_ln_gelu_kernel, lg, dim3(256), 0, st, s.h, s.cnt, s.cap, g, be);
    else hipLaunchKernelGGL(lg_ln_gelu_any_kernel, lg, dim3(256), 0, st, s.h, s.cnt, s.cap, 2 * d, g, be);
  }
  if (hipGetLastError() != hipSuccess) return -1;
  return linear(st, dm, gemm_call(EPI_RESID, s, B, s.h, 2 * d, w3, b3, d, s.x), w3h);
}

}  // namespace

EINX_EXPORT int einx_linear(const float* x, int M, int K, const float* w, const float* bias, int N, float* y, int accumulate, void* stream) {
  EINX_CHECK_ARG(x && w && bias && y, "null pointer");
  EINX_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 4 == 0, "bad shape (K must be a multiple of 4)");
  GemmCall c = gemm_call(accumulate ? EPI_RESID : EPI_BIAS, nullptr, M, 1, x, K, w, bias, N, y);
  c.bare = true;
  launch_gemm((hipStream_t)stream, c);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_normalize_keypoints(const float* kpts, int rows, int cols, float h, float w, float* out, int out_cols,
                                         void* stream) {
  EINX_CHECK_ARG(kpts && out, "null pointer");
  EINX_CHECK_ARG(rows > 0 && cols >= 2 && out_cols >= 2, "bad shape");
  hipLaunchKernelGGL(lg_normalize_kpts_kernel, dim3((unsigned)einx_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, kpts, cols,
                     (size_t)rows, h, w, out, out_cols);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

namespace {
// lightglue.py:456-461: head_dim = descriptor_dim // num_heads.  The attention kernel is instantiated for 32-, 64- and 128-wide
// heads; other widths run the next larger one on zero-padded heads (round 6).  Multiples of 4 (16-byte rows of a head; the
// rotary encoding needs an even width anyway) up to 256 (<256, 0>: 256 + 100 registers, one workgroup per SIMD -- rare widths, not tuned).
bool dims_of(int d, int heads, Dims& dm) {
  if (d <= 0 || heads <= 0 || d % heads != 0) return false;
  dm.d = d;
  dm.heads = heads;
  dm.dh = d / heads;
  return dm.dh % 4 == 0 && dm.dh <= 256;
}

// the one launch check of this file; `entry`: the exported function the error is reported under
#define LG_CHECK(entry, expr)                                         \
  do {                                                                \
    if ((expr) != 0 || hipGetLastError() != hipSuccess) {             \
      einx_set_error("%s: kernel launch failed at %s", entry, #expr); \
      return EINX_ERR_LAUNCH;                                         \
    }                                                                 \
  } while (0)
constexpr const char* LG = "einx_lightglue";  // all three modes report under it

size_t lg_ws_bytes(LgMode mode, int B, int cap0, int cap1, int d, int heads, int n_layers) {
  Dims dm;
  if (B <= 0 || cap0 <= 0 || cap1 <= 0 || !dims_of(d, heads, dm)) return 0;
  if (mode != LG_PLAIN && (n_layers < 1 || n_layers > LG_MAX_HEADS)) return 0;
  LgWs w;
  WsCarver c{nullptr};
  carve(c, w, mode, {B, cap0, cap1, d, dm.dh, n_layers});
  return c.bytes;
}
}  // namespace

// (input_dim: part of the ABI; the descriptors are projected in place, so no region depends on it)
EINX_EXPORT size_t einx_lg_ws_bytes_heads(int B, int cap0, int cap1, int d, int heads, int) { return lg_ws_bytes(LG_PLAIN, B, cap0, cap1, d, heads, 0); }

EINX_EXPORT size_t einx_lg_ws_bytes(int B, int cap0, int cap1, int d, int input_dim) {  // 64-wide heads (the LightGlue default)
  return d > 0 && d % 64 == 0 ? einx_lg_ws_bytes_heads(B, cap0, cap1, d, d / 64, input_dim) : 0;
}

EINX_EXPORT size_t einx_lightglue_early_stop_ws_bytes(int B, int cap0, int cap1, int d, int heads, int, int n_layers) {
  return lg_ws_bytes(LG_EARLY_STOP, B, cap0, cap1, d, heads, n_layers);
}

EINX_EXPORT size_t einx_lightglue_adaptive_ws_bytes(int B, int cap0, int cap1, int d, int heads, int, int n_layers) {
  return lg_ws_bytes(LG_ADAPTIVE, B, cap0, cap1, d, heads, n_layers);
}

namespace {
// One run of the matcher as the five exported entries describe it: einx_lightglue, _early_stop, _adaptive fill what they take,
// _flash and _mp everything (lg_dispatch picks the run); lg_run consumes it.
struct EarlyStop {
  const einx_lg_head* heads;
  size_t head_size;
  float depth_confidence;  // with point pruning: <= 0 means no stop decision
  int32_t* stop;           // with point pruning: may be null (carved in the workspace; route (a) reads it either way)
};
struct Adaptive {  // point pruning
  double width_confidence;
  int min_kpts;
  float *prune0, *prune1;
  int64_t *kept0, *kept1;
  int32_t* live;
};
struct LgCall {
  const char* entry;  // the exported function an argument error of the early-stop / adaptive checks is reported under
  unsigned mode;      // LG_ATTN_F16 | LG_LIN_F16
  const einx_lg_weights* w;
  Side in[2];  // kpts, desc, cnt, cap: the caller's; the buffers are carved by lg_run
  int B;
  float size[2][2];  // the images' (h, w)
  void* ws;
  int64_t* matches[2];
  float *scores[2], *la, *ref[2];
  int ref_layers;
  void* stream;
  EarlyStop es;
  Adaptive ad;
  LgMode run;  // which of the three runs: set by lg_early_stop / lg_adaptive, LG_PLAIN otherwise
};

// A set of keypoint counts: side 0 [B], side 1 [B], and the two as one [2B] array (what a launch over stacked sides reads)
struct Counts {
  const int32_t *c0, *c1, *both;
};

// the sides as a shared-weight stage iterates over them: one view of 2B entries (stacked), or two of B
struct Views {
  Side s[2];
  int n, entries;
};

struct LgCtx {
  hipStream_t st;
  const einx_lg_weights* w;
  Dims dm;
  LgShape sh;
  LgMode mode;
  const EarlyStop* es;  // the call's; null: LG_PLAIN
  const Adaptive* ad;   // the call's; null unless LG_ADAPTIVE
  bool decide;          // the stop decision runs (LG_ADAPTIVE: only with depth_confidence > 0)
  int32_t* stop;        // the caller's, or the workspace's; null: LG_PLAIN
  LgWs ws;
  Counts caller, layers, heads;  // see lg_run
  const LgCall* call;            // the image sizes and the outputs are read from it
  bool all_layers;  // ref holds every layer's descriptors (training-mode output)
};

Views views(const LgCtx& c, const Counts& cnt, bool stacked) {
  Views v{{c.ws.s[0], c.ws.s[1]}, stacked ? 1 : 2, stacked ? 2 * c.sh.B : c.sh.B};
  v.s[0].cnt = stacked ? cnt.both : cnt.c0;
  v.s[1].cnt = cnt.c1;
  return v;
}

// confidence_threshold of a layer (lightglue.py:718-722): in double, rounded to float32 once
float confidence_threshold(int li, int n_layers) {
  const double thr = 0.8 + 0.1 * exp(-4.0 * li / n_layers);
  return (float)(thr < 0.0 ? 0.0 : thr > 1.0 ? 1.0 : thr);
}

// li < 0: the init launch, which reads no field of a layer
TailArgs tail_args(const LgCtx& c, int li) {
  TailArgs t{};
  t.x0 = c.ws.s[0].x, t.x1 = c.ws.s[1].x;
  t.act = c.ws.act;
  t.stop = c.stop;
  t.cap0 = c.sh.cap0, t.cap1 = c.sh.cap1, t.d = c.sh.d, t.B = c.sh.B;
  if (li < 0) return t;
  t.layer = li;
  if (c.decide) t.tw = c.es->heads[li].token_w, t.tb = c.es->heads[li].token_b;
  t.thr = confidence_threshold(li, c.w->n_layers);
  return t;
}

PruneArgs prune_args(const LgCtx& c, int li) {
  const Side* s = c.ws.s;
  PruneArgs a{};
  a.t = tail_args(c, li);
  a.enc0 = s[0].enc, a.enc1 = s[1].enc;
  a.tx0 = s[0].ctx, a.tx1 = s[1].ctx, a.te0 = s[0].h, a.te1 = s[1].h;
  a.live = c.ad->live, a.prev = c.ws.prev;
  a.dst0 = c.ws.dst0, a.dst1 = c.ws.dst1;
  a.kept0 = c.ad->kept0, a.kept1 = c.ad->kept1, a.prune0 = c.ad->prune0, a.prune1 = c.ad->prune1;
  a.n = c.caller.c0, a.m = c.caller.c1;
  a.dh2 = 2 * c.sh.dh;
  a.min_kpts = c.ad->min_kpts;
  a.set_stop = c.decide ? 1 : 0;
  a.thr_w = (float)(1.0 - c.ad->width_confidence);
  if (li >= 0) a.mw = c.es->heads[li].match_w, a.mb = c.es->heads[li].match_b;
  return a;
}

// the grid of a launch over 2B entries that gives every workgroup `rows` rows of the longer side
dim3 tail_grid(const LgShape& sh, int rows) { return dim3((unsigned)einx_cdiv(sh.cap0 > sh.cap1 ? sh.cap0 : sh.cap1, rows), (unsigned)(2 * sh.B)); }

template <typename... Src>  // the arguments of a match_head()
void launch_matchability(hipStream_t st, const Side& s, const float* x, int entries, int d, Src... src) {
  hipLaunchKernelGGL(lg_matchability_kernel<Src...>, dim3((unsigned)einx_cdiv(s.cap, 4), (unsigned)entries), dim3(256), 0, st, x, s.cnt, s.cap, d, src...,
                     s.cert, s.dust);
}

// ---- what has to be on the device before the first layer.  Early stopping: the heads' table, the [2B] counts, the private
// counts, stop and the counters in one launch; point pruning: its outputs' start values.  Otherwise the [2B] counts when the
// stacked layers will read them; plain and unstacked: no launch.
int lg_setup(const LgCtx& c) {
  const LgShape& sh = c.sh;
  if (c.es) {
    HeadTable t;
    for (int i = 0; i < sh.n_layers; ++i) {
      t.p[4 * i + 0] = c.es->heads[i].proj_w;
      t.p[4 * i + 1] = c.es->heads[i].proj_b;
      t.p[4 * i + 2] = c.es->heads[i].match_w;
      t.p[4 * i + 3] = c.es->heads[i].match_b;
    }
    const int items = 4 * sh.n_layers > 2 * sh.B ? 4 * sh.n_layers : 2 * sh.B;
    hipLaunchKernelGGL(lg_es_init_kernel, dim3((unsigned)einx_cdiv(items, 256)), dim3(256), 0, c.st, t, sh.n_layers, c.ws.heads, c.caller.c0, c.caller.c1,
                       sh.B, sh.cap0, sh.cap1, c.ws.cnt2, c.ws.act, c.stop, c.ws.below, c.ws.done);
    if (c.ad) hipLaunchKernelGGL(lg_prune_init_kernel, tail_grid(sh, 256), dim3(256), 0, c.st, prune_args(c, -1));
  } else if (sh.stacked()) {
    hipLaunchKernelGGL(lg_stack_counts_kernel, dim3((unsigned)einx_cdiv(2 * sh.B, 256)), dim3(256), 0, c.st, c.caller.c0, c.caller.c1, sh.B, c.ws.cnt2);
  }
  LG_CHECK(LG, 0);
  return EINX_OK;
}

// ---- input projection (or copy) + positional encodings (per side: own inputs, own image size)
int lg_input(const LgCtx& c) {
  const einx_lg_weights* w = c.w;
  const int B = c.sh.B, d = c.sh.d, dh = c.sh.dh;
  const Views v = views(c, c.caller, false);
  for (int sd = 0; sd < 2; ++sd) {
    const Side& s = v.s[sd];
    if (w->in_w) {
      LG_CHECK(LG, launch_gemm(c.st, gemm_call(EPI_BIAS, s, B, s.desc, w->input_dim, w->in_w, w->in_b, d, s.x)));
    } else {
      const size_t per = (size_t)s.cap * d;
      hipLaunchKernelGGL(lg_copy_rows_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)B), dim3(256), 0, c.st, s.desc, s.x, s.cnt, s.cap, d, per);
      LG_CHECK(LG, 0);
    }
    hipLaunchKernelGGL(lg_posenc_kernel, dim3((unsigned)einx_cdiv(s.cap * (dh / 2), 256), (unsigned)B), dim3(256), 0, c.st, s.kpts, s.cnt, s.cap,
                       c.call->size[sd][0], c.call->size[sd][1], w->Wr, s.enc, dh);
    LG_CHECK(LG, 0);
  }
  return EINX_OK;
}

// ---- one transformer layer: SelfBlock, then CrossBlock
int lg_layer(const LgCtx& c, int li) {
  const einx_lg_layer& L = c.w->layers[li];
  const Dims& dm = c.dm;
  hipStream_t st = c.st;
  const int B = c.sh.B, d = c.sh.d;
  const Views v = views(c, c.layers, c.sh.stacked());
  const int E = v.entries;
  for (int sd = 0; sd < v.n; ++sd) {
    const Side& s = v.s[sd];
    LG_CHECK(LG, gemm_qkv_rope(st, s, E, dm, s.x, L.Wqkv, L.Wqkv_h, L.bqkv, s.q, s.k, s.v));
    LG_CHECK(LG, launch_attn(st, attn_call(dm, E, s.q, s.cnt, s.cap, s.k, s.v, s.cnt, s.cap, s.ctx)));
    // (no Wo: out_proj is folded into the FFN's first Linear at load time, message = context)
    if (L.Wo) LG_CHECK(LG, linear(st, dm, gemm_call(EPI_BIAS, s, E, s.ctx, d, L.Wo, L.bo, d, s.msg), L.Wo_h));
    LG_CHECK(LG, ffn(st, s, E, dm, L.Wo ? s.msg : s.ctx, L.sf0_w, L.sf0_h, L.sf0_b, L.sln_g, L.sln_b, L.sf3_w, L.sf3_h, L.sf3_b));
  }
  // to_qk and to_v read the same rows: with the merged weight image [Wqk; Wv] (shipped widths) they are ONE launch writing
  // qk | v side by side into the FFN's hidden buffer (free until ffn.0 runs), and the attention reads them at row stride 2 d --
  // the same k-ordered chain and bias per output, one launch less per layer
  const bool merged = L.Wqk_v && L.bqk_v && dm.shipped() && (!dm.lin16 || L.Wqk_v_h);
  for (int sd = 0; sd < v.n; ++sd) {
    const Side& s = v.s[sd];
    if (merged) {
      LG_CHECK(LG, linear(st, dm, gemm_call(EPI_BIAS, s, E, s.x, d, L.Wqk_v, L.bqk_v, 2 * d, s.h), L.Wqk_v_h));
    } else {
      LG_CHECK(LG, linear(st, dm, gemm_call(EPI_BIAS, s, E, s.x, d, L.Wqk, L.bqk, d, s.q), L.Wqk_h));
      LG_CHECK(LG, linear(st, dm, gemm_call(EPI_BIAS, s, E, s.x, d, L.Wv, L.bv, d, s.v), L.Wv_h));
    }
  }
  // side a's queries against side b's keys / values, over `entries` entries (merged: column blocks of the sides' h, row stride 2 d)
  auto cross = [&](const Side& a, const Side& b, int entries, int kv_shift) {
    AttnCall ac = merged ? attn_call(dm, entries, a.h, a.cnt, a.cap, b.h, b.h + d, b.cnt, b.cap, a.ctx)
                         : attn_call(dm, entries, a.q, a.cnt, a.cap, b.q, b.v, b.cnt, b.cap, a.ctx);
    ac.kv_shift = kv_shift;
    if (merged) ac.ld = 2 * d;
    return launch_attn(st, ac);
  };
  const Side &r0 = v.s[0], &r1 = v.s[1];
  if (v.n == 1) {  // stacked: entry b attends to the keys / values of its partner entry (b + B) mod 2B
    LG_CHECK(LG, cross(r0, r0, E, B));
  } else {
    LG_CHECK(LG, cross(r0, r1, B, 0));
    LG_CHECK(LG, cross(r1, r0, B, 0));
  }
  for (int sd = 0; sd < v.n; ++sd) {
    const Side& s = v.s[sd];
    if (L.Wco) LG_CHECK(LG, linear(st, dm, gemm_call(EPI_BIAS, s, E, s.ctx, d, L.Wco, L.bco, d, s.msg), L.Wco_h));
    LG_CHECK(LG, ffn(st, s, E, dm, L.Wco ? s.msg : s.ctx, L.cf0_w, L.cf0_h, L.cf0_b, L.cln_g, L.cln_b, L.cf3_w, L.cf3_h, L.cf3_b));
  }
  return EINX_OK;
}

// ---- ref_descriptors: x of both sides, rows below `cnt`, into slot `slot` of `slots` per pair (lightglue.py:626-629)
int lg_ref_copy(const LgCtx& c, const Counts& cnt, int slot, int slots) {
  const Views v = views(c, cnt, false);
  for (int sd = 0; sd < 2; ++sd) {
    const Side& s = v.s[sd];
    if (!c.call->ref[sd]) continue;
    const size_t per = (size_t)s.cap * c.sh.d;
    hipLaunchKernelGGL(lg_copy_rows_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)c.sh.B), dim3(256), 0, c.st, s.x, c.call->ref[sd] + (size_t)slot * per,
                       s.cnt, s.cap, c.sh.d, per * (size_t)slots);
    LG_CHECK(LG, 0);
  }
  return EINX_OK;
}

// ---- the pairs still running decide whether layer li was their last
int lg_stop(const LgCtx& c, int li) {
  StopArgs a{};
  a.t = tail_args(c, li);
  a.depth = c.es->depth_confidence;
  a.below = c.ws.below;
  a.done = c.ws.done;
  if (c.ad) a.tot0 = c.caller.c0, a.tot1 = c.caller.c1;
  EINX_PROF("lg_stop_kernel", c.st);
  hipLaunchKernelGGL(lg_stop_kernel, tail_grid(c.sh, STOP_ROWS), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  return EINX_OK;
}

// ---- point pruning behind layer li, after the stop decision (lightglue.py:632-652): a pair that has just stopped is not pruned
int lg_prune(const LgCtx& c, int li) {
  const LgShape& sh = c.sh;
  const PruneArgs a = prune_args(c, li);
  EINX_PROF("lg_prune (keep + scan + gather + copy back)", c.st);
  hipLaunchKernelGGL(lg_keep_kernel, tail_grid(sh, STOP_ROWS), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  hipLaunchKernelGGL(lg_prune_scan_kernel, dim3((unsigned)sh.B), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  hipLaunchKernelGGL(lg_prune_gather_kernel, tail_grid(sh, 4), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  const size_t quads = (size_t)(sh.cap0 > sh.cap1 ? sh.cap0 : sh.cap1) * ((sh.d + 2 * sh.dh) / 4);
  hipLaunchKernelGGL(lg_prune_copyback_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)(2 * sh.B)), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  return EINX_OK;
}

// ---- MatchAssignment's inputs (lightglue.py:365-377): final_proj / d^(1/4) and the matchability terms.  Early stopping, route
// (a): one stage over every pair's own rows, each pair with the head it stopped at (x frozen since then)
int lg_assign_heads(const LgCtx& c) {
  const einx_lg_weights* w = c.w;
  const int d = c.sh.d;
  const float div = sqrtf(sqrtf((float)d));
  const Views v = views(c, c.heads, c.sh.stacked());
  for (int sd = 0; sd < v.n; ++sd) {
    const Side& s = v.s[sd];
    GemmCall proj = gemm_call(c.es ? EPI_DIV_HEAD : EPI_DIV, s, v.entries, s.x, d, c.es ? nullptr : w->proj_w, c.es ? nullptr : w->proj_b, d, s.q);
    proj.div = div;
    if (c.es) proj.heads = c.ws.heads, proj.stop = c.stop, proj.pairs = c.sh.B, proj.nheads = c.sh.n_layers;  // W / bias: the head table's
    LG_CHECK(LG, launch_gemm(c.st, proj));
    if (c.es) launch_matchability(c.st, s, s.x, v.entries, d, c.ws.heads, c.stop, c.sh.B, c.sh.n_layers);
    else launch_matchability(c.st, s, s.x, v.entries, d, w->match_w, w->match_b);
    LG_CHECK(LG, 0);
  }
  return EINX_OK;
}

dim3 assign_grid(const MnnArgs& a, int B) { return dim3((unsigned)einx_cdiv(a.cap1, BN), (unsigned)einx_cdiv(a.cap0, BM), (unsigned)B); }

// The first half of every assignment: the MNN argument block from the two sides (q, cert, dust) and a pair of counts, then the
// softmax statistics (first tile pass) and their reduction.  The caller opens the profile scope and runs its own second pass.
int assign_prologue(const char* entry, hipStream_t st, MnnArgs& a, const Side& s0, const Side& s1, const int32_t* n, const int32_t* m, int B, int d,
                    float* la) {
  a.d0 = s0.q;
  a.d1 = s1.q;
  a.n = n;
  a.m = m;
  a.cap0 = s0.cap;
  a.cap1 = s1.cap;
  a.D = d;
  a.la = la;
  a.cert0 = s0.cert;
  a.cert1 = s1.cert;
  a.dust0 = s0.dust;
  a.dust1 = s1.dust;
  const int mx = a.cap0 > a.cap1 ? a.cap0 : a.cap1;
  hipLaunchKernelGGL((mnn_tile_kernel<1, false>), assign_grid(a, B), dim3(THREADS), 0, st, a);
  LG_CHECK(entry, 0);
  hipLaunchKernelGGL(mnn_lse_kernel, dim3((unsigned)einx_cdiv(mx + 1, 256), (unsigned)B), dim3(256), 0, st, a);
  LG_CHECK(entry, 0);
  return EINX_OK;
}

// ---- assignment scores, their arg-max keys, filter_matches
int lg_assign(const LgCtx& c) {
  const LgShape& sh = c.sh;
  hipStream_t st = c.st;
  MnnArgs a = c.ws.mnn;
  if (hipMemsetAsync(a.rowkey, 0, (char*)a.rowstat - (char*)a.rowkey, st) != hipSuccess) {  // rowkey | colkey
    einx_set_error("einx_lightglue: memset failed");
    return EINX_ERR_LAUNCH;
  }
  EINX_PROF("lg_assignment (3 tile passes + lse + finalize)", st);
  if (const int rc = assign_prologue(LG, st, a, c.ws.s[0], c.ws.s[1], c.heads.c0, c.heads.c1, sh.B, sh.d, c.call->la)) return rc;
  if (c.call->la) hipLaunchKernelGGL((mnn_tile_kernel<6, true>), assign_grid(a, sh.B), dim3(THREADS), 0, st, a);  // arg-max + log_assignment write in one visit
  else hipLaunchKernelGGL((mnn_tile_kernel<0, true>), assign_grid(a, sh.B), dim3(THREADS), 0, st, a);
  LG_CHECK(LG, 0);
  if (c.ad) {  // the keys are those of the live rows: back to original indexing
    hipLaunchKernelGGL(lg_finalize_scatter_kernel, dim3((unsigned)sh.B), dim3(256), 0, st, a.rowkey, a.colkey, c.heads.both, sh.B, c.ad->kept0,
                       c.ad->kept1, sh.cap0, sh.cap1, c.w->filter_threshold, c.call->matches[0], c.call->matches[1], c.call->scores[0], c.call->scores[1]);
  } else {
    const int mx = sh.cap0 > sh.cap1 ? sh.cap0 : sh.cap1;
    hipLaunchKernelGGL(lg_finalize_kernel, dim3((unsigned)einx_cdiv(mx, 256), (unsigned)sh.B), dim3(256), 0, st, a.rowkey, a.colkey, c.heads.c0, c.heads.c1,
                       sh.cap0, sh.cap1, c.w->filter_threshold, c.call->matches[0], c.call->matches[1], c.call->scores[0], c.call->scores[1]);
  }
  LG_CHECK(LG, 0);
  return EINX_OK;
}

int lg_run(const LgCall& call) {
  const einx_lg_weights* w = call.w;
  const Side &in0 = call.in[0], &in1 = call.in[1];
  const int B = call.B, ref_layers = call.ref_layers;
  EINX_CHECK_ARG(w && in0.kpts && in0.desc && in0.cnt && in1.kpts && in1.desc && in1.cnt && call.ws && call.matches[0] && call.matches[1] &&
                     call.scores[0] && call.scores[1],
                 "null pointer");
  Dims dm;
  EINX_CHECK_ARG(dims_of(w->d, w->heads, dm), "descriptor_dim must be num_heads x head_dim with head_dim a multiple of 4, at most 256");
  EINX_CHECK_ARG(w->struct_size == sizeof(einx_lg_weights) && w->layer_size == sizeof(einx_lg_layer),
                 "einx_lg_weights::struct_size / layer_size do not match this library (header / library ABI mismatch)");
  EINX_CHECK_ARG(w->n_layers >= 1 && w->layers, "no layers");
  EINX_CHECK_ARG(B > 0 && in0.cap > 0 && in1.cap > 0, "bad shape");
  EINX_CHECK_ARG(w->input_dim % 4 == 0 && w->input_dim > 0, "input_dim must be a multiple of 4");
  EINX_CHECK_ARG((w->input_dim == dm.d) == (w->in_w == nullptr), "input_proj must be given exactly when input_dim != d");
  EINX_CHECK_ARG(ref_layers == 0 || ref_layers == 1 || ref_layers == w->n_layers, "ref_layers must be 0/1 (last layer) or n_layers");
  LgCtx c{};
  c.st = (hipStream_t)call.stream;
  c.w = w;
  c.dm = dm;
  c.dm.flash = (call.mode & LG_ATTN_F16) != 0;
  c.dm.lin16 = (call.mode & LG_LIN_F16) != 0;
  c.sh = {B, in0.cap, in1.cap, dm.d, dm.dh, w->n_layers};
  c.mode = call.run;
  const EarlyStop* es = c.es = call.run != LG_PLAIN ? &call.es : nullptr;
  c.ad = call.run == LG_ADAPTIVE ? &call.ad : nullptr;
  WsCarver wc{(char*)call.ws};
  carve(wc, c.ws, c.mode, c.sh);
  c.call = &call;
  for (int sd = 0; sd < 2; ++sd) c.ws.s[sd].kpts = call.in[sd].kpts, c.ws.s[sd].desc = call.in[sd].desc, c.ws.s[sd].cap = call.in[sd].cap;
  // caller: the input stage and the all-layers ref copy; with pruning also the stop ratio's denominator
  // layers: the transformer layers; the stop decision zeroes a pair's, the pruning step shrinks them with the rows kept
  // heads:  the assignment heads, the last-layer ref copy, the assignment and filter_matches: what survived, also of a stopped pair
  c.caller = {in0.cnt, in1.cnt, c.ws.cnt2};
  c.layers = c.heads = c.caller;
  if (es) c.layers = {c.ws.act, c.ws.act + B, c.ws.act};
  if (c.ad) c.heads = {c.ad->live, c.ad->live + B, c.ad->live};
  if (es) c.stop = es->stop ? es->stop : c.ws.stop;
  c.decide = es && (!c.ad || es->depth_confidence > 0.0f);
  c.all_layers = ref_layers > 1;

  int rc = lg_setup(c);
  if (!rc) rc = lg_input(c);
  for (int li = 0; li < w->n_layers && !rc; ++li) {
    const bool last = li == w->n_layers - 1;
    rc = lg_layer(c, li);
    if (!rc && c.all_layers) rc = lg_ref_copy(c, c.caller, li, w->n_layers);
    if (!rc && c.decide && !last) rc = lg_stop(c, li);
    if (!rc && c.ad && !last) rc = lg_prune(c, li);
  }
  if (!rc) rc = lg_assign_heads(c);
  if (!rc && !c.all_layers) rc = lg_ref_copy(c, c.heads, 0, 1);
  if (!rc) rc = lg_assign(c);
  return rc;
}

// What is wrong with the heads of an early-stop or adaptive call, or null; in the order the entries have always checked: the
// struct's size, the layer count, the entry's complaint about its own scalars (`own`, or null), every layer's heads.  token_msg:
// the complaint about a missing token_confidence head, or null when none is needed.
const char* heads_error(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, const char* layers_msg, const char* own,
                        const char* token_msg) {
  if (head_size != sizeof(einx_lg_head)) return "head_size does not match this library's einx_lg_head (header / library ABI mismatch)";
  if (w->n_layers < 1 || w->n_layers > LG_MAX_HEADS) return layers_msg;
  if (own) return own;
  for (int i = 0; i < w->n_layers; ++i) {
    const einx_lg_head& h = heads[i];
    if (!(h.proj_w && h.proj_b && h.match_w && h.match_b)) return "every layer needs its log_assignment head";
    if (token_msg && i < w->n_layers - 1 && !(h.token_w && h.token_b)) return token_msg;
  }
  return nullptr;
}

// the early-stop and adaptive runs: their own argument checks, reported under the exported entry, then the shared body
#define LG_CHECK_ARG(cond, msg)                \
  do {                                         \
    if (!(cond)) {                             \
      einx_set_error("%s: %s", c.entry, msg);  \
      return EINX_ERR_ARG;                     \
    }                                          \
  } while (0)
int lg_early_stop(LgCall c) {
  LG_CHECK_ARG(c.w && c.es.heads && c.es.stop, "null pointer");
  const char* bad = heads_error(c.w, c.es.heads, c.es.head_size, "early stopping takes 1..32 layers", nullptr,
                                "every layer but the last needs its token_confidence head");
  LG_CHECK_ARG(!bad, bad);
  c.run = LG_EARLY_STOP;
  c.ref_layers = 1;
  return lg_run(c);
}

int lg_adaptive(LgCall c) {
  const Adaptive& ad = c.ad;
  LG_CHECK_ARG(c.w && c.es.heads && ad.prune0 && ad.prune1 && ad.kept0 && ad.kept1 && ad.live, "null pointer");
  const char* own = nullptr;
  if (c.la) own = "log_assignment is not produced with point pruning (DESIGN.md 8j): la must be null";
  if (!(ad.width_confidence > 0.0 && ad.width_confidence <= 1.0)) own = "width_confidence must be in (0, 1]";
  const char* token_msg =
      c.es.depth_confidence <= 0.0f ? nullptr : "with depth_confidence > 0 every layer but the last needs its token_confidence head";
  const char* bad = heads_error(c.w, c.es.heads, c.es.head_size, "point pruning takes 1..32 layers", own, token_msg);
  LG_CHECK_ARG(!bad, bad);
  c.run = LG_ADAPTIVE;
  c.la = nullptr;
  c.ref_layers = 1;
  return lg_run(c);
}

// einx_lightglue_flash / _mp: width_confidence > 0: the adaptive run; else depth_confidence > 0: the early-stop run; else the plain
// run (heads, stop and the pruning outputs unread)
int lg_dispatch(const LgCall& c) {
  if (c.ad.width_confidence > 0.0) {
    LG_CHECK_ARG(c.ref_layers == 0 || c.ref_layers == 1, "point pruning returns the surviving rows, not every layer's: ref_layers must be 0 or 1");
    return lg_adaptive(c);
  }
  if (c.es.depth_confidence > 0.0f) {
    LG_CHECK_ARG(c.ref_layers == 0 || c.ref_layers == 1, "early stopping returns the rows the stopping head read: ref_layers must be 0 or 1");
    return lg_early_stop(c);
  }
  return lg_run(c);
}
}  // namespace

// What every entry fills the same way, from parameters that carry the same names in all five: the reporting name, the mode bits,
// the weights, the two sides, the sizes, the workspace and the outputs; the entry then adds ref_layers, the stream and its options
#define LG_CALL(mode) \
  __func__, mode, w, {{kpts0, desc0, n, cap0}, {kpts1, desc1, m, cap1}}, B, {{h0, w0}, {h1, w1}}, ws, {matches0, matches1}, \
      {scores0, scores1}, la, {ref0, ref1}

EINX_EXPORT int einx_lightglue(const einx_lg_weights* w, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                               const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1,
                               float w1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la,
                               float* ref0, float* ref1, int ref_layers, void* stream) {
  return lg_run({LG_CALL(0), ref_layers, stream});
}

EINX_EXPORT int einx_lightglue_early_stop(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                          const float* kpts0, const float* desc0, const int32_t* n, int cap0, const float* kpts1,
                                          const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1, float w1, void* ws,
                                          int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, float* ref0,
                                          float* ref1, int32_t* stop, void* stream) {
  LgCall c{LG_CALL(0), 1, stream};
  c.es = {heads, head_size, depth_confidence, stop};
  return lg_early_stop(c);
}

EINX_EXPORT int einx_lightglue_adaptive(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                        double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                                        const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1,
                                        float w1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la,
                                        float* ref0, float* ref1, int32_t* stop, float* prune0, float* prune1, int64_t* kept0, int64_t* kept1,
                                        int32_t* live, void* stream) {
  LgCall c{LG_CALL(0), 1, stream};
  c.es = {heads, head_size, depth_confidence, stop};
  c.ad = {width_confidence, min_kpts, prune0, prune1, kept0, kept1, live};
  return lg_adaptive(c);
}

// conf.flash: the three runs above with every attention in fp16 on the matrix cores (lg_dispatch picks the run).
EINX_EXPORT size_t einx_lightglue_flash_ws_bytes(int B, int cap0, int cap1, int d, int heads, int, int n_layers) {
  // the kernel needs no region of its own: the largest carve of the three runs; a layer count only the plain run takes: its carve
  const size_t adaptive = lg_ws_bytes(LG_ADAPTIVE, B, cap0, cap1, d, heads, n_layers);
  return adaptive ? adaptive : lg_ws_bytes(LG_PLAIN, B, cap0, cap1, d, heads, 0);
}

EINX_EXPORT int einx_lightglue_flash(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                     double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                                     const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1,
                                     float w1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la,
                                     float* ref0, float* ref1, int ref_layers, int32_t* stop, float* prune0, float* prune1, int64_t* kept0,
                                     int64_t* kept1, int32_t* live, void* stream) {
  LgCall c{LG_CALL(LG_ATTN_F16), ref_layers, stream};
  c.es = {heads, head_size, depth_confidence, stop};
  c.ad = {width_confidence, min_kpts, prune0, prune1, kept0, kept1, live};
  return lg_dispatch(c);
}

// conf.mp: the same three runs with the precision modes as bits.  EINX_LG_LIN_F16: the nine linears of every layer on
// the f16 tile engine (inputs and weights rounded to binary16, fp32 accumulation, fp32 bias, fp32 result); EINX_LG_ATTN_F16: the
// attention of einx_lightglue_flash.  mode == 0 is einx_lightglue / _early_stop / _adaptive, mode == EINX_LG_ATTN_F16 is _flash.
EINX_EXPORT size_t einx_lightglue_mp_ws_bytes(int B, int cap0, int cap1, int d, int heads, int input_dim, int n_layers) {
  return einx_lightglue_flash_ws_bytes(B, cap0, cap1, d, heads, input_dim, n_layers);  // neither kernel needs a region of its own
}

EINX_EXPORT int einx_lightglue_mp(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                  double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                                  const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1, float w1,
                                  void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, float* ref0,
                                  float* ref1, int ref_layers, int32_t* stop, float* prune0, float* prune1, int64_t* kept0, int64_t* kept1,
                                  int32_t* live, int mode, void* stream) {
  EINX_CHECK_ARG(w, "null pointer");
  EINX_CHECK_ARG((mode & ~(LG_ATTN_F16 | LG_LIN_F16)) == 0, "mode takes EINX_LG_ATTN_F16 | EINX_LG_LIN_F16 only");
  if (mode & LG_LIN_F16) {  // the contract rounds the weights as written: no folded out_proj / to_out, and every linear's fp16 image
    EINX_CHECK_ARG(w->struct_size == sizeof(einx_lg_weights) && w->layer_size == sizeof(einx_lg_layer),
                   "einx_lg_weights::struct_size / layer_size do not match this library (header / library ABI mismatch)");
    EINX_CHECK_ARG(w->n_layers >= 1 && w->layers, "no layers");
    for (int li = 0; li < w->n_layers; ++li) {
      const einx_lg_layer& L = w->layers[li];
      EINX_CHECK_ARG(L.Wo && L.bo && L.Wco && L.bco, "linears in fp16 take unfolded weights: every layer needs Wo / bo / Wco / bco");
      EINX_CHECK_ARG(L.Wqkv_h && L.Wo_h && L.sf0_h && L.sf3_h && L.Wqk_h && L.Wv_h && L.Wco_h && L.cf0_h && L.cf3_h,
                     "linears in fp16 need the binary16 image of every layer's nine weights");
    }
  }
  LgCall c{LG_CALL((unsigned)mode), ref_layers, stream};
  c.es = {heads, head_size, depth_confidence, stop};
  c.ad = {width_confidence, min_kpts, prune0, prune1, kept0, kept1, live};
  return lg_dispatch(c);
}

// The linear of conf.mp alone (a test hook): Y[b, i, :] (+)= RN16(cat(X[b, i, :Ksplit], X2[b, i, :K - Ksplit])) @ W16^T + bias for the
// first min(cnt[b], cap) rows of entry b (cnt null: cap rows); rows past the count are not written.
EINX_EXPORT int einx_lg_linear_f16(const float* X, const float* X2, int Ksplit, int K, const uint16_t* W16, const float* bias, int N, float* Y, int ldy,
                                   const float* resid, const int32_t* cnt, int cap, int B, int epi, void* stream) {
  EINX_CHECK_ARG(X && W16 && bias && Y, "null pointer");
  EINX_CHECK_ARG(B > 0 && cap > 0 && N > 0 && K > 0 && K % 4 == 0, "bad shape (K must be a multiple of 4)");
  EINX_CHECK_ARG(ldy >= N, "ldy must be at least N");
  EINX_CHECK_ARG(!X2 || (Ksplit > 0 && Ksplit < K && Ksplit % einx_gemm16::BK == 0), "Ksplit must be a multiple of the 32-deep K slab inside (0, K)");
  EINX_CHECK_ARG(epi == 0 || epi == 1, "epi must be 0 (bias) or 1 (bias + residual)");
  EINX_CHECK_ARG(epi == 1 || resid == nullptr, "resid is read by epi 1 only: with epi 0 it must be null");
  EINX_CHECK_ARG(epi == 0 || resid == nullptr || resid == Y, "the residual is accumulated in place: resid must be Y (or null)");
  GemmCall c = gemm_call(epi ? EPI_RESID : EPI_BIAS, cnt, cap, B, X, K, nullptr, bias, N, Y);
  c.W16 = W16;
  c.ldy = ldy;
  if (X2) c.ldx = Ksplit, c.X2 = X2, c.ldx2 = K - Ksplit, c.Ksplit = Ksplit;
  if (launch_gemm((hipStream_t)stream, c) != 0) {
    einx_set_error("einx_lg_linear_f16: kernel launch failed");
    return EINX_ERR_LAUNCH;
  }
  return EINX_OK;
}

// The attention of conf.flash alone (a test hook): O[b, q, h dh ..] = RN16(softmax_j(RN16(Q_h[q]) . RN16(K_h[j]) / sqrt(dh)) RN16(V_h[j]))
// for the first nq[b] rows of entry b over the first nk[bk] keys of entry bk = (b + kv_shift) mod B.  Q / K / V: fp32 [B, cap, ld]
// (the heads' columns start at 0; ld >= heads * dh, a multiple of 4), O: fp32 [B, capq, heads * dh]; rows past nq are not written.
EINX_EXPORT int einx_lg_attention_f16(const float* Q, const float* K, const float* V, float* O, const int32_t* nq, const int32_t* nk, int capq,
                                      int capk, int B, int heads, int dh, int ld, int kv_shift, void* stream) {
  EINX_CHECK_ARG(Q && K && V && O && nq && nk, "null pointer");
  EINX_CHECK_ARG(B > 0 && capq > 0 && capk > 0, "bad shape");
  Dims dm;
  EINX_CHECK_ARG(heads > 0 && dh > 0 && dims_of(heads * dh, heads, dm), "head_dim must be a multiple of 4, at most 256");
  EINX_CHECK_ARG(ld >= dm.d && ld % 4 == 0, "ld must be a multiple of 4, at least heads x head_dim");
  EINX_CHECK_ARG(kv_shift >= 0 && kv_shift < B, "kv_shift must be in [0, B)");
  AttnCall c = attn_call(dm, B, Q, nq, capq, K, V, nk, capk, O);
  c.ld = ld, c.kv_shift = kv_shift;
  c.f16 = true;
  if (launch_attn((hipStream_t)stream, c) != 0) {
    einx_set_error("einx_lg_attention_f16: kernel launch failed");
    return EINX_ERR_LAUNCH;
  }
  return EINX_OK;
}

// ------------------------------------------------------------------------------------------
// Assignment NLL of one MatchAssignment head (lightglue.py:66-133, :751-769): the sums behind NLLLoss and
// row_norm without a log_assignment matrix.
// ------------------------------------------------------------------------------------------
namespace {

struct NllWs {
  Side s0, s1;  // q (projected descriptors), cert, dust
};

// einx_lg_assign_nll's workspace (einx_lg_assign_nll_ws_bytes walks it from a null base): per side the projected descriptors
// [B,cap,d] and cert / dust [B,cap]; the matcher's workspace (match_tiles.h); the per-chunk partial sums [B,cap0,nc64,3]; slack.
void carve_nll(WsCarver& c, NllWs& w, MnnArgs& a, int B, int cap0, int cap1, int d) {
  w.s0.q = c.take<float>((size_t)B * cap0 * d);
  w.s1.q = c.take<float>((size_t)B * cap1 * d);
  w.s0.cert = c.take<float>((size_t)B * cap0);
  w.s0.dust = c.take<float>((size_t)B * cap0);
  w.s1.cert = c.take<float>((size_t)B * cap1);
  w.s1.dust = c.take<float>((size_t)B * cap1);
  einx_match::carve(c, a, B, cap0, cap1);
  a.nllstat = c.take<float>((size_t)B * cap0 * a.nc64 * 3);
  c.slack(256);
}

constexpr int NLL_OUT = 8;  // S_pos, num_pos, S_neg0, num_neg0, S_neg1, num_neg1, sum of the row sums of exp, n

// One workgroup per pair.  A thread adds its rows (i = tid, tid + 256, ...) in ascending order, each row's chunk partials in
// ascending chunk order, then its columns; the threads' sums meet as in loss.hip: lane l of wave 0 adds the LDS entries l,
// l + 64, ... in order, then the xor butterfly.  float64 throughout, one fixed order: two calls give the same bits.
__global__ __launch_bounds__(256) void lg_nll_finish_kernel(const MnnArgs a, const int64_t* gt0, const int64_t* gt1, double* out) {
  __shared__ double red[7 * 256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = max(0, min(a.n[b], a.cap0)), m = max(0, min(a.m[b], a.cap1));
  double* o = out + (size_t)b * NLL_OUT;
  if (n == 0 || m == 0) {  // no assignment to speak of: zeros (uniform over the workgroup)
    if (tid < NLL_OUT) o[tid] = 0.0;
    return;
  }
  const int chunks = (m + 63) / 64;
  double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += 256) {
    const float* st = a.nllstat + ((size_t)b * a.cap0 + i) * a.nc64 * 3;
    double e = 0.0, sw = 0.0, cw = 0.0;
    for (int c = 0; c < chunks; ++c) {
      e += (double)st[3 * c];
      sw += (double)st[3 * c + 1];
      cw += (double)st[3 * c + 2];
    }
    const float d0 = a.dust0[(size_t)b * a.cap0 + i];
    v[0] += sw;
    v[1] += cw;
    v[6] += e + exp((double)d0);  // the dustbin column belongs to row_norm (:769)
    if (gt0[(size_t)b * a.cap0 + i] == -1) {
      v[2] += (double)d0;
      v[3] += 1.0;
    }
  }
  for (int j = tid; j < m; j += 256)
    if (gt1[(size_t)b * a.cap1 + j] == -1) {
      v[4] += (double)a.dust1[(size_t)b * a.cap1 + j];
      v[5] += 1.0;
    }
#pragma unroll
  for (int k = 0; k < 7; ++k) red[k * 256 + tid] = v[k];
  __syncthreads();
  if (tid < 64) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      double s = 0.0;
      for (int i = tid; i < 256; i += 64) s += red[k * 256 + i];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
      if (tid == 0) o[k] = s;
    }
    if (tid == 0) o[7] = (double)n;
  }
}

}  // namespace

EINX_EXPORT size_t einx_lg_assign_nll_ws_bytes(int B, int cap0, int cap1, int d) {
  if (B <= 0 || cap0 <= 0 || cap1 <= 0 || d <= 0 || d % 4 != 0) return 0;
  NllWs w;
  MnnArgs a;
  WsCarver c{nullptr};
  carve_nll(c, w, a, B, cap0, cap1, d);
  return c.bytes;
}

EINX_EXPORT int einx_lg_assign_nll(const float* proj_w, const float* proj_b, const float* match_w, const float* match_b, int d, const float* x0,
                                   const int32_t* n, int cap0, const float* x1, const int32_t* m, int cap1, int B, const int64_t* gt_matches0,
                                   const int64_t* gt_matches1, const int32_t* pos0, const unsigned char* assignment, int64_t as_b, int64_t as_i,
                                   int64_t as_j, void* ws, double* out, void* stream) {
  EINX_CHECK_ARG(proj_w && proj_b && match_w && match_b && x0 && n && x1 && m && gt_matches0 && gt_matches1 && ws && out, "null pointer");
  EINX_CHECK_ARG((pos0 != nullptr) != (assignment != nullptr), "give the positives as pos0 or as a dense assignment, not both");
  EINX_CHECK_ARG(B > 0 && cap0 > 0 && cap1 > 0 && d > 0 && d % 4 == 0, "bad shape (d must be a multiple of 4)");
  hipStream_t st = (hipStream_t)stream;
  const char* const entry = __func__;
  NllWs w{};
  MnnArgs a{};
  WsCarver c{(char*)ws};
  carve_nll(c, w, a, B, cap0, cap1, d);
  w.s0.cnt = n;
  w.s0.cap = cap0;
  w.s1.cnt = m;
  w.s1.cap = cap1;
  const float* x[2] = {x0, x1};
  const Side* sides[2] = {&w.s0, &w.s1};
  LG_CHECK(entry, 0);
  for (int sd = 0; sd < 2; ++sd) {  // MatchAssignment (lightglue.py:365-377): final_proj / d^(1/4) and the matchability terms
    const Side& s = *sides[sd];
    GemmCall proj = gemm_call(EPI_DIV, s, B, x[sd], d, proj_w, proj_b, d, s.q);
    proj.div = sqrtf(sqrtf((float)d));
    LG_CHECK(entry, launch_gemm(st, proj));
    launch_matchability(st, s, x[sd], B, d, match_w, match_b);
    LG_CHECK(entry, 0);
  }
  a.pos0 = pos0;
  a.assign = assignment;
  a.as_b = as_b;
  a.as_i = as_i;
  a.as_j = as_j;
  EINX_PROF("lg_assign_nll (2 tile passes + lse + finish)", st);
  if (const int rc = assign_prologue(entry, st, a, w.s0, w.s1, n, m, B, d, nullptr)) return rc;
  hipLaunchKernelGGL((mnn_tile_kernel<7, true>), assign_grid(a, B), dim3(THREADS), 0, st, a);
  LG_CHECK(entry, 0);
  hipLaunchKernelGGL(lg_nll_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, a, gt_matches0, gt_matches1, out);
  LG_CHECK(entry, 0);
  return EINX_OK;
}
