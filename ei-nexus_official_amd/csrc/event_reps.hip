// event_reps.hip -- the three other event representations of the reference's `representation_type` switch
// (datasets/MVSEC.py:706-718, datasets/EC.py:236-248), on gfx950: raw events (x, y, t, p) -> [B,bins,H,W] fp32.
//
// Replaces (reference file:line): datasets/representations.py:8-22 (time_normalization), :26-63 (events_to_time_surface),
// :178-212 (events_to_event_stack: a Python loop per event), :216-248 (events_to_distance_map: cv2.distanceTransform per bin).
//
// Common contract.  tn = (t - t[first]) / ((t[last] - t[first]) + 1e-8) in float64.  Event k belongs to bin i
// iff tn >= t0 && tn <= t1 with t0 = i * dt, t1 = t0 + dt, dt = 1.0 / nb in float64 (unfused: -ffp-contract=off), BOTH sides
// inclusive: an event on a boundary belongs to two bins.  For non-decreasing t this is the reference's pair of searchsorted calls
// (side "left" / "right"); for unsorted t the reference's slice is whatever its binary search lands on, here the per-event
// predicate holds.  xi = (int)x, yi = (int)y; an event outside 0 <= xi < W, 0 <= yi < H is dropped (where numpy would wrap a
// negative index or raise IndexError: the one deviation).  A sample without events gives zeros (distance map: 8192.0).
//
// Everything is integer work or one correctly rounded float64 division and cast: integer atomics (max / add / or) are exact
// and order-free, so two runs give the same bits.  No float atomic, no scratch, no LDS, no host synchronisation; the host offsets
// travel as kernel arguments (64 samples per launch), so a captured call replays without any library-owned staging.
//
// EventStack accumulates in int32 and converts once.  That equals the reference's sequential float32 `+=` whenever every partial
// sum of a cell stays within +-2^24 (float32 then represents each of them exactly).
#include "einx_common.h"

namespace {

constexpr int REP_CHUNK = 64;  // samples per launch: their offsets are kernel arguments
struct RepOffs {
  int64_t o[REP_CHUNK + 1];
};

enum { REP_TIME_SURFACE = 0, REP_EVENT_STACK = 1, REP_DISTANCE_MAP = 2 };

// the sample's time normalisation: time_normalization, representations.py:19-20
struct RepTime {
  double t0, den;
  __device__ __forceinline__ double norm(double t) const { return (t - t0) / den; }
};
__device__ __forceinline__ RepTime rep_time(const double* t, long long n) {
  const double t0 = t[0];
  return RepTime{t0, (t[n - 1] - t0) + 1e-8};
}

// One pass over the events; grid (ceil(max n / 256), samples of the chunk).
//   time surface: cell[c] = max(cell[c], k + 1) -- the highest-indexed event wins, numpy's rule for repeated indices
//   event stack:  cell[i] += 2 (int)p - 1
//   distance map: bit xi of row yi of slice i
template <int MODE>
__global__ __launch_bounds__(256) void rep_events_kernel(const float* x, const float* y, const double* t, const float* p, const RepOffs offs,
                                                         int b0, int bins, int H, int W, uint32_t* ws) {
  const long long o0 = offs.o[blockIdx.y], n = offs.o[blockIdx.y + 1] - o0;
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int xi = (int)x[o0 + k], yi = (int)y[o0 + k];
  if (xi < 0 || xi >= W || yi < 0 || yi >= H) return;
  const int nb = MODE == REP_TIME_SURFACE ? bins / 2 : bins;
  const double tn = rep_time(t + o0, n).norm(t[o0 + k]);
  const double dt = 1.0 / (double)nb;
  // an event lies in at most two bins, both among floor(tn * nb) - 1 .. + 1; membership is the exact predicate, never the floor
  const double f = fmin(fmax(tn * (double)nb, -1.0), (double)nb);  // (NaN -> -1: every predicate below is false for it anyway)
  const int i0 = (int)floor(f);
  const int pi = (int)p[o0 + k];
  const int b = b0 + blockIdx.y;
  for (int i = max(i0 - 1, 0); i <= min(i0 + 1, nb - 1); ++i) {
    const double t0 = (double)i * dt, t1 = t0 + dt;
    if (!(tn >= t0 && tn <= t1)) continue;
    if (MODE == REP_TIME_SURFACE) {
      int c = 2 * i + pi;
      if (c < 0 && c >= -bins) c += bins;  // numpy wraps a negative channel once (p = -1)
      if (c < 0 || c >= bins) continue;
      atomicMax(ws + (((size_t)b * bins + c) * H + yi) * W + xi, (uint32_t)k + 1u);
    } else if (MODE == REP_EVENT_STACK) {
      atomicAdd((int*)ws + (((size_t)b * bins + i) * H + yi) * W + xi, 2 * pi - 1);
    } else {
      const int ww = einx_cdiv(W, 32);
      atomicOr(ws + (((size_t)b * bins + i) * H + yi) * ww + (xi >> 5), 1u << (xi & 31));
    }
  }
}

// time surface: winner index -> (float)tn of that event, 0 where no event hit; grid (ceil(bins H W / 256), samples of the chunk)
__global__ __launch_bounds__(256) void time_surface_gather_kernel(const double* t, const RepOffs offs, int b0, int per, const uint32_t* win,
                                                                  float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  const long long o0 = offs.o[blockIdx.y], n = offs.o[blockIdx.y + 1] - o0;
  const size_t cell = (size_t)(b0 + blockIdx.y) * per + i;
  const uint32_t k1 = win[cell];
  out[cell] = k1 ? (float)rep_time(t + o0, n).norm(t[o0 + k1 - 1]) : 0.0f;
}

__global__ __launch_bounds__(256) void event_stack_convert_kernel(const int32_t* sum, size_t n, float* out) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (float)sum[i];
}

// ---- distance map: 3x3 chamfer distance in 16.16 fixed point --------------------------------------------------------------
constexpr int DM_HV = 62587;             // 0.955
constexpr int DM_DIAG = 89738;           // 1.3693
constexpr int DM_INF = 0x7fffffff >> 2;  // "no set pixel": (float)DM_INF / 65536 = 8192.0f
constexpr int DM_MAX_W = 1024, DM_MAX_H = 4096;  // DIAG * max(H, W) stays below DM_INF: no real distance saturates

// inclusive prefix minimum over the 64 lanes: four row_shr steps inside the rows of 16 lanes, then row_bcast:15 / :31
__device__ __forceinline__ int wave_prefix_min(int v) {
  constexpr int id = 0x7fffffff;  // what a lane without a source keeps: the identity of min
  v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x111, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x112, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x114, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x118, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x142, 0xa, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x143, 0xc, 0xf, false));
  return v;
}

// One raster sweep of the two-pass chamfer transform over one [H,W] slice, by ONE wave with the row in registers: lane l holds
// the PPL neighbouring pixels at positions l * PPL .. + PPL - 1 of the sweep's own left-to-right order.  The forward sweep
// (BACK = false) walks rows top-down and pixels left to right; the backward sweep is its mirror image, so it runs the SAME code
// on the slice turned by 180 degrees (position q is pixel 64 PPL - 1 - q, rows bottom-up).
//   c[q] = min(own[q], prev[q-1] + DIAG, prev[q] + HV, prev[q+1] + DIAG)      the three neighbours of the previous row
//   d[q] = min(c[q], d[q-1] + HV)                                              the neighbour to the left: a min-plus scan,
//          = HV q + prefix-min(c[q] - HV q): sequential inside a lane, one wave scan of the lanes' last values across them.
// own: forward 0 on a set pixel, DM_INF elsewhere; backward the forward sweep's value.  No value exceeds DM_INF + DIAG: int32.
template <int PPL, bool BACK>
__device__ __forceinline__ void dm_sweep(const uint32_t* bits, int ww, int* fwd, float* out, int H, int W) {
  const int lane = threadIdx.x & 63;
  const int q0 = lane * PPL;
  int pr[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) pr[k] = DM_INF;
  // what the next row brings, loaded one row ahead of the dependent chain
  int own[PPL];
  auto load_own = [&](int r) {
    const int yy = BACK ? H - 1 - r : r;
    if (BACK) {
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const int xx = 64 * PPL - 1 - (q0 + k);
        own[k] = xx < W ? fwd[(size_t)yy * W + xx] : DM_INF;
      }
    } else {
      const int w0 = min(q0 >> 5, ww - 1), w1 = min(w0 + 1, ww - 1);  // a lane's pixels span at most two words
      const unsigned long long m = (((unsigned long long)bits[(size_t)yy * ww + w1] << 32) | bits[(size_t)yy * ww + w0]) >> (q0 & 31);
#pragma unroll
      for (int k = 0; k < PPL; ++k) own[k] = (q0 + k < W && ((m >> k) & 1)) ? 0 : DM_INF;
    }
  };
  load_own(0);
  for (int r = 0; r < H; ++r) {
    int c[PPL];
    {
      int left = __shfl_up(pr[PPL - 1], 1, 64), right = __shfl_down(pr[0], 1, 64);
      if (lane == 0) left = DM_INF;
      if (lane == 63) right = DM_INF;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const int l = k > 0 ? pr[k - 1] : left, rr = k < PPL - 1 ? pr[k + 1] : right;
        const int xx = BACK ? 64 * PPL - 1 - (q0 + k) : q0 + k;
        c[k] = xx < W ? min(own[k], min(min(l, rr) + DM_DIAG, pr[k] + DM_HV)) : DM_INF;  // the padding beyond W carries no distance
      }
    }
    if (r + 1 < H) load_own(r + 1);
    // inside the lane, as if nothing came in from the left
#pragma unroll
    for (int k = 1; k < PPL; ++k) c[k] = min(c[k], c[k - 1] + DM_HV);
    // across the lanes: in[l] = min over j < l of (last[j] + (l - 1 - j) S), S = PPL HV
    constexpr int S = PPL * DM_HV;
    int u = __shfl_up(c[PPL - 1] - lane * S, 1, 64);
    if (lane == 0) u = 0x7fffffff;
    int in = wave_prefix_min(u) + (lane - 1) * S;
    if (lane == 0) in = DM_INF;
    const int yy = BACK ? H - 1 - r : r;
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      const int xx = BACK ? 64 * PPL - 1 - (q0 + k) : q0 + k;
      const int d = xx < W ? min(c[k], in + (k + 1) * DM_HV) : DM_INF;
      pr[k] = d;
      if (xx < W) {
        if (BACK) out[(size_t)yy * W + xx] = (float)d * (1.0f / 65536.0f);
        else fwd[(size_t)yy * W + xx] = d;
      }
    }
  }
}

// one wave per (sample, bin) slice; the forward sweep's int32 values wait in the output buffer for the backward sweep
template <int PPL>
__global__ __launch_bounds__(64) void distance_map_kernel(const uint32_t* bits_all, int H, int W, float* out_all) {
  const int ww = einx_cdiv(W, 32);
  const uint32_t* bits = bits_all + (size_t)blockIdx.x * H * ww;
  float* out = out_all + (size_t)blockIdx.x * H * W;
  dm_sweep<PPL, false>(bits, ww, (int*)out, out, H, W);
  // the backward sweep reads, on other lanes of this wave, what the forward sweep stored: same CU, same L1
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  dm_sweep<PPL, true>(bits, ww, (int*)out, out, H, W);
}

template <int PPL>
void launch_distance_map(const uint32_t* bits, int slices, int H, int W, float* out, hipStream_t s) {
  hipLaunchKernelGGL(distance_map_kernel<PPL>, dim3((unsigned)slices), dim3(64), 0, s, bits, H, W, out);
}

// The instantiations, narrowest first: pixels per lane, the name einx_distance_map_plan reports, the launch.  A new arm is a line
// here (and its widths in tests/event_reps_cases.py).
struct DmArm {
  int ppl;
  const char* name;
  void (*launch)(const uint32_t*, int, int, int, float*, hipStream_t);
};
#define DM_ARM(P) {P, "distance_map_kernel<" #P ">", launch_distance_map<P>}
constexpr DmArm DM_ARMS[] = {DM_ARM(2), DM_ARM(4), DM_ARM(6), DM_ARM(8), DM_ARM(12), DM_ARM(16)};
#undef DM_ARM
static_assert(DM_ARMS[sizeof(DM_ARMS) / sizeof(DM_ARMS[0]) - 1].ppl * 64 == DM_MAX_W, "the widest arm sets the documented limit");

// the one selection, used by the launch and by einx_distance_map_plan: the first arm whose 64 lanes hold a row of W pixels;
// nullptr for a shape the op refuses
const DmArm* dm_select(int H, int W) {
  if (H <= 0 || W <= 0 || W > DM_MAX_W || H > DM_MAX_H) return nullptr;
  for (const DmArm& a : DM_ARMS)
    if (einx_cdiv(W, 64) <= a.ppl) return &a;
  return nullptr;
}

// workspace of all three ops: ONE region of 32-bit words the event pass fills (time surface: winner index + 1 per cell, event
// stack: int32 sum per cell, distance map: one bit per pixel in rows of ceil(W / 32) words), and 256 bytes of slack that pay
// for rounding the caller's base up
uint32_t* carve(WsCarver& c, int mode, int B, int bins, int H, int W) {
  const size_t row = mode == REP_DISTANCE_MAP ? (size_t)einx_cdiv(W, 32) : (size_t)W;
  uint32_t* words = c.take<uint32_t>((size_t)B * bins * H * row);
  c.slack(256);
  return words;
}

bool rep_shape_ok(int mode, int B, int bins, int H, int W) {
  if (B <= 0 || bins <= 0 || H <= 0 || W <= 0 || H >= 60000 || W >= 60000) return false;
  if (mode == REP_TIME_SURFACE && bins < 2) return false;  // bins // 2 == 0 bins: the reference divides by zero
  if (mode == REP_DISTANCE_MAP && !dm_select(H, W)) return false;
  return true;
}

size_t rep_ws_bytes(int mode, int B, int bins, int H, int W, int64_t total_events) {
  if (!rep_shape_ok(mode, B, bins, H, W) || total_events < 0) return 0;
  WsCarver c{nullptr};
  carve(c, mode, B, bins, H, W);
  return c.bytes;
}

template <int MODE>
int rep_run(const char* name, const float* x, const float* y, const double* t, const float* p, const int64_t* offsets_host, int B, int bins,
            int H, int W, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!(offsets_host && out && ws)) {
    einx_set_error("%s: null pointer", name);
    return EINX_ERR_ARG;
  }
  if (!rep_shape_ok(MODE, B, bins, H, W) || (size_t)bins * H * W >= ((size_t)1 << 31)) {
    einx_set_error("%s: bad shape", name);
    return EINX_ERR_ARG;
  }
  const int64_t N = offsets_host[B];
  long long mx = 0;
  bool sorted = offsets_host[0] == 0;
  for (int b = 0; b < B && sorted; ++b) {
    const long long n = offsets_host[b + 1] - offsets_host[b];
    sorted = n >= 0;
    mx = n > mx ? n : mx;
  }
  if (!sorted || N >= ((int64_t)1 << 31) || (N > 0 && !(x && y && t && p))) {
    einx_set_error("%s: offsets_host must start at 0 and not decrease; event arrays must not be null", name);
    return EINX_ERR_ARG;
  }
  if (ws_bytes < rep_ws_bytes(MODE, B, bins, H, W, N)) {
    einx_set_error("%s: workspace smaller than its *_ws_bytes", name);
    return EINX_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  WsCarver c = WsCarver::aligned_up(ws);
  uint32_t* words = carve(c, MODE, B, bins, H, W);
  if (hipMemsetAsync(words, 0, c.bytes - 256 /* the region without the slack */, s) != hipSuccess) {
    einx_set_error("%s: memset failed", name);
    return EINX_ERR_LAUNCH;
  }
  const int per = bins * H * W;
  for (int b0 = 0; b0 < B; b0 += REP_CHUNK) {
    const int nb = B - b0 < REP_CHUNK ? B - b0 : REP_CHUNK;
    RepOffs offs;
    long long cmx = 0;
    for (int j = 0; j <= REP_CHUNK; ++j) offs.o[j] = offsets_host[b0 + (j < nb ? j : nb)];
    for (int j = 0; j < nb; ++j) cmx = offs.o[j + 1] - offs.o[j] > cmx ? offs.o[j + 1] - offs.o[j] : cmx;
    if (cmx > 0) {
      hipLaunchKernelGGL(rep_events_kernel<MODE>, dim3((unsigned)((cmx + 255) / 256), (unsigned)nb), dim3(256), 0, s, x, y, t, p, offs, b0, bins, H,
                         W, words);
      EINX_CHECK_LAUNCH();
    }
    if (MODE == REP_TIME_SURFACE) {
      hipLaunchKernelGGL(time_surface_gather_kernel, dim3((unsigned)einx_cdiv(per, 256), (unsigned)nb), dim3(256), 0, s, t, offs, b0, per, words, out);
      EINX_CHECK_LAUNCH();
    }
  }
  if (MODE == REP_EVENT_STACK) {
    const size_t n = (size_t)B * per;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(event_stack_convert_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, (const int32_t*)words, n, out);
    EINX_CHECK_LAUNCH();
  }
  if (MODE == REP_DISTANCE_MAP) {
    dm_select(H, W)->launch(words, B * bins, H, W, out, s);  // never null here: rep_shape_ok asked dm_select too
    EINX_CHECK_LAUNCH();
  }
  return EINX_OK;
}

}  // namespace

EINX_EXPORT size_t einx_time_surface_ws_bytes(int B, int bins, int H, int W, int64_t total_events) {
  return rep_ws_bytes(REP_TIME_SURFACE, B, bins, H, W, total_events);
}
EINX_EXPORT size_t einx_event_stack_ws_bytes(int B, int bins, int H, int W, int64_t total_events) {
  return rep_ws_bytes(REP_EVENT_STACK, B, bins, H, W, total_events);
}
EINX_EXPORT size_t einx_distance_map_ws_bytes(int B, int bins, int H, int W, int64_t total_events) {
  return rep_ws_bytes(REP_DISTANCE_MAP, B, bins, H, W, total_events);
}

EINX_EXPORT const char* einx_distance_map_plan(int H, int W) {
  const DmArm* a = dm_select(H, W);
  return a ? a->name : nullptr;
}

EINX_EXPORT int einx_time_surface(const float* x, const float* y, const double* t, const float* p, const int64_t* offsets_host, int B,
                                  int bins, int H, int W, float* out, void* ws, size_t ws_bytes, void* stream) {
  return rep_run<REP_TIME_SURFACE>(__func__, x, y, t, p, offsets_host, B, bins, H, W, out, ws, ws_bytes, stream);
}
EINX_EXPORT int einx_event_stack(const float* x, const float* y, const double* t, const float* p, const int64_t* offsets_host, int B,
                                 int bins, int H, int W, float* out, void* ws, size_t ws_bytes, void* stream) {
  return rep_run<REP_EVENT_STACK>(__func__, x, y, t, p, offsets_host, B, bins, H, W, out, ws, ws_bytes, stream);
}
EINX_EXPORT int einx_distance_map(const float* x, const float* y, const double* t, const float* p, const int64_t* offsets_host, int B,
                                  int bins, int H, int W, float* out, void* ws, size_t ws_bytes, void* stream) {
  return rep_run<REP_DISTANCE_MAP>(__func__, x, y, t, p, offsets_host, B, bins, H, W, out, ws, ws_bytes, stream);
}
