// rectify.hip -- rectification of raw recordings on gfx950: the step the reference runs once per dataset on the
// host before any of its dataset classes can read `events_rect` / `image_rect` (datasets/MVSEC.py:224-260) or
// `events_corrected` / `images_corrected` (datasets/EC.py:56-72).
//
// Replaces (reference file:line): datasets/MVSEC_rectify.py:16-21 (cv.remap per frame), :23-45 (map lookup per event and the
// bounds filter), :91-106 (cv.fisheye.initUndistortRectifyMap); datasets/rectify_ec.py:48-50 (cv.undistort per frame), :70-78
// (cv.undistortPoints + rint per event), :80-83 (the bounds filter).
//
// The maps are H x W: one thread per pixel in float64, stored as float32 (-ffp-contract=off: every operation is rounded as it
// is written, so a float64 host restatement of the same expressions differs by a double rounding at most).  The event pass
// is a gather, a predicate and a STABLE stream compaction over int64 lengths, in three steps without a spin or an ordered
// atomic: (1) every workgroup counts the kept events of its chunk of EV_CHUNK events, (2) the counts are scanned (tiles of
// SCAN_TILE counts, then the tiles' sums by one workgroup), (3) every workgroup classifies its chunk again, ranks the kept
// events with wave ballots, packs them in LDS and writes them out as one dense run at its scanned offset.  A workgroup's
// offset is a sum of integers and so a pure function of its position: two calls give the same bits.  The one atomic is an
// integer add of the out-of-map count, which is order-free.
#include "einx_common.h"

#include <math.h>

namespace {

// ---- maps ------------------------------------------------------------------------------------------------------------------
struct MapParams {
  double fx, fy, cx, cy;  // K
  double d[5];            // fisheye: k1..k4; radtan: k1, k2, p1, p2, k3
  double m[9];            // rectify maps: iR = (P R)^-1; undistort-points map: P
  int H, W, iters, round_out;
};

// radial factor and tangential shift of the radtan model at the normalised point (x, y)
struct RadTan {
  double kr, dx, dy;
};
__device__ __forceinline__ RadTan radtan(const MapParams& q, double x, double y) {
  const double k1 = q.d[0], k2 = q.d[1], p1 = q.d[2], p2 = q.d[3], k3 = q.d[4];
  const double r2 = x * x + y * y;
  RadTan o;
  o.kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  o.dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * (x * x));
  o.dy = p1 * (r2 + 2.0 * (y * y)) + 2.0 * p2 * x * y;
  return o;
}

enum { MAP_FISHEYE = 0, MAP_RADTAN = 1, MAP_POINTS = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void rectify_map_kernel(const MapParams q, float* map_x, float* map_y) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // H * W may come within 255 of 2^31
  if (i >= (long long)q.H * q.W) return;
  const double u = (double)(i % q.W), v = (double)(i / q.W);
  double ox, oy;
  if (MODE == MAP_POINTS) {
    // cv.undistortPoints: invert the distortion by fixed-point iteration from the distorted point, then project with P
    const double x0 = (u - q.cx) / q.fx, y0 = (v - q.cy) / q.fy;
    double x = x0, y = y0;
    for (int it = 0; it < q.iters; ++it) {
      const RadTan t = radtan(q, x, y);
      x = (x0 - t.dx) / t.kr;
      y = (y0 - t.dy) / t.kr;
    }
    const double X = q.m[0] * x + q.m[1] * y + q.m[2];
    const double Y = q.m[3] * x + q.m[4] * y + q.m[5];
    const double Wp = q.m[6] * x + q.m[7] * y + q.m[8];
    ox = X / Wp;
    oy = Y / Wp;
    if (q.round_out) {
      ox = rint(ox);
      oy = rint(oy);
    }
  } else {
    const double X = q.m[0] * u + q.m[1] * v + q.m[2];
    const double Y = q.m[3] * u + q.m[4] * v + q.m[5];
    const double Wd = q.m[6] * u + q.m[7] * v + q.m[8];
    const double x = X / Wd, y = Y / Wd;
    if (MODE == MAP_FISHEYE) {
      if (Wd <= 0.0) {
        ox = -1.0;
        oy = -1.0;
      } else {
        const double r = sqrt(x * x + y * y);
        const double th = atan(r);
        const double th2 = th * th, th4 = th2 * th2, th6 = th4 * th2, th8 = th4 * th4;
        const double thd = th * (1.0 + q.d[0] * th2 + q.d[1] * th4 + q.d[2] * th6 + q.d[3] * th8);
        const double s = r == 0.0 ? 1.0 : thd / r;
        ox = q.fx * x * s + q.cx;
        oy = q.fy * y * s + q.cy;
      }
    } else {
      const RadTan t = radtan(q, x, y);
      ox = q.fx * (x * t.kr + t.dx) + q.cx;
      oy = q.fy * (y * t.kr + t.dy) + q.cy;
    }
  }
  map_x[i] = (float)ox;
  map_y[i] = (float)oy;
}

bool invert3(const double* a, double* o) {
  const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c0 + a[1] * c1 + a[2] * c2;
  if (!(det != 0.0) || !isfinite(det)) return false;
  o[0] = c0 / det;
  o[1] = (a[2] * a[7] - a[1] * a[8]) / det;
  o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
  o[3] = c1 / det;
  o[4] = (a[0] * a[8] - a[2] * a[6]) / det;
  o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
  o[6] = c2 / det;
  o[7] = (a[1] * a[6] - a[0] * a[7]) / det;
  o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
  return true;
}

template <int MODE>
int map_run(const char* name, const double* K, const double* D, int nd, const double* R, const double* P, int H, int W, int iters,
            int round_out, float* map_x, float* map_y, void* stream) {
  if (!(K && D && P && map_x && map_y) || (MODE != MAP_POINTS && !R)) {
    einx_set_error("%s: null pointer", name);
    return EINX_ERR_ARG;
  }
  if (H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31) || iters < 0) {
    einx_set_error("%s: H and W must be positive with H * W < 2^31, iters >= 0", name);
    return EINX_ERR_ARG;
  }
  MapParams q{};
  q.fx = K[0], q.fy = K[1], q.cx = K[2], q.cy = K[3];
  for (int i = 0; i < nd; ++i) q.d[i] = D[i];
  if (MODE == MAP_POINTS) {
    for (int i = 0; i < 9; ++i) q.m[i] = P[i];
  } else {
    double pr[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) pr[3 * i + j] = P[3 * i] * R[j] + P[3 * i + 1] * R[3 + j] + P[3 * i + 2] * R[6 + j];
    if (!invert3(pr, q.m)) {
      einx_set_error("%s: P R is singular", name);
      return EINX_ERR_ARG;
    }
  }
  q.H = H, q.W = W, q.iters = iters, q.round_out = round_out;
  hipLaunchKernelGGL(rectify_map_kernel<MODE>, dim3((unsigned)(((long long)H * W + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, map_x, map_y);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

// ---- frames ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float remap_load(const uint8_t* p) { return (float)*p; }
__device__ __forceinline__ float remap_load(const float* p) { return *p; }
__device__ __forceinline__ void remap_store(uint8_t* p, float v) { *p = (uint8_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }
__device__ __forceinline__ void remap_store(float* p, float v) { *p = v; }

// one thread per destination pixel and per gridDim.y-th frame: the launch gives a stack just enough frame slices to fill the
// chip (REMAP_BLOCKS workgroups), and a thread walks the frames of its slice with the map entry and the four tap offsets computed
// once
constexpr long long REMAP_BLOCKS = 4096;  // workgroups that fill the chip (16 per CU); frames beyond them are walked
template <typename T>
__global__ __launch_bounds__(256) void remap_bilinear_kernel(const T* src, int F, int Hs, int Ws, const float* map_x, const float* map_y, int HW,
                                                             T* dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const float mx = map_x[i], my = map_y[i];
  // a position whose four taps all lie outside the source (or that is not a number) gives the border value
  const bool in = mx > -1.0f && mx < (float)Ws && my > -1.0f && my < (float)Hs;
  const float x0f = floorf(mx), y0f = floorf(my);
  const float fx = mx - x0f, fy = my - y0f;
  const int x0 = in ? (int)x0f : 0, y0 = in ? (int)y0f : 0;
  const bool l = x0 >= 0, r = x0 + 1 < Ws, t = y0 >= 0, b = y0 + 1 < Hs;
  const size_t plane = (size_t)Hs * Ws;
  for (int f = blockIdx.y; f < F; f += gridDim.y) {
    float v = 0.0f;
    if (in) {
      const T* s = src + (size_t)f * plane + (ptrdiff_t)y0 * Ws + x0;
      const float i00 = t && l ? remap_load(s) : 0.0f, i01 = t && r ? remap_load(s + 1) : 0.0f;
      const float i10 = b && l ? remap_load(s + Ws) : 0.0f, i11 = b && r ? remap_load(s + Ws + 1) : 0.0f;
      const float top = i00 + fx * (i01 - i00), bot = i10 + fx * (i11 - i10);
      v = top + fy * (bot - top);
    }
    remap_store(dst + (size_t)f * HW + i, v);
  }
}

// ---- events ----------------------------------------------------------------------------------------------------------------
constexpr int EV_THREADS = 256, EV_WAVES = EV_THREADS / 64;
constexpr int EV_VEC = 4;                                  // consecutive events per thread and round: one 16-byte load of x, y and p
constexpr int EV_ROUNDS = 2;                               // rounds per workgroup
constexpr int EV_ROUND = EV_THREADS * EV_VEC;              // events per round
constexpr int EV_CHUNK = EV_ROUND * EV_ROUNDS;             // events per workgroup: 2048
constexpr int SCAN_THREADS = 256, SCAN_VEC = 4, SCAN_TILE = SCAN_THREADS * SCAN_VEC;  // counts per scan workgroup: 1024

struct EvMap {
  const float *map_x, *map_y;
  int H, W;
  float x_hi, y_hi;
};

enum { EV_DROP = 0, EV_KEEP = 1, EV_OUTSIDE = 2 };

// the rule of one event (MVSEC_rectify.py:29-43, rectify_ec.py:80-83): np.round is rint (half to even); a raw coordinate that is
// not a pixel of the map is refused, not wrapped; NaN fails every comparison
__device__ __forceinline__ int ev_classify(const EvMap& m, float x, float y, float* ox, float* oy) {
  const float rx = rintf(x), ry = rintf(y);
  if (!(rx >= 0.0f && rx < (float)m.W && ry >= 0.0f && ry < (float)m.H)) return EV_OUTSIDE;
  const int i = (int)ry * m.W + (int)rx;
  const float a = m.map_x[i], b = m.map_y[i];
  *ox = a;
  *oy = b;
  return (a >= 0.0f && a < m.x_hi && b >= 0.0f && b < m.y_hi) ? EV_KEEP : EV_DROP;
}

// EV_VEC consecutive elements starting at k: one 16-byte load inside a full, aligned chunk; element by element (0 past n) otherwise
template <typename T>
__device__ __forceinline__ void ev_load(const T* p, long long k, long long n, bool wide, T (&v)[EV_VEC]) {
  if (wide) {
    if constexpr (sizeof(T) == 4) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(p + k);
#pragma unroll
      for (int j = 0; j < EV_VEC; ++j) v[j] = q[j];
    } else {
      typedef double f64x2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int j = 0; j < EV_VEC; j += 2) {
        const f64x2 q = *reinterpret_cast<const f64x2*>(p + k + j);
        v[j] = q[0];
        v[j + 1] = q[1];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < EV_VEC; ++j) v[j] = k + j < n ? p[k + j] : (T)0;
  }
}

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// step 1: kept events per chunk; the chunk's out-of-map events are added to *outside (an integer sum: order-free)
__global__ __launch_bounds__(EV_THREADS) void ev_count_kernel(const float* x, const float* y, long long n, int aligned, const EvMap m,
                                                              long long* counts, unsigned long long* outside) {
  __shared__ int s_keep[EV_WAVES], s_out[EV_WAVES];
  const long long c0 = (long long)blockIdx.x * EV_CHUNK;
  const bool wide = aligned && c0 + EV_CHUNK <= n;
  int keep = 0, out = 0;
#pragma unroll
  for (int r = 0; r < EV_ROUNDS; ++r) {
    const long long k = c0 + r * EV_ROUND + threadIdx.x * EV_VEC;
    float xv[EV_VEC], yv[EV_VEC];
    ev_load(x, k, n, wide, xv);
    ev_load(y, k, n, wide, yv);
#pragma unroll
    for (int j = 0; j < EV_VEC; ++j) {
      float a, b;
      const int c = k + j < n ? ev_classify(m, xv[j], yv[j], &a, &b) : EV_DROP;
      keep += c == EV_KEEP;
      out += c == EV_OUTSIDE;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    keep += __shfl_xor(keep, off, 64);
    out += __shfl_xor(out, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_keep[threadIdx.x >> 6] = keep;
    s_out[threadIdx.x >> 6] = out;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int ks = 0, os = 0;
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) {
      ks += s_keep[w];
      os += s_out[w];
    }
    counts[blockIdx.x] = ks;
    if (os) atomicAdd(outside, (unsigned long long)os);
  }
}

// exclusive scan of the workgroup's SCAN_TILE values (SCAN_VEC consecutive ones per thread); returns the tile's sum to every thread
__device__ __forceinline__ long long scan_tile(long long (&v)[SCAN_VEC], long long* s_wave) {
  long long own = 0;
#pragma unroll
  for (int j = 0; j < SCAN_VEC; ++j) own += v[j];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long inc = own;  // inclusive scan over the wave's lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long up = __shfl_up(inc, off, 64);
    if (lane >= off) inc += up;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  long long base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < SCAN_THREADS / 64; ++w) {
    const long long s = s_wave[w];
    if (w < wave) base += s;
    total += s;
  }
  __syncthreads();  // s_wave may be written again by the caller's next tile
  long long run = base + inc - own;
#pragma unroll
  for (int j = 0; j < SCAN_VEC; ++j) {
    const long long c = v[j];
    v[j] = run;
    run += c;
  }
  return total;
}

// step 2a: counts[] -> exclusive prefix inside each tile of SCAN_TILE chunks, in place; tile_sums[tile] = the tile's sum
__global__ __launch_bounds__(SCAN_THREADS) void ev_scan_tiles_kernel(long long* counts, long long nchunks, long long* tile_sums) {
  __shared__ long long s_wave[SCAN_THREADS / 64];
  const long long i0 = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_VEC;
  long long v[SCAN_VEC];
#pragma unroll
  for (int j = 0; j < SCAN_VEC; ++j) v[j] = i0 + j < nchunks ? counts[i0 + j] : 0;
  const long long total = scan_tile(v, s_wave);
#pragma unroll
  for (int j = 0; j < SCAN_VEC; ++j)
    if (i0 + j < nchunks) counts[i0 + j] = v[j];
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// step 2b: one workgroup turns tile_sums[] into its exclusive prefix, SCAN_TILE of them at a time with a running carry, and
// writes the number kept
__global__ __launch_bounds__(SCAN_THREADS) void ev_scan_top_kernel(long long* tile_sums, long long ntiles, long long* out_counts) {
  __shared__ long long s_wave[SCAN_THREADS / 64];
  long long carry = 0;
  for (long long t0 = 0; t0 < ntiles; t0 += SCAN_TILE) {
    const long long i0 = t0 + threadIdx.x * SCAN_VEC;
    long long v[SCAN_VEC];
#pragma unroll
    for (int j = 0; j < SCAN_VEC; ++j) v[j] = i0 + j < ntiles ? tile_sums[i0 + j] : 0;
    const long long total = scan_tile(v, s_wave);
#pragma unroll
    for (int j = 0; j < SCAN_VEC; ++j)
      if (i0 + j < ntiles) tile_sums[i0 + j] = carry + v[j];
    carry += total;
  }
  if (threadIdx.x == 0) out_counts[0] = carry;
}

// step 3: the chunk's kept events, in input order, as one dense run at the chunk's scanned offset
__global__ __launch_bounds__(EV_THREADS) void ev_scatter_kernel(const float* x, const float* y, const double* t, const float* p, long long n,
                                                                int aligned, const EvMap m, const long long* chunk_prefix,
                                                                const long long* tile_prefix, float* out_x, float* out_y, double* out_t,
                                                                float* out_p) {
  __shared__ float s_x[EV_CHUNK], s_y[EV_CHUNK], s_p[EV_CHUNK];
  __shared__ double s_t[EV_CHUNK];
  __shared__ int s_cnt[EV_ROUNDS][EV_WAVES];
  const long long c0 = (long long)blockIdx.x * EV_CHUNK;
  const bool wide = aligned && c0 + EV_CHUNK <= n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float ox[EV_ROUNDS][EV_VEC], oy[EV_ROUNDS][EV_VEC], pv[EV_ROUNDS][EV_VEC];
  double tv[EV_ROUNDS][EV_VEC];
  int rank[EV_ROUNDS];         // kept events of this (round, wave) before this lane's first one
  unsigned kept[EV_ROUNDS];    // bit j: the lane's event j of the round is kept
#pragma unroll
  for (int r = 0; r < EV_ROUNDS; ++r) {
    const long long k = c0 + r * EV_ROUND + threadIdx.x * EV_VEC;
    float xv[EV_VEC], yv[EV_VEC];
    ev_load(x, k, n, wide, xv);
    ev_load(y, k, n, wide, yv);
    ev_load(p, k, n, wide, pv[r]);
    ev_load(t, k, n, wide, tv[r]);
    kept[r] = 0;
    int before = 0, wave_total = 0;
#pragma unroll
    for (int j = 0; j < EV_VEC; ++j) {
      const bool kp = k + j < n && ev_classify(m, xv[j], yv[j], &ox[r][j], &oy[r][j]) == EV_KEEP;
      const unsigned long long ball = __ballot(kp);
      before += lanes_below(ball);
      wave_total += __popcll(ball);
      kept[r] |= (unsigned)kp << j;
    }
    rank[r] = before;
    if (lane == 0) s_cnt[r][wave] = wave_total;
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int r = 0; r < EV_ROUNDS; ++r) {
    int base = 0;
#pragma unroll
    for (int rr = 0; rr < EV_ROUNDS; ++rr)
#pragma unroll
      for (int w = 0; w < EV_WAVES; ++w) {
        const int c = s_cnt[rr][w];
        if (rr < r || (rr == r && w < wave)) base += c;
        if (r == 0) total += c;
      }
    // inside the (round, wave): lanes in order, each lane's events in order
    int at = base + rank[r];
#pragma unroll
    for (int j = 0; j < EV_VEC; ++j) {
      if (kept[r] >> j & 1u) {
        s_x[at] = ox[r][j];
        s_y[at] = oy[r][j];
        s_p[at] = pv[r][j];
        s_t[at] = tv[r][j];
        ++at;
      }
    }
  }
  __syncthreads();
  const long long dst = chunk_prefix[blockIdx.x] + tile_prefix[blockIdx.x / SCAN_TILE];
  for (int i = threadIdx.x; i < total; i += EV_THREADS) {
    out_x[dst + i] = s_x[i];
    out_y[dst + i] = s_y[i];
    out_p[dst + i] = s_p[i];
    out_t[dst + i] = s_t[i];
  }
}

struct EvWs {
  long long* counts;     // [chunks]: kept per chunk, then its exclusive prefix inside the tile
  long long* tile_sums;  // [tiles]: kept per tile, then its exclusive prefix
};
long long ev_chunks(int64_t N) { return (N + EV_CHUNK - 1) / EV_CHUNK; }
long long ev_tiles(int64_t N) { return (ev_chunks(N) + SCAN_TILE - 1) / SCAN_TILE; }
EvWs ev_carve(WsCarver& c, int64_t N) {
  EvWs w;
  w.counts = c.take<long long>((size_t)(ev_chunks(N) > 0 ? ev_chunks(N) : 1));
  w.tile_sums = c.take<long long>((size_t)(ev_tiles(N) > 0 ? ev_tiles(N) : 1));
  c.slack(256);
  return w;
}

}  // namespace

EINX_EXPORT int einx_rectify_map_fisheye(const double* K, const double* D, const double* R, const double* P, int H, int W, float* map_x,
                                         float* map_y, void* stream) {
  return map_run<MAP_FISHEYE>(__func__, K, D, 4, R, P, H, W, 0, 0, map_x, map_y, stream);
}

EINX_EXPORT int einx_rectify_map_radtan(const double* K, const double* D, const double* R, const double* P, int H, int W, float* map_x,
                                        float* map_y, void* stream) {
  return map_run<MAP_RADTAN>(__func__, K, D, 5, R, P, H, W, 0, 0, map_x, map_y, stream);
}

EINX_EXPORT int einx_undistort_points_map_radtan(const double* K, const double* D, const double* P, int H, int W, int iters, int round_out,
                                                 float* map_x, float* map_y, void* stream) {
  return map_run<MAP_POINTS>(__func__, K, D, 5, nullptr, P, H, W, iters, round_out, map_x, map_y, stream);
}

EINX_EXPORT int einx_remap_bilinear(const void* src, int src_type, int F, int Hs, int Ws, const float* map_x, const float* map_y, int H, int W,
                                    void* dst, void* stream) {
  EINX_CHECK_ARG(src && map_x && map_y && dst, "null pointer");
  EINX_CHECK_ARG(src_type == EINX_REMAP_U8 || src_type == EINX_REMAP_F32, "src_type must be EINX_REMAP_U8 or EINX_REMAP_F32");
  EINX_CHECK_ARG(F > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "sizes must be positive");
  EINX_CHECK_ARG((long long)Hs * Ws < (1ll << 31) && (long long)H * W < (1ll << 31), "a frame or a map of 2^31 pixels or more");
  const long long gx = ((long long)H * W + 255) / 256, slices = (REMAP_BLOCKS + gx - 1) / gx;
  const dim3 grid((unsigned)gx, (unsigned)(F < slices ? F : slices));
  if (src_type == EINX_REMAP_U8)
    hipLaunchKernelGGL(remap_bilinear_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, F, Hs, Ws, map_x, map_y, H * W,
                       (uint8_t*)dst);
  else
    hipLaunchKernelGGL(remap_bilinear_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, F, Hs, Ws, map_x, map_y, H * W,
                       (float*)dst);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT size_t einx_events_remap_ws_bytes(int64_t N) {
  if (N < 0) return 0;
  WsCarver c{nullptr};
  ev_carve(c, N);
  return c.bytes;
}

EINX_EXPORT int einx_events_remap(const float* x, const float* y, const double* t, const float* p, int64_t N, const float* map_x,
                                  const float* map_y, int H, int W, float x_hi, float y_hi, float* out_x, float* out_y, double* out_t,
                                  float* out_p, int64_t* out_counts, void* ws, size_t ws_bytes, void* stream) {
  EINX_CHECK_ARG(N >= 0, "N is negative");
  EINX_CHECK_ARG(map_x && map_y && out_counts && ws, "null pointer");
  EINX_CHECK_ARG(N == 0 || (x && y && t && p && out_x && out_y && out_t && out_p), "null event array");
  EINX_CHECK_ARG(H > 0 && W > 0 && (long long)H * W < (1ll << 31), "H and W must be positive with H * W < 2^31");
  EINX_CHECK_ARG(ws_bytes >= einx_events_remap_ws_bytes(N), "workspace smaller than einx_events_remap_ws_bytes");
  const long long chunks = ev_chunks(N), tiles = ev_tiles(N);
  EINX_CHECK_ARG(chunks < (1ll << 31), "N too large for one launch");
  hipStream_t s = (hipStream_t)stream;
  WsCarver c = WsCarver::aligned_up(ws);
  const EvWs w = ev_carve(c, N);
  if (hipMemsetAsync(out_counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
    einx_set_error("%s: memset failed", __func__);
    return EINX_ERR_LAUNCH;
  }
  if (N == 0) return EINX_OK;
  const EvMap m{map_x, map_y, H, W, x_hi, y_hi};
  // 16-byte loads want every array on a 16-byte boundary; chunk starts are multiples of EV_CHUNK elements
  const int aligned = ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)t | (uintptr_t)p) & 15) == 0);
  hipLaunchKernelGGL(ev_count_kernel, dim3((unsigned)chunks), dim3(EV_THREADS), 0, s, x, y, (long long)N, aligned, m, w.counts,
                     (unsigned long long*)(out_counts + 1));
  EINX_CHECK_LAUNCH();
  hipLaunchKernelGGL(ev_scan_tiles_kernel, dim3((unsigned)tiles), dim3(SCAN_THREADS), 0, s, w.counts, chunks, w.tile_sums);
  EINX_CHECK_LAUNCH();
  hipLaunchKernelGGL(ev_scan_top_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, w.tile_sums, tiles, (long long*)out_counts);
  EINX_CHECK_LAUNCH();
  hipLaunchKernelGGL(ev_scatter_kernel, dim3((unsigned)chunks), dim3(EV_THREADS), 0, s, x, y, t, p, (long long)N, aligned, m,
                     (const long long*)w.counts, (const long long*)w.tile_sums, out_x, out_y, out_t, out_p);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

/* the chunk size of einx_events_remap: the tests place stream lengths around it */
EINX_EXPORT int einx_events_remap_chunk(void) { return EV_CHUNK; }
