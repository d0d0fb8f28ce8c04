// gt_matches.hip -- ground-truth matches from depth + pose (or a homography) and the matcher's precision / recall against them
// (DESIGN.md section 8e): the consumer of the matcher's output in the reference's matcher validation.
//
// Replaces (reference file:line): core/geometry/gt_generation.py:15-224 (gt_matches_from_pose_depth, gt_matches_from_homography),
// core/geometry/depth.py:9-60 (sample_depth, project with ccth=None), core/geometry/wrappers.py:337-385 (pinhole cam2image),
// core/modules/matchers/lightglue.py:17-63 (matcher_metrics).
//   stage A  gt_project_kernel / gt_warp_kernel: one thread per keypoint, both directions in one launch (the depth sampler and the
//            projection are gt_project.h's, shared with metrics.hip)
//   stage B  gt_label_kernel: one thread per row (column), the other side staged in LDS and read with broadcast loads; no N x M
//            intermediate; gt_finalize_kernel: mutual check + the three-way label
//   stage C  match_pr_kernel: one wave per pair
//   dense    gt_dense_*_kernel (datasets/generate_MVSEC_relative_pose_val.py:194-346, check_indices): both
//            keypoint sets are the pixel grid, one thread per pixel; stage B searches a (2 pos_th + 3)^2 window of the other map
//            instead of all of it, with the same labels bit for bit; per-pair match / visibility counts
// fp32, unfused (-ffp-contract=off).  No floating-point atomics (the dense counts are integer sums): two runs give the same bits.
// Every launch goes on the caller's stream.
#include "einx_common.h"
#include "gt_project.h"

namespace {

// a pair's count as the kernels use it: clamped to [0, cap] (a negative count is an empty side)
__device__ __forceinline__ int gt_count(const int32_t* cnt, int b, int cap) { return max(0, min(cnt[b], cap)); }

constexpr int GT_CHUNK = 1024;  // points of the other side per LDS stage: 5 words each, 20 KB

struct GtSide {
  const float* kp;      // [B,cap,cols]
  const int32_t* cnt;   // [B]
  const float* depth;   // [B,H,W] or null (precomputed depths)
  const float* K;       // [B,9]
  const float* T;       // [B,16] this side -> the other, or null: the inverse of T_other
  const float* T_other; // [B,16] the other side -> this one
  const float* dk_in;   // [B,cap] precomputed depths or null
  const uint8_t* vk_in; // [B,cap]
  float* dk;            // [B,cap]
  uint8_t* valid;       // [B,cap]
  float* proj;          // [B,cap,2]
  uint8_t* vis;         // [B,cap]
  int cap, cols, H, W;
};

struct GtProjArgs {
  GtSide s[2];
  int kp_yx;
};

__global__ __launch_bounds__(256) void gt_project_kernel(const GtProjArgs a) {
  const int b = blockIdx.y;
  const int blocks0 = einx_cdiv(a.s[0].cap, 256);
  const int side = (int)blockIdx.x >= blocks0 ? 1 : 0;
  const GtSide& s = a.s[side];
  const GtSide& o = a.s[1 - side];
  const int i = ((int)blockIdx.x - (side ? blocks0 : 0)) * 256 + threadIdx.x;
  if (i >= s.cap) return;
  const size_t r = (size_t)b * s.cap + i;
  const int cnt = gt_count(s.cnt, b, s.cap);
  if (i >= cnt) {
    s.dk[r] = 0.0f;
    s.valid[r] = 0;
    s.vis[r] = 0;
    s.proj[2 * r] = 0.0f;
    s.proj[2 * r + 1] = 0.0f;
    return;
  }
  const float* k = s.kp + r * s.cols;
  const float x = k[a.kp_yx ? 1 : 0], y = k[a.kp_yx ? 0 : 1];
  float d;
  bool valid;
  if (s.dk_in) {
    d = s.dk_in[r];
    valid = s.vk_in[r] != 0;
  } else {
    d = gt_sample_depth(s.depth + (size_t)b * s.H * s.W, s.H, s.W, x, y);
    valid = d == d && d > 0.0f;
  }
  float u, v;
  const bool seen = gt_project_point(x, y, d, s.K + b * 9, o.K + b * 9, s.T ? s.T + b * 16 : nullptr,
                                     s.T ? nullptr : s.T_other + b * 16, &u, &v);
  s.dk[r] = d;
  s.valid[r] = valid;
  s.proj[2 * r] = u;
  s.proj[2 * r + 1] = v;
  s.vis[r] = valid && seen;
}

struct GtWarpArgs {
  const float *kp0, *kp1, *H;  // H [B,9]
  const int32_t *n, *m;
  float *proj01, *proj10;
  int cap0, cap1, cols0, cols1, kp_yx;
};

// warp_points_torch (homography.py:161-180): (H [x,y,1])[:2] / ((H [x,y,1])[2] + 1e-5); side 1 with inverse(H) rounded to fp32,
// from the adjugate in double
__global__ __launch_bounds__(256) void gt_warp_kernel(const GtWarpArgs a) {
  __shared__ float h[9];  // H for a side-0 workgroup, inverse(H) for a side-1 workgroup: computed once, by thread 0
  const int b = blockIdx.y;
  const int blocks0 = einx_cdiv(a.cap0, 256);
  const int side = (int)blockIdx.x >= blocks0 ? 1 : 0;
  if (threadIdx.x == 0) {
    const float* Hb = a.H + b * 9;
    if (!side) {
#pragma unroll
      for (int q = 0; q < 9; ++q) h[q] = Hb[q];
    } else {
      double g[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) g[q] = (double)Hb[q];
      const double c00 = g[4] * g[8] - g[5] * g[7], c01 = g[5] * g[6] - g[3] * g[8], c02 = g[3] * g[7] - g[4] * g[6];
      const double det = g[0] * c00 + g[1] * c01 + g[2] * c02;
      h[0] = (float)(c00 / det);
      h[1] = (float)((g[2] * g[7] - g[1] * g[8]) / det);
      h[2] = (float)((g[1] * g[5] - g[2] * g[4]) / det);
      h[3] = (float)(c01 / det);
      h[4] = (float)((g[0] * g[8] - g[2] * g[6]) / det);
      h[5] = (float)((g[2] * g[3] - g[0] * g[5]) / det);
      h[6] = (float)(c02 / det);
      h[7] = (float)((g[1] * g[6] - g[0] * g[7]) / det);
      h[8] = (float)((g[0] * g[4] - g[1] * g[3]) / det);
    }
  }
  __syncthreads();
  const int i = ((int)blockIdx.x - (side ? blocks0 : 0)) * 256 + threadIdx.x;
  const int cap = side ? a.cap1 : a.cap0, cols = side ? a.cols1 : a.cols0;
  if (i >= cap) return;
  const size_t r = (size_t)b * cap + i;
  float* out = (side ? a.proj10 : a.proj01) + 2 * r;
  if (i >= gt_count(side ? a.m : a.n, b, cap)) {
    out[0] = 0.0f;
    out[1] = 0.0f;
    return;
  }
  const float* k = (side ? a.kp1 : a.kp0) + r * cols;
  const float x = k[a.kp_yx ? 1 : 0], y = k[a.kp_yx ? 0 : 1];
  const float wx = (x * h[0] + y * h[1]) + h[2];
  const float wy = (x * h[3] + y * h[4]) + h[5];
  const float ww = ((x * h[6] + y * h[7]) + h[8]) + 1e-5f;
  out[0] = wx / ww;
  out[1] = wy / ww;
}

struct GtLabelArgs {
  const float *kp0, *kp1, *proj01, *proj10;
  const uint8_t *vis0, *vis1, *valid0, *valid1;  // null: every point visible / valid (the homography form)
  const int32_t *n, *m;
  int32_t *min0, *min1;   // ws: arg-min of dist per row / column
  float *dmin0, *dmin1;   // ws: dist at the arg-min
  float *near0, *near1;   // ws: min dist0 per row, min dist1 per column, over ALL points of the other side
  int64_t *matches0, *matches1;
  float *scores0, *scores1;
  int32_t* pos0;          // [B,cap0] or null
  int cap0, cap1, cols0, cols1, kp_yx;
  float pos_sq, neg_sq;
};

// Rows (blockIdx.x < blocks0) and columns of dist = max(dist0, dist1) masked by visibility.  With "self" the side whose point the
// thread owns: a = |self.proj - other.kp|^2, c = |self.kp - other.proj|^2; for a row these are (dist0, dist1), for a column
// (dist1, dist0), so both kinds of workgroup run the same code on swapped pointers and evaluate bit-identical dist[i,j].
__global__ __launch_bounds__(256) void gt_label_kernel(const GtLabelArgs a) {
  // structure of arrays, read four points at a time (ds_read_b128, the same address in every lane: a broadcast)
  __shared__ __attribute__((aligned(16))) float s_kx[GT_CHUNK], s_ky[GT_CHUNK], s_px[GT_CHUNK], s_py[GT_CHUNK];
  __shared__ __attribute__((aligned(16))) int s_vis[GT_CHUNK];
  const int b = blockIdx.y;
  const int blocks0 = einx_cdiv(a.cap0, 256);
  const int side = (int)blockIdx.x >= blocks0 ? 1 : 0;
  const int tid = threadIdx.x;
  const int i = ((int)blockIdx.x - (side ? blocks0 : 0)) * 256 + tid;
  const int n = gt_count(a.n, b, a.cap0), m = gt_count(a.m, b, a.cap1);
  const int cs = side ? a.cap1 : a.cap0, co = side ? a.cap0 : a.cap1;
  const int ns = side ? m : n, no = side ? n : m;
  const int cols_s = side ? a.cols1 : a.cols0, cols_o = side ? a.cols0 : a.cols1;
  const float* kp_s = (side ? a.kp1 : a.kp0) + (size_t)b * cs * cols_s;
  const float* kp_o = (side ? a.kp0 : a.kp1) + (size_t)b * co * cols_o;
  const float* pr_s = (side ? a.proj10 : a.proj01) + (size_t)b * cs * 2;
  const float* pr_o = (side ? a.proj01 : a.proj10) + (size_t)b * co * 2;
  const uint8_t* vis_s = side ? a.vis1 : a.vis0;
  const uint8_t* vis_o = side ? a.vis0 : a.vis1;
  const int xi = a.kp_yx ? 1 : 0, yi = a.kp_yx ? 0 : 1;
  if (i - tid >= ns) return;  // the whole workgroup is past the count (uniform: i - tid is the workgroup's first row)
  const bool live = i < ns;
  float kx = 0.0f, ky = 0.0f, px = 0.0f, py = 0.0f;
  bool vis = false;
  if (live) {
    kx = kp_s[(size_t)i * cols_s + xi];
    ky = kp_s[(size_t)i * cols_s + yi];
    px = pr_s[2 * i];
    py = pr_s[2 * i + 1];
    vis = vis_s ? vis_s[(size_t)b * cs + i] != 0 : true;
  }
  const float inf = einx_u2f(0x7f800000u);
  float best = inf, near = inf;
  int arg = 0;
  for (int j0 = 0; j0 < no; j0 += GT_CHUNK) {
    const int cnt = min(GT_CHUNK, no - j0);
    __syncthreads();
    const int cnt4 = (cnt + 3) & ~3;  // the last group of four is padded with NaN points: they win no comparison
    for (int j = tid; j < cnt4; j += 256) {
      const bool in = j < cnt;
      const int jj = in ? j0 + j : j0;
      const float nanv = einx_u2f(0x7fc00000u);
      s_kx[j] = in ? kp_o[(size_t)jj * cols_o + xi] : nanv;
      s_ky[j] = in ? kp_o[(size_t)jj * cols_o + yi] : nanv;
      s_px[j] = in ? pr_o[2 * jj] : nanv;
      s_py[j] = in ? pr_o[2 * jj + 1] : nanv;
      s_vis[j] = in ? (vis_o ? (int)vis_o[(size_t)b * co + jj] : 1) : 0;
    }
    __syncthreads();
    if (live) {
      for (int j = 0; j < cnt4; j += 4) {
        const f32x4 okx = *reinterpret_cast<const f32x4*>(&s_kx[j]), oky = *reinterpret_cast<const f32x4*>(&s_ky[j]);
        const f32x4 opx = *reinterpret_cast<const f32x4*>(&s_px[j]), opy = *reinterpret_cast<const f32x4*>(&s_py[j]);
        const int4 ov = *reinterpret_cast<const int4*>(&s_vis[j]);
        const int ovis[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float ax = px - okx[u], ay = py - oky[u];
          const float cx = kx - opx[u], cy = ky - opy[u];
          const float da = ax * ax + ay * ay;
          const float dc = cx * cx + cy * cy;
          if (da < near) near = da;
          const float d = (vis && ovis[u]) ? fmaxf(da, dc) : inf;
          if (d < best) {  // strict: the lowest index wins a tie; an all-inf row keeps 0
            best = d;
            arg = j0 + j + u;
          }
        }
      }
    }
  }
  if (live) {
    const size_t r = (size_t)b * cs + i;
    (side ? a.min1 : a.min0)[r] = arg;
    (side ? a.dmin1 : a.dmin0)[r] = best;
    (side ? a.near1 : a.near0)[r] = near;
  }
}

__global__ __launch_bounds__(256) void gt_finalize_kernel(const GtLabelArgs a) {
  const int b = blockIdx.y;
  const int blocks0 = einx_cdiv(a.cap0, 256);
  const int side = (int)blockIdx.x >= blocks0 ? 1 : 0;
  const int i = ((int)blockIdx.x - (side ? blocks0 : 0)) * 256 + threadIdx.x;
  const int cs = side ? a.cap1 : a.cap0, co = side ? a.cap0 : a.cap1;
  if (i >= cs) return;
  const int n = gt_count(a.n, b, a.cap0), m = gt_count(a.m, b, a.cap1);
  const int ns = side ? m : n;
  const size_t r = (size_t)b * cs + i;
  int64_t* matches = side ? a.matches1 : a.matches0;
  float* scores = side ? a.scores1 : a.scores0;
  long long label;
  int pos = -1;
  if (i >= ns) {
    label = -2;  // IGNORE_FEATURE: a row past the pair's count
  } else if (n == 0 || m == 0) {
    label = -1;  // the reference's early return
  } else {
    const int32_t* min_s = (side ? a.min1 : a.min0) + (size_t)b * cs;
    const int32_t* min_o = (side ? a.min0 : a.min1) + (size_t)b * co;
    const int j = min_s[i];
    if (min_o[j] == i && (side ? a.dmin1 : a.dmin0)[r] < a.pos_sq) pos = j;
    const uint8_t* valid = side ? a.valid1 : a.valid0;
    const bool neg = (valid ? valid[r] != 0 : true) && (side ? a.near1 : a.near0)[r] > a.neg_sq;
    label = neg ? -1 : (pos >= 0 ? pos : -2);
  }
  matches[r] = label;
  scores[r] = label > -1 ? 1.0f : 0.0f;
  if (!side && a.pos0) a.pos0[r] = pos;
}

// matcher_metrics (lightglue.py:17-63) of one pair per wave, over its first n[b] rows: recall, precision, accuracy and the
// closed form of ranking_ap = precision * (recall - r_first), r_first taken at the highest-score row (lowest index on a tie)
__global__ __launch_bounds__(64) void match_pr_kernel(const int64_t* matches0, const float* scores0, const int64_t* gt0, const int32_t* n,
                                                      int cap0, double* out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int cnt = gt_count(n, b, cap0);
  const int64_t* mm = matches0 + (size_t)b * cap0;
  const int64_t* gg = gt0 + (size_t)b * cap0;
  const float* sc = scores0 + (size_t)b * cap0;
  int tp_r = 0, c_r = 0, tp_a = 0, c_a = 0, tp_p = 0, c_p = 0;
  float top = -einx_u2f(0x7f800000u);
  int top_i = 0x7fffffff;
  for (int i = lane; i < cnt; i += 64) {
    const long long mi = mm[i], gi = gg[i];
    const int eq = mi == gi;
    const int mr = gi > -1, ma = gi >= -1, mp = mi > -1 && gi >= -1;
    tp_r += eq & mr;
    c_r += mr;
    tp_a += eq & ma;
    c_a += ma;
    tp_p += eq & mp;
    c_p += mp;
    const float s = sc[i];
    if (s > top || top_i == 0x7fffffff) {  // ascending i per lane: the first of equal scores stays
      top = s;
      top_i = i;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    tp_r += __shfl_xor(tp_r, off, 64);
    c_r += __shfl_xor(c_r, off, 64);
    tp_a += __shfl_xor(tp_a, off, 64);
    c_a += __shfl_xor(c_a, off, 64);
    tp_p += __shfl_xor(tp_p, off, 64);
    c_p += __shfl_xor(c_p, off, 64);
    const float os = __shfl_xor(top, off, 64);
    const int oi = __shfl_xor(top_i, off, 64);
    if (oi != 0x7fffffff && (top_i == 0x7fffffff || os > top || (os == top && oi < top_i))) {
      top = os;
      top_i = oi;
    }
  }
  if (lane == 0) {
    double* o = out + (size_t)b * 4;
    if (cnt <= 0) {
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      o[0] = o[1] = o[2] = o[3] = nan;
      return;
    }
    const double recall = (double)tp_r / (1e-8 + (double)c_r);
    const double precision = (double)tp_p / (1e-8 + (double)c_p);
    const double accuracy = (double)tp_a / (1e-8 + (double)c_a);
    const int first = (mm[top_i] == gg[top_i]) && gg[top_i] > -1;
    const double r_first = (double)first / (1e-8 + (double)c_r);
    o[0] = recall;
    o[1] = precision;
    o[2] = accuracy;
    o[3] = precision * (recall - r_first);
  }
}

// ---- both keypoint sets are the pixel grid of their depth map: pixel i = y W + x is the keypoint (x + 0.5, y + 0.5)
struct GtDenseSide {
  const float* depth;    // [F,H,W]
  const int32_t* idx;    // [B] frame of pair b, clamped to [0, F); null: frame b
  const float* K;        // [B,9]
  const float* T;        // [B,16] this side -> the other, or null: the inverse of T_other
  const float* T_other;  // [B,16]
  float* dk;             // outputs [B,H W], each may be null
  uint8_t* valid;
  float* proj_out;       // [B,H W,2]
  uint8_t* vis;
  int64_t* matches;
  float* scores;
  float* proj;           // ws [B,H W,2]
  uint8_t* flags;        // ws [B,H W]: bit 0 visible, bit 1 valid
  uint8_t* neg;          // ws [B,H W]: valid && near > neg_sq
  int32_t* arg;          // ws [B,H W]: the row's arg-min among the candidates with dist < pos_sq, -1 without one
  int F, H, W;
};

struct GtDenseArgs {
  GtDenseSide s[2];
  int32_t* counts;  // [B,4]: #(matches0 > -1), #(matches1 > -1), #visible0, #visible1
  float pos_sq, neg_sq;
};

// the side and the pixel of a thread: side 0's workgroups come first (as in gt_project_kernel)
__device__ __forceinline__ int gt_dense_pixel(const GtDenseArgs& a, int* side) {
  const int blocks0 = einx_cdiv(a.s[0].H * a.s[0].W, 256);
  *side = (int)blockIdx.x >= blocks0 ? 1 : 0;
  return ((int)blockIdx.x - (*side ? blocks0 : 0)) * 256 + threadIdx.x;
}

// stage A: gt_project_kernel's work for the pixel centres; also zeroes the pair's counts for gt_dense_finalize_kernel
__global__ __launch_bounds__(256) void gt_dense_project_kernel(const GtDenseArgs a) {
  const int b = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x < 4) a.counts[4 * b + threadIdx.x] = 0;
  int side;
  const int i = gt_dense_pixel(a, &side);
  const GtDenseSide& s = a.s[side];
  const GtDenseSide& o = a.s[1 - side];
  const int npix = s.H * s.W;
  if (i >= npix) return;
  const int f = s.idx ? max(0, min(s.idx[b], s.F - 1)) : b;
  const float x = (float)(i % s.W) + 0.5f, y = (float)(i / s.W) + 0.5f;
  const float d = gt_sample_depth(s.depth + (size_t)f * npix, s.H, s.W, x, y);
  const bool valid = d == d && d > 0.0f;
  float u, v;
  const bool seen = gt_project_point(x, y, d, s.K + b * 9, o.K + b * 9, s.T ? s.T + b * 16 : nullptr,
                                     s.T ? nullptr : s.T_other + b * 16, &u, &v);
  const bool vis = valid && seen;
  const size_t r = (size_t)b * npix + i;
  s.proj[2 * r] = u;
  s.proj[2 * r + 1] = v;
  s.flags[r] = (uint8_t)((vis ? 1 : 0) | (valid ? 2 : 0));
  if (s.dk) s.dk[r] = d;
  if (s.valid) s.valid[r] = valid;
  if (s.vis) s.vis[r] = vis;
  if (s.proj_out) {
    s.proj_out[2 * r] = u;
    s.proj_out[2 * r + 1] = v;
  }
}

// stage B: gt_label_kernel's row (column) of pixel i restricted to the pixels of the other map within r = pos_th + 1 of its
// projection p, in raster order.  dist >= |p - kp_other|^2, so every candidate with dist < pos_sq is inside the box, and the
// arg-min over them is the row's global arg-min whenever that can become a positive.  kp_other is x + 0.5f.
__global__ __launch_bounds__(256) void gt_dense_label_kernel(const GtDenseArgs a) {
  const int b = blockIdx.y;
  int side;
  const int i = gt_dense_pixel(a, &side);
  const GtDenseSide& s = a.s[side];
  const GtDenseSide& o = a.s[1 - side];
  if (i >= s.H * s.W) return;
  const size_t r = (size_t)b * s.H * s.W + i;
  const size_t ro = (size_t)b * o.H * o.W;
  const float inf = einx_u2f(0x7f800000u);
  const float kx = (float)(i % s.W) + 0.5f, ky = (float)(i / s.W) + 0.5f;
  const float px = s.proj[2 * r], py = s.proj[2 * r + 1];
  const int fl = s.flags[r];
  float best = inf;
  int arg = -1;
  if ((fl & 1) && fabsf(px) < inf && fabsf(py) < inf) {  // an invisible row has dist = inf everywhere; NaN / inf: an empty box
    const float rad = sqrtf(a.pos_sq) + 1.0f;
    // |x + 0.5 - p.x| <= rad, clamped to the map in float so that the conversions are defined
    const int x0 = (int)fminf(fmaxf(ceilf(px - rad - 0.5f), 0.0f), (float)o.W);
    const int x1 = (int)fmaxf(fminf(floorf(px + rad - 0.5f), (float)(o.W - 1)), -1.0f);
    const int y0 = (int)fminf(fmaxf(ceilf(py - rad - 0.5f), 0.0f), (float)o.H);
    const int y1 = (int)fmaxf(fminf(floorf(py + rad - 0.5f), (float)(o.H - 1)), -1.0f);
    for (int yy = y0; yy <= y1; ++yy) {
      const float oky = (float)yy + 0.5f;
      for (int xx = x0; xx <= x1; ++xx) {
        const int j = yy * o.W + xx;
        // the flag first: a byte per candidate, and the 8 bytes of the projection only where it counts (one 8-byte load of a
        // NaN-masked projection for every candidate instead was measured: 0.93 ms against 0.69 ms at B = 32, 260 x 346, 6.8 % holes)
        if (!(o.flags[ro + j] & 1)) continue;  // dist = inf
        const float okx = (float)xx + 0.5f;
        const float opx = o.proj[2 * (ro + j)], opy = o.proj[2 * (ro + j) + 1];
        const float ax = px - okx, ay = py - oky;
        const float cx = kx - opx, cy = ky - opy;
        const float da = ax * ax + ay * ay;
        const float dc = cx * cx + cy * cy;
        const float d = fmaxf(da, dc);
        if (d < a.pos_sq && d < best) {  // strict: the lowest raster index wins a tie
          best = d;
          arg = j;
        }
      }
    }
  }
  // min_j dist0[i,j] over ALL j: the distance to the nearest pixel centre, clamped to the map (fp32 rounding is monotone, so the
  // minimum of (p.x - cx)^2 + (p.y - cy)^2 sits at the nearest column and the nearest row); NaN compares false everywhere: +inf
  const float ncx = fminf(fmaxf(floorf(px), 0.0f), (float)(o.W - 1)) + 0.5f;
  const float ncy = fminf(fmaxf(floorf(py), 0.0f), (float)(o.H - 1)) + 0.5f;
  const float nx = px - ncx, ny = py - ncy;
  const float dn = nx * nx + ny * ny;
  const float near = dn == dn ? dn : inf;
  s.arg[r] = arg;
  s.neg[r] = (fl & 2) && near > a.neg_sq;
}

constexpr int GT_DENSE_FIN = 8;  // pixels per thread of gt_dense_finalize_kernel: 2048 per workgroup

// mutual check, the three-way label and stage C.  The counts are integer sums, so two runs give the same bits; a workgroup adds its
// 2048 pixels up before its one atomicAdd per counter (one per wave made the launch wait on ~180,000 atomics to 128 words at
// B = 32, 260 x 346: 0.77 ms, more than the labelling itself; now 0.04 ms)
__global__ __launch_bounds__(256) void gt_dense_finalize_kernel(const GtDenseArgs a) {
  __shared__ int s_nm[4], s_nv[4];
  const int b = blockIdx.y;
  const int per = 256 * GT_DENSE_FIN;
  const int blocks0 = einx_cdiv(a.s[0].H * a.s[0].W, per);
  const int side = (int)blockIdx.x >= blocks0 ? 1 : 0;
  const GtDenseSide& s = a.s[side];
  const GtDenseSide& o = a.s[1 - side];
  const int npix = s.H * s.W;
  const int first = ((int)blockIdx.x - (side ? blocks0 : 0)) * per + threadIdx.x;
  int nm = 0, nv = 0;
#pragma unroll
  for (int k = 0; k < GT_DENSE_FIN; ++k) {
    const int i = first + 256 * k;
    if (i >= npix) break;
    const size_t r = (size_t)b * npix + i;
    const int j = s.arg[r];
    const int pos = (j >= 0 && o.arg[(size_t)b * o.H * o.W + j] == i) ? j : -1;
    const long long label = s.neg[r] ? -1 : (pos >= 0 ? pos : -2);
    nm += label > -1;
    nv += s.flags[r] & 1;
    if (s.matches) s.matches[r] = label;
    if (s.scores) s.scores[r] = label > -1 ? 1.0f : 0.0f;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    nm += __shfl_xor(nm, off, 64);
    nv += __shfl_xor(nv, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_nm[threadIdx.x >> 6] = nm;
    s_nv[threadIdx.x >> 6] = nv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    nm = (s_nm[0] + s_nm[1]) + (s_nm[2] + s_nm[3]);
    nv = (s_nv[0] + s_nv[1]) + (s_nv[2] + s_nv[3]);
    if (nm) atomicAdd(a.counts + 4 * b + side, nm);
    if (nv) atomicAdd(a.counts + 4 * b + 2 + side, nv);
  }
}

bool dense_params_ok(const einx_gt_dense_params* p) {
  return p && p->struct_size == sizeof(einx_gt_dense_params) && p->B > 0 && p->B <= 65535 && p->F0 > 0 && p->F1 > 0 && p->H0 > 0 &&
         p->W0 > 0 && p->H1 > 0 && p->W1 > 0 && (int64_t)p->H0 * p->W0 <= (1 << 24) && (int64_t)p->H1 * p->W1 <= (1 << 24) &&
         p->pos_sq > 0.0f && p->pos_sq < einx_u2f(0x7f800000u) && p->neg_sq >= 0.0f;
}

// einx_gt_dense's workspace: O(B (H0 W0 + H1 W1)), no N x M term; and 256 bytes of slack
void dense_carve(WsCarver& c, GtDenseArgs& a, const einx_gt_dense_params* p) {
  const size_t n[2] = {(size_t)p->B * p->H0 * p->W0, (size_t)p->B * p->H1 * p->W1};
  for (int side = 0; side < 2; ++side) {
    a.s[side].proj = c.take<float>(2 * n[side]);
    a.s[side].arg = c.take<int32_t>(n[side]);
    a.s[side].flags = c.take<uint8_t>(n[side]);
    a.s[side].neg = c.take<uint8_t>(n[side]);
  }
  c.slack(256);
}

bool params_ok(const einx_gt_matches_params* p) {
  return p && p->struct_size == sizeof(einx_gt_matches_params) && p->B > 0 && p->B <= 65535 && p->cap0 > 0 && p->cap1 > 0 && p->cols0 >= 2 &&
         p->cols1 >= 2 && p->cap0 <= (1 << 24) && p->cap1 <= (1 << 24);
}

// einx_gt_label's workspace (einx_gt_matches uses the same one), and 256 bytes of slack
void carve(WsCarver& c, GtLabelArgs& a, const einx_gt_matches_params* p) {
  const size_t n0 = (size_t)p->B * p->cap0, n1 = (size_t)p->B * p->cap1;
  a.min0 = c.take<int32_t>(n0);
  a.min1 = c.take<int32_t>(n1);
  a.dmin0 = c.take<float>(n0);
  a.dmin1 = c.take<float>(n1);
  a.near0 = c.take<float>(n0);
  a.near1 = c.take<float>(n1);
  c.slack(256);
}

dim3 both_sides_grid(const einx_gt_matches_params* p) {
  return dim3((unsigned)(einx_cdiv(p->cap0, 256) + einx_cdiv(p->cap1, 256)), (unsigned)p->B);
}

}  // namespace

EINX_EXPORT size_t einx_gt_matches_ws_bytes(const einx_gt_matches_params* p) {
  if (!params_ok(p)) return 0;
  WsCarver c{nullptr};
  GtLabelArgs a;
  carve(c, a, p);
  return c.bytes;
}

EINX_EXPORT int einx_gt_project(const einx_gt_matches_params* p, const float* kp0, const float* kp1, const int32_t* n, const int32_t* m,
                                const float* depth0, const float* depth1, const float* K0, const float* K1, const float* T_0to1,
                                const float* T_1to0, const float* dk0_in, const float* dk1_in, const uint8_t* vk0_in, const uint8_t* vk1_in,
                                float* dk0, float* dk1, uint8_t* valid0, uint8_t* valid1, float* proj01, float* proj10, uint8_t* vis0,
                                uint8_t* vis1, void* stream) {
  EINX_CHECK_ARG(params_ok(p), "bad params (struct_size, shape)");
  EINX_CHECK_ARG(kp0 && kp1 && n && m && K0 && K1 && T_0to1, "null pointer");
  EINX_CHECK_ARG(dk0 && dk1 && valid0 && valid1 && proj01 && proj10 && vis0 && vis1, "null output");
  const bool pre = dk0_in || dk1_in || vk0_in || vk1_in;
  EINX_CHECK_ARG(!pre || (dk0_in && dk1_in && vk0_in && vk1_in), "precomputed depths need all four arrays");
  EINX_CHECK_ARG(pre || (depth0 && depth1 && p->H0 > 0 && p->W0 > 0 && p->H1 > 0 && p->W1 > 0), "depth maps missing");
  GtProjArgs a;
  a.kp_yx = p->kp_yx;
  a.s[0] = GtSide{kp0, n, pre ? nullptr : depth0, K0, T_0to1, T_1to0, dk0_in, vk0_in, dk0, valid0, proj01, vis0, p->cap0, p->cols0, p->H0, p->W0};
  a.s[1] = GtSide{kp1, m, pre ? nullptr : depth1, K1, T_1to0, T_0to1, dk1_in, vk1_in, dk1, valid1, proj10, vis1, p->cap1, p->cols1, p->H1, p->W1};
  EINX_PROF("gt_project", stream);
  hipLaunchKernelGGL(gt_project_kernel, both_sides_grid(p), dim3(256), 0, (hipStream_t)stream, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_gt_warp(const einx_gt_matches_params* p, const float* kp0, const float* kp1, const int32_t* n, const int32_t* m,
                             const float* H, float* proj01, float* proj10, void* stream) {
  EINX_CHECK_ARG(params_ok(p), "bad params (struct_size, shape)");
  EINX_CHECK_ARG(kp0 && kp1 && n && m && H && proj01 && proj10, "null pointer");
  GtWarpArgs a{kp0, kp1, H, n, m, proj01, proj10, p->cap0, p->cap1, p->cols0, p->cols1, p->kp_yx};
  EINX_PROF("gt_warp", stream);
  hipLaunchKernelGGL(gt_warp_kernel, both_sides_grid(p), dim3(256), 0, (hipStream_t)stream, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_gt_label(const einx_gt_matches_params* p, const float* kp0, const float* kp1, const int32_t* n, const int32_t* m,
                              const float* proj01, const float* proj10, const uint8_t* vis0, const uint8_t* vis1, const uint8_t* valid0,
                              const uint8_t* valid1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1,
                              int32_t* pos0, void* stream) {
  EINX_CHECK_ARG(params_ok(p), "bad params (struct_size, shape)");
  EINX_CHECK_ARG(kp0 && kp1 && n && m && proj01 && proj10 && ws && matches0 && matches1 && scores0 && scores1, "null pointer");
  EINX_CHECK_ARG((vis0 != nullptr) == (vis1 != nullptr) && (valid0 != nullptr) == (valid1 != nullptr), "visibility / validity of one side only");
  GtLabelArgs a;
  a.kp0 = kp0;
  a.kp1 = kp1;
  a.proj01 = proj01;
  a.proj10 = proj10;
  a.vis0 = vis0;
  a.vis1 = vis1;
  a.valid0 = valid0;
  a.valid1 = valid1;
  a.n = n;
  a.m = m;
  a.matches0 = matches0;
  a.matches1 = matches1;
  a.scores0 = scores0;
  a.scores1 = scores1;
  a.pos0 = pos0;
  a.cap0 = p->cap0;
  a.cap1 = p->cap1;
  a.cols0 = p->cols0;
  a.cols1 = p->cols1;
  a.kp_yx = p->kp_yx;
  a.pos_sq = p->pos_sq;
  a.neg_sq = p->neg_sq;
  WsCarver c{(char*)ws};
  carve(c, a, p);
  hipStream_t s = (hipStream_t)stream;
  {
    EINX_PROF("gt_label", stream);
    hipLaunchKernelGGL(gt_label_kernel, both_sides_grid(p), dim3(256), 0, s, a);
    EINX_CHECK_LAUNCH();
  }
  EINX_PROF("gt_finalize", stream);
  hipLaunchKernelGGL(gt_finalize_kernel, both_sides_grid(p), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_gt_matches(const einx_gt_matches_params* p, const float* kp0, const float* kp1, const int32_t* n, const int32_t* m,
                                const float* depth0, const float* depth1, const float* K0, const float* K1, const float* T_0to1,
                                const float* T_1to0, const float* dk0_in, const float* dk1_in, const uint8_t* vk0_in, const uint8_t* vk1_in,
                                const float* H, void* ws, float* dk0, float* dk1, uint8_t* valid0, uint8_t* valid1, float* proj01,
                                float* proj10, uint8_t* vis0, uint8_t* vis1, int64_t* matches0, int64_t* matches1, float* scores0,
                                float* scores1, int32_t* pos0, void* stream) {
  EINX_CHECK_ARG(params_ok(p), "bad params (struct_size, shape)");
  if (p->homography) {
    const int rc = einx_gt_warp(p, kp0, kp1, n, m, H, proj01, proj10, stream);
    if (rc != EINX_OK) return rc;
    return einx_gt_label(p, kp0, kp1, n, m, proj01, proj10, nullptr, nullptr, nullptr, nullptr, ws, matches0, matches1, scores0, scores1,
                         pos0, stream);
  }
  const int rc = einx_gt_project(p, kp0, kp1, n, m, depth0, depth1, K0, K1, T_0to1, T_1to0, dk0_in, dk1_in, vk0_in, vk1_in, dk0, dk1, valid0,
                                 valid1, proj01, proj10, vis0, vis1, stream);
  if (rc != EINX_OK) return rc;
  return einx_gt_label(p, kp0, kp1, n, m, proj01, proj10, vis0, vis1, valid0, valid1, ws, matches0, matches1, scores0, scores1, pos0, stream);
}

EINX_EXPORT int einx_match_pr(const int64_t* matches0, const float* scores0, const int64_t* gt_matches0, const int32_t* n, int B, int cap0,
                              double* out, void* stream) {
  EINX_CHECK_ARG(matches0 && scores0 && gt_matches0 && n && out, "null pointer");
  EINX_CHECK_ARG(B > 0 && cap0 > 0, "bad shape");
  EINX_PROF("match_pr", stream);
  hipLaunchKernelGGL(match_pr_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, matches0, scores0, gt_matches0, n, cap0, out);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT size_t einx_gt_dense_ws_bytes(const einx_gt_dense_params* p) {
  if (!dense_params_ok(p)) return 0;
  WsCarver c{nullptr};
  GtDenseArgs a;
  dense_carve(c, a, p);
  return c.bytes;
}

EINX_EXPORT int einx_gt_dense(const einx_gt_dense_params* p, const float* depth0, const float* depth1, const int32_t* idx0,
                              const int32_t* idx1, const float* K0, const float* K1, const float* T_0to1, const float* T_1to0, void* ws,
                              float* dk0, float* dk1, uint8_t* valid0, uint8_t* valid1, float* proj01, float* proj10, uint8_t* vis0,
                              uint8_t* vis1, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, int32_t* counts,
                              void* stream) {
  EINX_CHECK_ARG(dense_params_ok(p), "bad params (struct_size, shape, pos_sq must be finite and > 0)");
  EINX_CHECK_ARG(depth0 && depth1 && K0 && K1 && T_0to1 && ws && counts, "null pointer");
  EINX_CHECK_ARG((idx0 || p->F0 >= p->B) && (idx1 || p->F1 >= p->B), "without frame indices a stack needs a frame per pair");
  GtDenseArgs a;
  a.s[0] = GtDenseSide{depth0, idx0, K0, T_0to1, T_1to0, dk0, valid0, proj01, vis0, matches0, scores0, nullptr, nullptr, nullptr, nullptr,
                       p->F0, p->H0, p->W0};
  a.s[1] = GtDenseSide{depth1, idx1, K1, T_1to0, T_0to1, dk1, valid1, proj10, vis1, matches1, scores1, nullptr, nullptr, nullptr, nullptr,
                       p->F1, p->H1, p->W1};
  a.counts = counts;
  a.pos_sq = p->pos_sq;
  a.neg_sq = p->neg_sq;
  WsCarver c{(char*)ws};
  dense_carve(c, a, p);
  const dim3 grid((unsigned)(einx_cdiv(p->H0 * p->W0, 256) + einx_cdiv(p->H1 * p->W1, 256)), (unsigned)p->B);
  hipStream_t s = (hipStream_t)stream;
  {
    EINX_PROF("gt_dense_project", stream);
    hipLaunchKernelGGL(gt_dense_project_kernel, grid, dim3(256), 0, s, a);
    EINX_CHECK_LAUNCH();
  }
  {
    EINX_PROF("gt_dense_label", stream);
    hipLaunchKernelGGL(gt_dense_label_kernel, grid, dim3(256), 0, s, a);
    EINX_CHECK_LAUNCH();
  }
  EINX_PROF("gt_dense_finalize", stream);
  const int per = 256 * GT_DENSE_FIN;
  const dim3 fin_grid((unsigned)(einx_cdiv(p->H0 * p->W0, per) + einx_cdiv(p->H1 * p->W1, per)), (unsigned)p->B);
  hipLaunchKernelGGL(gt_dense_finalize_kernel, fin_grid, dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
