// geometry.hip -- core.geometry.depth and core.geometry.epipolar on the device: the projection of keypoints
// or of every pixel into the other view with the reference's cycle ("circle") consistency check, the feature-map sampler, and the
// all-pairs symmetric epipolar distance.
//
// Replaces (reference file:line): core/geometry/depth.py:9-25 (sample_fmap, sample_depth), :37-69 (project, ccth given or None),
// :72-89 (dense_warp_consistency), core/geometry/epipolar.py:59-72 (sym_epipolar_distance_all), core/geometry/wrappers.py:186-193
// (Pose.transform), :337-398 (pinhole cam2image / image2cam).
//   geom_project_kernel     one thread per keypoint, one or both directions in one launch (gt_project_kernel's split of blockIdx.x)
//   geom_dense_warp_kernel  one thread per pixel of depth_i; per-pair integer counts of valid and visible pixels
//   geom_sample_kernel      one thread per (point, channel): stores contiguous in [B,N,C]
//   epipolar_all_kernel     threads along M (a thread owns a column: its point, E^T p1 and the norm live in registers), 32 rows per
//                           workgroup whose lines E p0 and norms are computed once into LDS and read as broadcasts
// The sampler and the projection are gt_project.h's, shared with gt_matches.hip and metrics.hip: one text, the same bits.
// fp32, unfused (-ffp-contract=off).  No floating-point atomics (the counts are integer sums): two runs give the same bits.
// Every launch goes on the caller's stream; nothing allocates or synchronises.
#include "einx_common.h"
#include "gt_project.h"

namespace {

struct GeomProjArgs {
  einx_geom_side s[2];
  int kp_yx, cc;
  float bound;
};

__global__ __launch_bounds__(256) void geom_project_kernel(const GeomProjArgs a) {
  const int b = blockIdx.y;
  const int blocks0 = einx_cdiv(a.s[0].cap, 256);
  const int side = (int)blockIdx.x >= blocks0 ? 1 : 0;
  const einx_geom_side& s = a.s[side];
  const int i = ((int)blockIdx.x - (side ? blocks0 : 0)) * 256 + threadIdx.x;
  if (i >= s.cap) return;
  const size_t r = (size_t)b * s.cap + i;
  const int cnt = s.count ? max(0, min(s.count[b], s.cap)) : s.cap;
  if (i >= cnt) {  // rows past the count: zeros, as einx_gt_project writes them
    if (s.d_out) s.d_out[r] = 0.0f;
    if (s.valid_out) s.valid_out[r] = 0;
    s.visible[r] = 0;
    s.proj[2 * r] = 0.0f;
    s.proj[2 * r + 1] = 0.0f;
    return;
  }
  const float* k = s.kp + r * s.cols;
  const float x = k[a.kp_yx ? 1 : 0], y = k[a.kp_yx ? 0 : 1];
  float d;
  bool valid;
  if (s.d_in) {
    d = s.d_in[r];
    valid = s.valid_in[r] != 0;
  } else {
    d = gt_sample_depth(s.depth + (size_t)b * s.H * s.W, s.H, s.W, x, y);
    valid = d == d && d > 0.0f;
  }
  GtOtherDepth od{nullptr, s.Ho, s.Wo, 0.0f, false};
  if (a.cc) {
    if (s.depth_other) {
      od.dm = s.depth_other + (size_t)b * s.Ho * s.Wo;
    } else {
      od.dj = s.dj_in[r];
      od.validj = s.validj_in[r] != 0;
    }
  }
  float u, v, dj;
  const bool seen = gt_project_cc(x, y, d, s.K + b * 9, s.K_other + b * 9, s.T ? s.T + b * 16 : nullptr,
                                  s.T ? nullptr : s.T_other + b * 16, a.cc != 0, a.bound, od, &u, &v, &dj);
  if (s.d_out) s.d_out[r] = d;
  if (s.valid_out) s.valid_out[r] = valid;
  s.proj[2 * r] = u;
  s.proj[2 * r + 1] = v;
  s.visible[r] = valid && seen;
}

struct GeomDenseArgs {
  einx_geom_dense_side s[2];
  int32_t* counts;  // [B,sides,2]: valid, visible
  int sides, cc;
  float bound;
};

// clears the counts ahead of geom_dense_warp_kernel: a kernel node of its own, so that a captured call replays it like an eager one
__global__ void geom_zero_kernel(int32_t* p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

// depth.py:72-89: the keypoint of pixel i = y W + x is its centre, its depth the pixel's own value (no sampling), valid_i = d > 0.
// The counts are integer sums (one atomicAdd per workgroup and counter): two runs give the same bits.
__global__ __launch_bounds__(256) void geom_dense_warp_kernel(const GeomDenseArgs a) {
  __shared__ int s_nv[4], s_ns[4];
  const int b = blockIdx.y;
  const int blocks0 = einx_cdiv(a.s[0].H * a.s[0].W, 256);
  const int side = (int)blockIdx.x >= blocks0 ? 1 : 0;
  const einx_geom_dense_side& s = a.s[side];
  const int i = ((int)blockIdx.x - (side ? blocks0 : 0)) * 256 + threadIdx.x;
  const int npix = s.H * s.W;
  bool valid = false, vis = false;
  if (i < npix) {
    const size_t r = (size_t)b * npix + i;
    const float x = (float)(i % s.W) + 0.5f, y = (float)(i / s.W) + 0.5f;
    const float d = s.depth[r];
    valid = d > 0.0f;
    const GtOtherDepth od{a.cc ? s.depth_other + (size_t)b * s.Ho * s.Wo : nullptr, s.Ho, s.Wo, 0.0f, false};
    float u, v, dj;
    const bool seen = gt_project_cc(x, y, d, s.K + b * 9, s.K_other + b * 9, s.T ? s.T + b * 16 : nullptr,
                                    s.T ? nullptr : s.T_other + b * 16, a.cc != 0, a.bound, od, &u, &v, &dj);
    vis = valid && seen;
    reinterpret_cast<float2*>(s.warp)[r] = make_float2(u, v);  // 8 bytes per lane, contiguous
    s.visible[r] = vis;
  }
  const int nv = __popcll(__ballot(valid)), ns = __popcll(__ballot(vis));
  if ((threadIdx.x & 63) == 0) {
    s_nv[threadIdx.x >> 6] = nv;
    s_ns[threadIdx.x >> 6] = ns;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tv = (s_nv[0] + s_nv[1]) + (s_nv[2] + s_nv[3]);
    const int ts = (s_ns[0] + s_ns[1]) + (s_ns[2] + s_ns[3]);
    int32_t* c = a.counts + ((size_t)b * a.sides + side) * 2;
    if (tv) atomicAdd(c, tv);
    if (ts) atomicAdd(c + 1, ts);
  }
}

// depth.py:9-25: thread t = n C + c of pair b samples channel c at point n.  depth_rule: a hole is <= 0 or NaN (sample_depth on
// its NaN-masked map), otherwise a NaN; valid (C == 1) = not NaN and > 0
__global__ __launch_bounds__(256) void geom_sample_kernel(const float* fmap, int C, int H, int W, const float* pts, int N, int depth_rule,
                                                          float* out, uint8_t* valid) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= N * C) return;
  const int n = t / C, c = t - n * C;
  const float* p = pts + ((size_t)b * N + n) * 2;
  const float* dm = fmap + ((size_t)b * C + c) * H * W;
  const float v = depth_rule ? gt_sample_map<false>(dm, H, W, p[0], p[1]) : gt_sample_map<true>(dm, H, W, p[0], p[1]);
  out[(size_t)b * N * C + t] = v;
  if (valid) valid[(size_t)b * N + n] = v == v && v > 0.0f;
}

constexpr int EPI_ROWS = 32;  // rows of a workgroup's tile; its 256 threads are 256 columns

// epipolar.py:59-72.  Row n: l = E p0 (l_i = (E[i,0] x + E[i,1] y) + E[i,2] w), n0 = sqrt((l_0^2 + l_1^2) + eps).  Column m:
// c_k = (E[0,k] x' + E[1,k] y') + E[2,k] w' for k = 0, 1, n1 = sqrt((c_0^2 + c_1^2) + eps).  Entry: s = |(x' l_0 + y' l_1) + w' l_2|,
// out = (s / n0 + s / n1) * 0.5.
__global__ __launch_bounds__(256) void epipolar_all_kernel(const float* p0, int cols0, const float* p1, int cols1, const float* E, int N,
                                                           int M, float eps, float* out) {
  __shared__ __attribute__((aligned(16))) float s_row[EPI_ROWS][4];  // l_0, l_1, l_2, n0
  const int b = blockIdx.z;
  const int n0 = blockIdx.y * EPI_ROWS;
  const int tid = threadIdx.x;
  const int j = blockIdx.x * 256 + tid;
  const float* e = E + (size_t)b * 9;
  if (tid < EPI_ROWS && n0 + tid < N) {
    const float* p = p0 + ((size_t)b * N + n0 + tid) * cols0;
    const float x = p[0], y = p[1], w = cols0 == 3 ? p[2] : 1.0f;
    const float l0 = (e[0] * x + e[1] * y) + e[2] * w;
    const float l1 = (e[3] * x + e[4] * y) + e[5] * w;
    const float l2 = (e[6] * x + e[7] * y) + e[8] * w;
    s_row[tid][0] = l0;
    s_row[tid][1] = l1;
    s_row[tid][2] = l2;
    s_row[tid][3] = sqrtf((l0 * l0 + l1 * l1) + eps);
  }
  float x1 = 0.0f, y1 = 0.0f, w1 = 1.0f, n1 = 1.0f;
  if (j < M) {
    const float* p = p1 + ((size_t)b * M + j) * cols1;
    x1 = p[0];
    y1 = p[1];
    w1 = cols1 == 3 ? p[2] : 1.0f;
    const float c0 = (e[0] * x1 + e[3] * y1) + e[6] * w1;
    const float c1 = (e[1] * x1 + e[4] * y1) + e[7] * w1;
    n1 = sqrtf((c0 * c0 + c1 * c1) + eps);
  }
  __syncthreads();
  if (j >= M) return;
  const int rows = min(EPI_ROWS, N - n0);
  float* o = out + ((size_t)b * N + n0) * M + j;
  for (int r = 0; r < rows; ++r) {
    const f32x4 l = *reinterpret_cast<const f32x4*>(&s_row[r][0]);  // the same address in every lane: a broadcast
    const float s = fabsf((x1 * l[0] + y1 * l[1]) + w1 * l[2]);
    o[(size_t)r * M] = (s / l[3] + s / n1) * 0.5f;
  }
}

bool side_dims_ok(int cap, int cols) { return cap > 0 && cap <= (1 << 24) && cols >= 2; }

}  // namespace

EINX_EXPORT int einx_geom_project(const einx_geom_project_params* p, void* stream) {
  EINX_CHECK_ARG(p && p->struct_size == sizeof(einx_geom_project_params), "bad params (struct_size)");
  EINX_CHECK_ARG(p->B > 0 && p->B <= 65535 && (p->sides == 1 || p->sides == 2), "bad shape (B, sides)");
  EINX_CHECK_ARG(!p->cc || p->cc_bound == p->cc_bound, "the cycle-check bound is NaN");
  GeomProjArgs a;
  a.kp_yx = p->kp_yx;
  a.cc = p->cc;
  a.bound = p->cc_bound;
  for (int k = 0; k < p->sides; ++k) {
    const einx_geom_side& s = p->side[k];
    EINX_CHECK_ARG(side_dims_ok(s.cap, s.cols), "bad shape (cap, cols)");
    EINX_CHECK_ARG(s.kp && s.K && s.K_other && (s.T || s.T_other) && s.proj && s.visible, "null pointer");
    EINX_CHECK_ARG((s.d_in != nullptr) == (s.valid_in != nullptr), "given depths need d_in and valid_in");
    EINX_CHECK_ARG(s.d_in || (s.depth && s.H > 0 && s.W > 0), "neither this view's depth map nor given depths");
    if (p->cc) {
      EINX_CHECK_ARG((s.dj_in != nullptr) == (s.validj_in != nullptr), "given depths under the projections need dj_in and validj_in");
      EINX_CHECK_ARG(s.dj_in || (s.depth_other && s.Ho > 0 && s.Wo > 0),
                     "the cycle check needs the other view's depth map or its depths under the projections");
    }
    a.s[k] = s;
  }
  if (p->sides == 1) {
    a.s[1] = a.s[0];
    a.s[1].cap = 0;
  }
  const dim3 grid((unsigned)(einx_cdiv(a.s[0].cap, 256) + einx_cdiv(a.s[1].cap, 256)), (unsigned)p->B);
  EINX_PROF("geom_project", stream);
  hipLaunchKernelGGL(geom_project_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_geom_dense_warp(const einx_geom_dense_params* p, void* stream) {
  EINX_CHECK_ARG(p && p->struct_size == sizeof(einx_geom_dense_params), "bad params (struct_size)");
  EINX_CHECK_ARG(p->B > 0 && p->B <= 65535 && (p->sides == 1 || p->sides == 2), "bad shape (B, sides)");
  EINX_CHECK_ARG(p->counts, "null counts");
  EINX_CHECK_ARG(!p->cc || p->cc_bound == p->cc_bound, "the cycle-check bound is NaN");
  GeomDenseArgs a;
  a.counts = p->counts;
  a.sides = p->sides;
  a.cc = p->cc;
  a.bound = p->cc_bound;
  for (int k = 0; k < p->sides; ++k) {
    const einx_geom_dense_side& s = p->side[k];
    EINX_CHECK_ARG(s.H > 0 && s.W > 0 && (int64_t)s.H * s.W <= (1 << 24), "bad shape (H, W)");
    EINX_CHECK_ARG(s.depth && s.K && s.K_other && (s.T || s.T_other) && s.warp && s.visible, "null pointer");
    EINX_CHECK_ARG(((uintptr_t)s.warp & 7) == 0, "warp must be aligned to 8 bytes");
    EINX_CHECK_ARG(!p->cc || (s.depth_other && s.Ho > 0 && s.Wo > 0), "the cycle check needs the other view's depth map");
    a.s[k] = s;
  }
  if (p->sides == 1) {
    a.s[1] = a.s[0];
    a.s[1].H = 0;
  }
  hipStream_t st = (hipStream_t)stream;
  const int ncounts = 2 * p->sides * p->B;
  hipLaunchKernelGGL(geom_zero_kernel, dim3((unsigned)einx_cdiv(ncounts, 256)), dim3(256), 0, st, p->counts, ncounts);
  EINX_CHECK_LAUNCH();
  const dim3 grid((unsigned)(einx_cdiv(a.s[0].H * a.s[0].W, 256) + einx_cdiv(a.s[1].H * a.s[1].W, 256)), (unsigned)p->B);
  EINX_PROF("geom_dense_warp", stream);
  hipLaunchKernelGGL(geom_dense_warp_kernel, grid, dim3(256), 0, st, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_geom_sample(const float* fmap, int B, int C, int H, int W, const float* pts, int N, int depth_rule, float* out,
                                 uint8_t* valid, void* stream) {
  EINX_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0 && N >= 0, "bad shape");
  EINX_CHECK_ARG((int64_t)N * C < (1ll << 31) && (int64_t)H * W < (1ll << 31), "shape too large (N C and H W must stay below 2^31)");
  EINX_CHECK_ARG(!valid || (depth_rule && C == 1), "valid is written for a depth map only (depth_rule, C == 1)");
  if (N == 0) return EINX_OK;
  EINX_CHECK_ARG(fmap && pts && out, "null pointer");
  EINX_PROF("geom_sample", stream);
  hipLaunchKernelGGL(geom_sample_kernel, dim3((unsigned)einx_cdiv(N * C, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, fmap, C, H,
                     W, pts, N, depth_rule, out, valid);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_epipolar_all(const float* p0, int cols0, const float* p1, int cols1, const float* E, int B, int N, int M, float eps,
                                  float* out, void* stream) {
  EINX_CHECK_ARG(B > 0 && B <= 65535 && N >= 0 && M >= 0 && N <= (1 << 21) && M <= (1 << 24), "bad shape");
  EINX_CHECK_ARG((cols0 == 2 || cols0 == 3) && (cols1 == 2 || cols1 == 3), "points have 2 or 3 columns");
  if (N == 0 || M == 0) return EINX_OK;
  EINX_CHECK_ARG(p0 && p1 && E && out, "null pointer");
  EINX_PROF("epipolar_all", stream);
  const dim3 grid((unsigned)einx_cdiv(M, 256), (unsigned)einx_cdiv(N, EPI_ROWS), (unsigned)B);
  hipLaunchKernelGGL(epipolar_all_kernel, grid, dim3(256), 0, (hipStream_t)stream, p0, cols0, p1, cols1, E, N, M, eps, out);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
