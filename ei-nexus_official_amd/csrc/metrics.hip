// metrics.hip -- the consumers right after the extract+match path: per-pair
// MatchingRatio, MeanMatchingAccuracy@t and ValidDescriptorsDistance (repeatability / descriptor
// distance / angle @t) computed on the device for a whole batch, so the evaluation harness needs no
// per-pair .item() round trips and the multi-GPU job can all-reduce plain sums.
//
// Replaces (reference file:line): core/metrics/matching_metrics.py:30-51 (MatchingRatio),
// :84-156 (MeanMatchingAccuracy), core/metrics/keypoints_metrics.py:160-290
// (ValidDescriptorsDistance), core/metrics/util.py:5-104 (warp_points, keep_true_points).
// Latency-bound integer/compare work on <=1024x1024 point pairs: one wave per keypoint, lanes
// over the other image's keypoints, wave shuffles for the arg-min.
// einx_pair_metrics_pose measures the same quantities, and the share of matches near their epipolar lines,
// for a pair related by depth maps and a motion instead of a homography (core/geometry/depth.py:9-69, epipolar.py:59-80).
#include "einx_common.h"
#include "gt_project.h"

namespace {

struct MetArgs {
  const float *k0, *k1, *d0, *d1, *mk0, *mk1, *hom;
  const int32_t *n, *m, *nmatch;
  float* tw0;    // [B,cap0,2] keypoints0 warped by H (x,y)
  float* p1;     // [B,cap1,2] keypoints1 (x,y)
  uint8_t* keep0;
  uint8_t* keep1;
  int32_t* icnt;  // [B][16]: N1, N2, mma_good@t.. at 10..; the pose form (8p) also counts judged matches at 2 and EPI@t.. at 4..
  float* near0;   // [B,cap0,3] per kept keypoint of image 0: nearest distance, descriptor distance, angle
  float* near1;   // [B,cap1,3] same for image 1
  double* out;
  einx_metric_params p;
};

__device__ __forceinline__ void load_h(const float* hom, int b, float* h) {
  if (hom) {
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = hom[b * 9 + i];
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = (i % 4 == 0) ? 1.0f : 0.0f;
  }
}

// torch.mm(H, [x;y;1]) then division by the third row (core/metrics/util.py:17-33)
__device__ __forceinline__ void warp(const float* h, float x, float y, float* ox, float* oy) {
  const float a = fmaf(h[2], 1.0f, fmaf(h[1], y, h[0] * x));
  const float b = fmaf(h[5], 1.0f, fmaf(h[4], y, h[3] * x));
  const float c = fmaf(h[8], 1.0f, fmaf(h[7], y, h[6] * x));
  *ox = a / c;
  *oy = b / c;
}

__device__ __forceinline__ void inverse3(const float* h, float* inv) {
  const float c00 = h[4] * h[8] - h[5] * h[7], c01 = h[5] * h[6] - h[3] * h[8], c02 = h[3] * h[7] - h[4] * h[6];
  const float det = h[0] * c00 + h[1] * c01 + h[2] * c02;
  inv[0] = c00 / det;
  inv[1] = (h[2] * h[7] - h[1] * h[8]) / det;
  inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
  inv[3] = c01 / det;
  inv[4] = (h[0] * h[8] - h[2] * h[6]) / det;
  inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
  inv[6] = c02 / det;
  inv[7] = (h[1] * h[6] - h[0] * h[7]) / det;
  inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
}

constexpr int ICNT = 16;

__global__ void metric_prepare_kernel(const MetArgs a) {
  const int b = blockIdx.y;
  const int n = min(a.n[b], a.p.cap0), m = min(a.m[b], a.p.cap1);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  float h[9], hi[9];
  load_h(a.hom, b, h);
  const int xi = a.p.kp_yx ? 1 : 0, yi = a.p.kp_yx ? 0 : 1;
  if (t < n) {
    const float* k = a.k0 + ((size_t)b * a.p.cap0 + t) * 3;
    float wx, wy;
    warp(h, k[xi], k[yi], &wx, &wy);
    a.tw0[((size_t)b * a.p.cap0 + t) * 2] = wx;
    a.tw0[((size_t)b * a.p.cap0 + t) * 2 + 1] = wy;
    const bool keep = wx >= 0.0f && wx < (float)a.p.W1 && wy >= 0.0f && wy < (float)a.p.H1;  // inside img2_shape
    a.keep0[(size_t)b * a.p.cap0 + t] = keep;
    if (keep) atomicAdd(&a.icnt[b * ICNT + 0], 1);
  }
  if (t < m) {
    inverse3(h, hi);
    const float* k = a.k1 + ((size_t)b * a.p.cap1 + t) * 3;
    float wx, wy;
    warp(hi, k[xi], k[yi], &wx, &wy);
    a.p1[((size_t)b * a.p.cap1 + t) * 2] = k[xi];
    a.p1[((size_t)b * a.p.cap1 + t) * 2 + 1] = k[yi];
    const bool keep = wx >= 0.0f && wx < (float)a.p.W0 && wy >= 0.0f && wy < (float)a.p.H0;  // inside img1_shape
    a.keep1[(size_t)b * a.p.cap1 + t] = keep;
    if (keep) atomicAdd(&a.icnt[b * ICNT + 1], 1);
  }
}

// SIDE 0: for each kept warped keypoint of image 0, nearest kept keypoint of image 1 (torch.min(norm,1));
// SIDE 1: for each kept keypoint of image 1, nearest warped keypoint of image 0 (torch.min(norm,0)).
template <int SIDE>
__global__ __launch_bounds__(256) void metric_nearest_kernel(const MetArgs a) {
  const int b = blockIdx.y;
  const int n = min(a.n[b], a.p.cap0), m = min(a.m[b], a.p.cap1);
  const int self_n = SIDE == 0 ? n : m, other_n = SIDE == 0 ? m : n;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= self_n) return;
  const int cs = SIDE == 0 ? a.p.cap0 : a.p.cap1, co = SIDE == 0 ? a.p.cap1 : a.p.cap0;
  const uint8_t* keep_s = (SIDE == 0 ? a.keep0 : a.keep1) + (size_t)b * cs;
  const uint8_t* keep_o = (SIDE == 0 ? a.keep1 : a.keep0) + (size_t)b * co;
  if (!keep_s[i]) {
    if (lane == 0) ((SIDE == 0 ? a.near0 : a.near1) + ((size_t)b * cs + i) * 3)[0] = einx_u2f(0x7f800000u);
    return;
  }
  const float* ps = (SIDE == 0 ? a.tw0 : a.p1) + ((size_t)b * cs + i) * 2;
  const float* po = (SIDE == 0 ? a.p1 : a.tw0) + (size_t)b * co * 2;
  const float sx = ps[0], sy = ps[1];
  float best = einx_u2f(0x7f800000u);
  int bj = 0x7fffffff;
  // four candidates per lane and trip, their flags and coordinates requested together from clamped addresses (one guarded
  // load per iteration is a memory round trip each); evaluated in ascending j as before (strict <: the first minimum wins)
  for (int j0 = lane; j0 < other_n; j0 += 256) {
    uint8_t kk[4];
    float ox[4], oy[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int jc = min(j0 + 64 * u, other_n - 1);
      kk[u] = keep_o[jc];
      ox[u] = po[2 * jc];
      oy[u] = po[2 * jc + 1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + 64 * u;
      if (j >= other_n || !kk[u]) continue;
      // norm of (warped0 - p1): the difference is taken in that direction on both sides
      const float dx = SIDE == 0 ? sx - ox[u] : ox[u] - sx;
      const float dy = SIDE == 0 ? sy - oy[u] : oy[u] - sy;
      const float d = sqrtf(fmaf(dy, dy, dx * dx));
      if (d < best) {
        best = d;
        bj = j;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ob = __shfl_xor(best, off, 64);
    const int oj = __shfl_xor(bj, off, 64);
    if (ob < best || (ob == best && oj < bj)) {
      best = ob;
      bj = oj;
    }
  }
  float* nout = (SIDE == 0 ? a.near0 : a.near1) + ((size_t)b * cs + i) * 3;
  if (bj == 0x7fffffff) {
    if (lane == 0) nout[0] = einx_u2f(0x7f800000u);
    return;
  }
  // descriptor distance and angle of the pair (keypoints_metrics.py:233-247)
  const int D = a.p.D;
  const float* da = (SIDE == 0 ? a.d0 : a.d1) + ((size_t)b * cs + i) * D;
  const float* db = (SIDE == 0 ? a.d1 : a.d0) + ((size_t)b * co + bj) * D;
  // valid_desc1 always indexes image 0 and valid_desc2 image 1, whichever side drives the loop
  const float* v1 = SIDE == 0 ? da : db;
  const float* v2 = SIDE == 0 ? db : da;
  float sq = 0.0f, dot = 0.0f, n1 = 0.0f, n2 = 0.0f;
  for (int c0 = lane; c0 < D; c0 += 256) {  // same per-lane order c = lane, lane + 64, ...; four channel pairs in flight
    float a1[4], a2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int cc = min(c0 + 64 * u, D - 1);
      a1[u] = v1[cc];
      a2[u] = v2[cc];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (c0 + 64 * u >= D) continue;
      const float x1 = a1[u], x2 = a2[u];
      const float df = x1 - x2;
      sq = fmaf(df, df, sq);
      dot = fmaf(x1, x2, dot);
      n1 = fmaf(x1, x1, n1);
      n2 = fmaf(x2, x2, n2);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sq += __shfl_xor(sq, off, 64);
    dot += __shfl_xor(dot, off, 64);
    n1 += __shfl_xor(n1, off, 64);
    n2 += __shfl_xor(n2, off, 64);
  }
  if (lane == 0) {
    nout[0] = best;
    nout[1] = sqrtf(sq);
    nout[2] = einx_acosf(dot / (sqrtf(n1) * sqrtf(n2))) * 57.29577951308232f;
  }
}

__global__ void metric_mma_kernel(const MetArgs a) {
  const int b = blockIdx.y;
  const int M = min(a.nmatch[b], a.p.cap0);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M) return;
  float h[9];
  load_h(a.hom, b, h);
  const int xi = a.p.kp_yx ? 1 : 0, yi = a.p.kp_yx ? 0 : 1;
  const float* q0 = a.mk0 + ((size_t)b * a.p.cap0 + t) * a.p.cols;
  const float* q1 = a.mk1 + ((size_t)b * a.p.cap0 + t) * a.p.cols;
  float wx, wy;
  warp(h, q0[xi], q0[yi], &wx, &wy);
  const float dx = wx - q1[xi], dy = wy - q1[yi];
  const float d = sqrtf(dx * dx + dy * dy);
  for (int k = 0; k < a.p.n_mma; ++k)
    if (d <= a.p.mma_thr[k]) atomicAdd(&a.icnt[b * ICNT + 10 + k], 1);
}

// one workgroup per pair: fixed-order (deterministic) reduction of the per-keypoint records
__global__ __launch_bounds__(256) void metric_finalize_kernel(const MetArgs a) {
  __shared__ double sh[256];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = min(a.n[b], a.p.cap0), m = min(a.m[b], a.p.cap1), M = min(a.nmatch[b], a.p.cap0);
  const int nout = 1 + a.p.n_mma + 3 * a.p.n_vdd;
  double* o = a.out + (size_t)b * nout;
  const int32_t* ic = a.icnt + b * ICNT;
  auto block_sum = [&](double v) {
    sh[tid] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if (tid < off) sh[tid] += sh[tid + off];
      __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
  };
  if (tid == 0) {
    o[0] = (double)M / ((double)(n < m ? n : m) + 1e-8);  // MatchingRatio
    for (int k = 0; k < a.p.n_mma; ++k) o[1 + k] = M > 0 ? (double)((float)ic[10 + k] / (float)M) : 0.0;  // mask.float().mean()
  }
  const int N1 = ic[0], N2 = ic[1];
  for (int t = 0; t < a.p.n_vdd; ++t) {
    double c = 0.0, sd = 0.0, sa = 0.0;
    const float thr = a.p.vdd_thr[t];
    if (a.p.n_vdd > 0) {
      for (int i = tid; i < n; i += 256) {
        const float* r = a.near0 + ((size_t)b * a.p.cap0 + i) * 3;
        if (r[0] <= thr) {
          c += 1.0;
          sd += (double)r[1];
          sa += (double)r[2];
        }
      }
      for (int j = tid; j < m; j += 256) {
        const float* r = a.near1 + ((size_t)b * a.p.cap1 + j) * 3;
        if (r[0] <= thr) {
          c += 1.0;
          sd += (double)r[1];
          sa += (double)r[2];
        }
      }
    }
    c = block_sum(c);
    sd = block_sum(sd);
    sa = block_sum(sa);
    if (tid == 0) {
      double rep = 0.0, vd = 0.0, ang = 0.0;
      if (N1 != 0 && N2 != 0) {
        rep = (double)((float)c / (float)(N1 + N2));
        vd = sd / c;  // 0/0 -> NaN exactly like the reference when nothing is within t
        ang = sa / c;
      }
      if (a.p.rep_nan_if_empty && N1 + N2 == 0) rep = __longlong_as_double(0x7ff8000000000000LL);
      o[1 + a.p.n_mma + 3 * t + 0] = rep;
      o[1 + a.p.n_mma + 3 * t + 1] = vd;
      o[1 + a.p.n_mma + 3 * t + 2] = ang;
    }
  }
}

// einx_pair_metrics' workspace, and 256 bytes of slack.  icnt is zeroed by a memset that ends where near0 begins.
void carve(WsCarver& c, MetArgs& a, const einx_metric_params* p) {
  const size_t n0 = (size_t)p->B * p->cap0, n1 = (size_t)p->B * p->cap1;
  a.tw0 = c.take<float>(n0 * 2);
  a.p1 = c.take<float>(n1 * 2);
  a.keep0 = c.take<uint8_t>(n0);
  a.keep1 = c.take<uint8_t>(n1);
  a.icnt = c.take<int32_t>((size_t)p->B * ICNT);
  a.near0 = c.take<float>(n0 * 3);
  a.near1 = c.take<float>(n1 * 3);
  c.slack(256);
}

// ---- the same quantities under depth + pose instead of a homography: einx_pair_metrics_pose.  The keypoints of
// each view go through their own depth map and the pair's motion (8e stage A's sampler and projection, gt_project.h) into the other
// view; metric_nearest_kernel then runs unchanged on tw0 / p1 / keep0 / keep1.
struct PoseView {
  const float* depth;    // [B,H,W], null: no depth form
  const float* K;        // [B,9]
  const float* T;        // [B,16] this view -> the other, or null: the inverse of T_other
  const float* T_other;  // [B,16] the other view -> this one
  int H, W;              // of the depth map
};

struct PoseMetArgs {
  MetArgs m;       // what the nearest kernels read; m.p holds the shapes, m.hom is unused
  PoseView v[2];
  float occ_sq;    // occlusion_th^2, 0: no occlusion check
  int n_epi;
  float epi_thr[4];
};

constexpr int IC_JUDGED = 2, IC_EPI = 4;  // icnt slots beside N1, N2 (0, 1) and mma_good@t (10..)

// (x, y) of view s through its depth map and its motion into view o (contract 1 and 2 of 8p).  Returns valid && front, with the
// occlusion check on also && valid' && front' && consistent: the other map sampled at (u, v), back-projected with the inverse
// motion, must come back to within occlusion_th of (x, y).
__device__ __forceinline__ bool pose_project(const PoseView& s, const PoseView& o, int b, float x, float y, float occ_sq, float* u_out,
                                             float* v_out) {
  const float* Ks = s.K + b * 9;
  const float* Ko = o.K + b * 9;
  const float* T = s.T ? s.T + b * 16 : nullptr;
  const float* Tinv = o.T ? o.T + b * 16 : nullptr;
  const float* T_other = s.T ? nullptr : s.T_other + b * 16;  // a null motion is (R^T, -R^T t) of the other direction's
  const float* Tinv_other = o.T ? nullptr : o.T_other + b * 16;
  const float d = gt_sample_depth(s.depth + (size_t)b * s.H * s.W, s.H, s.W, x, y);
  const bool valid = d == d && d > 0.0f;
  float u, v;
  gt_project_point(x, y, d, Ks, Ko, T, T_other, &u, &v);
  const bool front = gt_point_qz(x, y, d, Ks, T, T_other) > 1e-4f;
  *u_out = u;
  *v_out = v;
  bool ok = valid && front;
  if (occ_sq > 0.0f) {
    const float d2 = gt_sample_depth(o.depth + (size_t)b * o.H * o.W, o.H, o.W, u, v);
    const bool valid2 = d2 == d2 && d2 > 0.0f;
    float bx, by;
    gt_project_point(u, v, d2, Ko, Ks, Tinv, Tinv_other, &bx, &by);
    const bool front2 = gt_point_qz(u, v, d2, Ko, Tinv, Tinv_other) > 1e-4f;
    const float dx = x - bx, dy = y - by;
    const bool consistent = dx * dx + dy * dy < occ_sq;  // NaN: false
    ok = ok && valid2 && front2 && consistent;
  }
  return ok;
}

// one thread per keypoint, both views in one launch (side 0's workgroups first): tw0 / keep0 / N1 and p1 / keep1 / N2
__global__ __launch_bounds__(256) void pose_prepare_kernel(const PoseMetArgs a) {
  const int b = blockIdx.y;
  const einx_metric_params& p = a.m.p;
  const int blocks0 = einx_cdiv(p.cap0, 256);
  const int side = (int)blockIdx.x >= blocks0 ? 1 : 0;
  const int i = ((int)blockIdx.x - (side ? blocks0 : 0)) * 256 + threadIdx.x;
  const int cnt = side ? min(a.m.m[b], p.cap1) : min(a.m.n[b], p.cap0);
  if (i >= cnt) return;
  const int cap = side ? p.cap1 : p.cap0;
  const int xi = p.kp_yx ? 1 : 0, yi = p.kp_yx ? 0 : 1;
  const size_t r = (size_t)b * cap + i;
  const float* k = (side ? a.m.k1 : a.m.k0) + r * 3;
  const float x = k[xi], y = k[yi];
  float u, v;
  const bool ok = pose_project(a.v[side], a.v[1 - side], b, x, y, a.occ_sq, &u, &v);
  // inside the OTHER image (keep_true_points of metrics.hip), not the camera's 2c - 1 of 8e
  const float Wo = (float)(side ? p.W0 : p.W1), Ho = (float)(side ? p.H0 : p.H1);
  const bool keep = ok && u >= 0.0f && u < Wo && v >= 0.0f && v < Ho;
  if (side == 0) {
    a.m.tw0[2 * r] = u;
    a.m.tw0[2 * r + 1] = v;
    a.m.keep0[r] = keep;
  } else {
    a.m.p1[2 * r] = x;
    a.m.p1[2 * r + 1] = y;
    a.m.keep1[r] = keep;
  }
  if (keep) atomicAdd(&a.m.icnt[b * ICNT + side], 1);
}

// one thread per match: the reprojection error of the judged matches (contract 4) and the symmetric epipolar distance (5)
__global__ __launch_bounds__(256) void pose_match_kernel(const PoseMetArgs a) {
  __shared__ double F[9];  // K1^-T [t]x R K0^-1 of the pair: formed once per workgroup, by thread 0
  const int b = blockIdx.y;
  const einx_metric_params& p = a.m.p;
  if (a.n_epi > 0 && threadIdx.x == 0) {
    const float* K0 = a.v[0].K + b * 9;
    const float* K1 = a.v[1].K + b * 9;
    const float* T = a.v[0].T + b * 16;
    double R[9], E[9], G[9];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * q + c] = (double)T[4 * q + c];
    const double tx = (double)T[3], ty = (double)T[7], tz = (double)T[11];
#pragma unroll
    for (int c = 0; c < 3; ++c) {  // [t]x R
      E[c] = ty * R[6 + c] - tz * R[3 + c];
      E[3 + c] = tz * R[c] - tx * R[6 + c];
      E[6 + c] = tx * R[3 + c] - ty * R[c];
    }
    // the closed-form inverse of a pinhole K: [[1/fx, 0, -cx/fx], [0, 1/fy, -cy/fy], [0, 0, 1]]
    const double a0 = 1.0 / (double)K0[0], b0 = 1.0 / (double)K0[4], c0 = -(double)K0[2] / (double)K0[0], d0 = -(double)K0[5] / (double)K0[4];
    const double a1 = 1.0 / (double)K1[0], b1 = 1.0 / (double)K1[4], c1 = -(double)K1[2] / (double)K1[0], d1 = -(double)K1[5] / (double)K1[4];
#pragma unroll
    for (int q = 0; q < 3; ++q) {  // E K0^-1
      G[3 * q] = E[3 * q] * a0;
      G[3 * q + 1] = E[3 * q + 1] * b0;
      G[3 * q + 2] = (E[3 * q] * c0 + E[3 * q + 1] * d0) + E[3 * q + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {  // K1^-T (E K0^-1)
      F[c] = a1 * G[c];
      F[3 + c] = b1 * G[3 + c];
      F[6 + c] = (c1 * G[c] + d1 * G[3 + c]) + G[6 + c];
    }
  }
  __syncthreads();
  const int M = min(a.m.nmatch[b], p.cap0);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M) return;
  const int xi = p.kp_yx ? 1 : 0, yi = p.kp_yx ? 0 : 1;
  const float* q0 = a.m.mk0 + ((size_t)b * p.cap0 + t) * p.cols;
  const float* q1 = a.m.mk1 + ((size_t)b * p.cap0 + t) * p.cols;
  const float x0 = q0[xi], y0 = q0[yi], x1 = q1[xi], y1 = q1[yi];
  if (a.v[0].depth) {
    float u, v;
    // judged: the depth map can say where the match's point went; being inside the image is not asked for
    if (pose_project(a.v[0], a.v[1], b, x0, y0, a.occ_sq, &u, &v)) {
      atomicAdd(&a.m.icnt[b * ICNT + IC_JUDGED], 1);
      const float dx = u - x1, dy = v - y1;
      const float d = sqrtf(dx * dx + dy * dy);
      for (int k = 0; k < p.n_mma; ++k)
        if (d <= p.mma_thr[k]) atomicAdd(&a.m.icnt[b * ICNT + 10 + k], 1);
    }
  }
  if (a.n_epi > 0) {
    // lines l1 = F p0 in view 1 and l0 = F^T p1 in view 0, e = |l1 . p1|; the mean of the two point-to-line distances
    const double X0 = (double)x0, Y0 = (double)y0, X1 = (double)x1, Y1 = (double)y1;
    const double l1x = (F[0] * X0 + F[1] * Y0) + F[2], l1y = (F[3] * X0 + F[4] * Y0) + F[5], l1z = (F[6] * X0 + F[7] * Y0) + F[8];
    const double l0x = (F[0] * X1 + F[3] * Y1) + F[6], l0y = (F[1] * X1 + F[4] * Y1) + F[7];
    const double e = fabs((l1x * X1 + l1y * Y1) + l1z);
    const double dist = 0.5 * (e / sqrt((l1x * l1x + l1y * l1y) + 1e-15) + e / sqrt((l0x * l0x + l0y * l0y) + 1e-15));
    for (int k = 0; k < a.n_epi; ++k)
      if (dist <= (double)a.epi_thr[k]) atomicAdd(&a.m.icnt[b * ICNT + IC_EPI + k], 1);
  }
}

// metric_finalize_kernel with 8p's rules: a quotient whose denominator is empty is NaN (nothing could be judged), not 0
__global__ __launch_bounds__(256) void pose_finalize_kernel(const PoseMetArgs a) {
  __shared__ double sh[256];
  const einx_metric_params& p = a.m.p;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = min(a.m.n[b], p.cap0), m = min(a.m.m[b], p.cap1), M = min(a.m.nmatch[b], p.cap0);
  const int nout = 1 + p.n_mma + 1 + 3 * p.n_vdd + a.n_epi;
  double* o = a.m.out + (size_t)b * nout;
  const int32_t* ic = a.m.icnt + b * ICNT;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const bool depth = a.v[0].depth != nullptr;
  auto block_sum = [&](double v) {
    sh[tid] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if (tid < off) sh[tid] += sh[tid + off];
      __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
  };
  if (tid == 0) {
    o[0] = (double)M / ((double)(n < m ? n : m) + 1e-8);  // MatchingRatio
    const int J = ic[IC_JUDGED];
    for (int k = 0; k < p.n_mma; ++k) o[1 + k] = depth && J > 0 ? (double)((float)ic[10 + k] / (float)J) : nan;
    o[1 + p.n_mma] = depth && M > 0 ? (double)((float)J / (float)M) : nan;  // judged_ratio
    for (int k = 0; k < a.n_epi; ++k) o[2 + p.n_mma + 3 * p.n_vdd + k] = M > 0 ? (double)((float)ic[IC_EPI + k] / (float)M) : nan;
  }
  const int N1 = ic[0], N2 = ic[1];
  const bool judged = depth && N1 != 0 && N2 != 0;  // uniform over the workgroup
  for (int t = 0; t < p.n_vdd; ++t) {
    double c = 0.0, sd = 0.0, sa = 0.0;
    const float thr = p.vdd_thr[t];
    if (judged) {
      for (int i = tid; i < n; i += 256) {
        const float* r = a.m.near0 + ((size_t)b * p.cap0 + i) * 3;
        if (r[0] <= thr) {
          c += 1.0;
          sd += (double)r[1];
          sa += (double)r[2];
        }
      }
      for (int j = tid; j < m; j += 256) {
        const float* r = a.m.near1 + ((size_t)b * p.cap1 + j) * 3;
        if (r[0] <= thr) {
          c += 1.0;
          sd += (double)r[1];
          sa += (double)r[2];
        }
      }
    }
    c = block_sum(c);
    sd = block_sum(sd);
    sa = block_sum(sa);
    if (tid == 0) {
      double* ot = o + 2 + p.n_mma + 3 * t;
      ot[0] = judged ? (double)((float)c / (float)(N1 + N2)) : nan;
      ot[1] = judged ? sd / c : nan;  // 0 / 0 -> NaN when nothing is within t, as the homography form
      ot[2] = judged ? sa / c : nan;
    }
  }
}

bool pose_params_ok(const einx_pose_metric_params* p) {
  return p && p->struct_size == sizeof(einx_pose_metric_params) && p->B > 0 && p->B <= 65535 && p->cap0 > 0 && p->cap1 > 0 && p->D > 0 &&
         p->H0 > 0 && p->W0 > 0 && p->H1 > 0 && p->W1 > 0 && (p->cols == 2 || p->cols == 3) && p->n_mma >= 0 && p->n_mma <= 4 &&
         p->n_vdd >= 0 && p->n_vdd <= 4 && p->n_epi >= 0 && p->n_epi <= 4;
}

// the shapes as the nearest kernels and `carve` read them
einx_metric_params pose_shapes(const einx_pose_metric_params* p) {
  einx_metric_params q = {};
  q.B = p->B, q.cap0 = p->cap0, q.cap1 = p->cap1, q.D = p->D, q.cols = p->cols;
  q.H0 = p->H0, q.W0 = p->W0, q.H1 = p->H1, q.W1 = p->W1;
  q.kp_yx = p->kp_yx;
  q.n_mma = p->n_mma, q.n_vdd = p->n_vdd;
  for (int k = 0; k < 4; ++k) q.mma_thr[k] = p->mma_thr[k], q.vdd_thr[k] = p->vdd_thr[k];
  return q;
}

}  // namespace

EINX_EXPORT size_t einx_metrics_ws_bytes(const einx_metric_params* p) {
  if (!p || p->B <= 0) return 0;
  WsCarver c{nullptr};
  MetArgs a;
  carve(c, a, p);
  return c.bytes;
}

EINX_EXPORT int einx_pair_metrics(const einx_metric_params* p, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                                  const int32_t* n, const int32_t* m, const float* mk0, const float* mk1, const int32_t* nmatch,
                                  const float* homography, void* ws, double* out, void* stream) {
  EINX_CHECK_ARG(p && kpts0 && kpts1 && desc0 && desc1 && n && m && mk0 && mk1 && nmatch && ws && out, "null pointer");
  EINX_CHECK_ARG(p->B > 0 && p->cap0 > 0 && p->cap1 > 0 && p->D > 0, "bad shape");
  EINX_CHECK_ARG(p->n_mma >= 0 && p->n_mma <= 4 && p->n_vdd >= 0 && p->n_vdd <= 4, "at most 4 thresholds per metric");
  EINX_CHECK_ARG(p->cols == 2 || p->cols == 3, "matched keypoints have 2 or 3 columns");
  hipStream_t s = (hipStream_t)stream;
  MetArgs a;
  a.k0 = kpts0;
  a.k1 = kpts1;
  a.d0 = desc0;
  a.d1 = desc1;
  a.mk0 = mk0;
  a.mk1 = mk1;
  a.hom = homography;
  a.n = n;
  a.m = m;
  a.nmatch = nmatch;
  a.p = *p;
  a.out = out;
  const size_t B = p->B;
  WsCarver c{(char*)ws};
  carve(c, a, p);
  if (hipMemsetAsync(a.icnt, 0, (char*)a.near0 - (char*)a.icnt, s) != hipSuccess) {
    einx_set_error("einx_pair_metrics: memset failed");
    return EINX_ERR_LAUNCH;
  }
  const int mx = p->cap0 > p->cap1 ? p->cap0 : p->cap1;
  hipLaunchKernelGGL(metric_prepare_kernel, dim3((unsigned)einx_cdiv(mx, 256), (unsigned)B), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  if (p->n_vdd > 0) {
    hipLaunchKernelGGL(metric_nearest_kernel<0>, dim3((unsigned)einx_cdiv(p->cap0, 4), (unsigned)B), dim3(256), 0, s, a);
    EINX_CHECK_LAUNCH();
    hipLaunchKernelGGL(metric_nearest_kernel<1>, dim3((unsigned)einx_cdiv(p->cap1, 4), (unsigned)B), dim3(256), 0, s, a);
    EINX_CHECK_LAUNCH();
  }
  if (p->n_mma > 0) {
    hipLaunchKernelGGL(metric_mma_kernel, dim3((unsigned)einx_cdiv(p->cap0, 256), (unsigned)B), dim3(256), 0, s, a);
    EINX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(metric_finalize_kernel, dim3((unsigned)B), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT size_t einx_pair_metrics_pose_ws_bytes(const einx_pose_metric_params* p) {
  if (!pose_params_ok(p)) return 0;
  const einx_metric_params q = pose_shapes(p);
  WsCarver c{nullptr};
  MetArgs a;
  carve(c, a, &q);  // einx_pair_metrics' regions: O(B (cap0 + cap1)), no N x M term
  return c.bytes;
}

EINX_EXPORT int einx_pair_metrics_pose(const einx_pose_metric_params* p, const float* kpts0, const float* kpts1, const float* desc0,
                                       const float* desc1, const int32_t* n, const int32_t* m, const float* mk0, const float* mk1,
                                       const int32_t* nmatch, const float* depth0, const float* depth1, const float* K0, const float* K1,
                                       const float* T_0to1, const float* T_1to0, void* ws, double* out, void* stream) {
  EINX_CHECK_ARG(p && p->struct_size == sizeof(einx_pose_metric_params), "bad struct_size");
  EINX_CHECK_ARG(p->n_mma >= 0 && p->n_mma <= 4 && p->n_vdd >= 0 && p->n_vdd <= 4 && p->n_epi >= 0 && p->n_epi <= 4,
                 "at most 4 thresholds per metric");
  EINX_CHECK_ARG(p->cols == 2 || p->cols == 3, "matched keypoints have 2 or 3 columns");
  EINX_CHECK_ARG(pose_params_ok(p), "bad shape (B, capacities, D and the image sizes must be positive, B <= 65535)");
  EINX_CHECK_ARG((depth0 != nullptr) == (depth1 != nullptr), "depth maps: both or neither");
  EINX_CHECK_ARG(!depth0 || (p->dH0 > 0 && p->dW0 > 0 && p->dH1 > 0 && p->dW1 > 0), "bad depth map size");
  EINX_CHECK_ARG(kpts0 && kpts1 && desc0 && desc1 && n && m && mk0 && mk1 && nmatch && K0 && K1 && T_0to1 && ws && out, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  PoseMetArgs a;
  a.m.k0 = kpts0;
  a.m.k1 = kpts1;
  a.m.d0 = desc0;
  a.m.d1 = desc1;
  a.m.mk0 = mk0;
  a.m.mk1 = mk1;
  a.m.hom = nullptr;
  a.m.n = n;
  a.m.m = m;
  a.m.nmatch = nmatch;
  a.m.p = pose_shapes(p);
  a.m.out = out;
  a.v[0] = PoseView{depth0, K0, T_0to1, T_1to0, p->dH0, p->dW0};
  a.v[1] = PoseView{depth1, K1, T_1to0, T_0to1, p->dH1, p->dW1};
  a.occ_sq = depth0 && p->occlusion_th > 0.0f ? p->occlusion_th * p->occlusion_th : 0.0f;
  a.n_epi = p->n_epi;
  for (int k = 0; k < 4; ++k) a.epi_thr[k] = p->epi_thr[k];
  const unsigned B = (unsigned)p->B;
  WsCarver c{(char*)ws};
  carve(c, a.m, &a.m.p);
  if (hipMemsetAsync(a.m.icnt, 0, (char*)a.m.near0 - (char*)a.m.icnt, s) != hipSuccess) {
    einx_set_error("einx_pair_metrics_pose: memset failed");
    return EINX_ERR_LAUNCH;
  }
  if (depth0 && p->n_vdd > 0) {
    {
      EINX_PROF("pose_prepare", stream);
      hipLaunchKernelGGL(pose_prepare_kernel, dim3((unsigned)(einx_cdiv(p->cap0, 256) + einx_cdiv(p->cap1, 256)), B), dim3(256), 0, s, a);
      EINX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(metric_nearest_kernel<0>, dim3((unsigned)einx_cdiv(p->cap0, 4), B), dim3(256), 0, s, a.m);
    EINX_CHECK_LAUNCH();
    hipLaunchKernelGGL(metric_nearest_kernel<1>, dim3((unsigned)einx_cdiv(p->cap1, 4), B), dim3(256), 0, s, a.m);
    EINX_CHECK_LAUNCH();
  }
  if (depth0 || p->n_epi > 0) {
    EINX_PROF("pose_match", stream);
    hipLaunchKernelGGL(pose_match_kernel, dim3((unsigned)einx_cdiv(p->cap0, 256), B), dim3(256), 0, s, a);
    EINX_CHECK_LAUNCH();
  }
  EINX_PROF("pose_finalize", stream);
  hipLaunchKernelGGL(pose_finalize_kernel, dim3(B), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
