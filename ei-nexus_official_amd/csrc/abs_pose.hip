// abs_pose.hip -- absolute (metric) pose of view 1 in view 0's frame for a batch of matched pairs on the device: the matches of
// view 0 are lifted through its depth map to 3-D points, RANSAC runs over Grunert's perspective-three-point solver, a
// Levenberg-Marquardt refit polishes (R, t) on the inliers' pixel residuals, and the epilogue measures the pose against the true
// one.  The contract (lift, guards, root finding, inlier rule, selection scan, damping rule, error rows) is DESIGN.md section 8u;
// tests/abs_pose_f64.py restates it in float64 numpy.  The reference has no such estimator: its different-time evaluation stops at
// the essential matrix (core/metrics/matching_metrics.py:362-518), a rotation and a translation direction.
//
// Launch sequence for B pairs with ragged nmatch, all on the caller's stream, no host synchronisation:
//   ap_lift_kernel       one workgroup per pair: depth per match, the usable matches compacted in order, X and view 1's pixel in double
//   in rounds of iterations (32, 32, 64, 128, ...), each pair skipping the iterations at or past its current scan bound:
//   ap_solve_kernel      one wave per (iteration, pair): three draws, P3P -> up to 4 (R, t) per sample
//   ap_score_kernel      one workgroup per (iteration, pair): reprojection inlier counts of the sample's models
//   ransac_select_kernel one lane per pair: the sequential scan with its shrinking iteration bound, resumed per round
//   ap_refine_kernel     one workgroup per pair: mask, LM refit on the inliers, errors
#include "einx_common.h"
#include "gt_project.h"
#include "ransac.h"

namespace {

constexpr int MAXS = 4;  // poses of one three-point sample
constexpr int MODEL = 12;  // R row-major, t
constexpr int LM_ITERS = 10;
constexpr double FLT_EPS = 1.1920928955078125e-07;
constexpr double COLLINEAR_TOL2 = 1e-12;  // (1e-6)^2: |(P2 - P1) x (P3 - P1)|^2 against |P2 - P1|^2 |P3 - P1|^2
constexpr double BEARING_TOL2 = 1e-12;    // (1e-6)^2: |f_i x f_j|^2 of unit bearings
constexpr double LEAD_TOL = 1e-12;        // a leading coefficient at or below this fraction of the largest lowers the degree

struct ApPoint {
  double X, Y, Z, x, y;  // the lifted point of view 0, the pixel of view 1
};

struct ApWs {
  ApPoint* pts;      // [B,cap] the usable matches, compacted
  int32_t* uidx;     // [B,cap] their match indices
  int32_t* nu;       // [B] their count
  uint8_t* inl;      // [B,cap] the RANSAC model's inlier flags over the usable list
  double* models;    // [B,iters,MAXS,MODEL]
  int32_t* nsol;     // [B,iters]
  int32_t* cnt;      // [B,iters,MAXS]
  RansacScan* scan;  // [B] best = iteration * MAXS + solution
};

// the workspace's regions; ws == nullptr: only their total size in *bytes
ApWs carve(const einx_abs_pose_params* p, void* ws, size_t* bytes = nullptr) {
  const size_t B = p->B, cap = p->cap, it = p->max_iters;
  WsCarver c{(char*)ws};
  ApWs w;
  w.pts = c.take<ApPoint>(B * cap);
  w.uidx = c.take<int32_t>(B * cap);
  w.nu = c.take<int32_t>(B);
  w.inl = c.take<uint8_t>(B * cap);
  w.models = c.take<double>(B * it * MAXS * MODEL);
  w.nsol = c.take<int32_t>(B * it);
  w.cnt = c.take<int32_t>(B * it * MAXS);
  w.scan = c.take<RansacScan>(B);
  if (bytes) *bytes = c.bytes;
  return w;
}

struct ApArgs {
  const float *mk0, *mk1;
  const int32_t* nmatch;
  const float* depth0;
  const float* d_in;
  const uint8_t* valid_in;
  const float *K0, *K1;
  const double* T;
  double *R_out, *t_out, *rows_out;
  uint8_t* mask_out;
  int32_t* status;
  ApWs w;
  einx_abs_pose_params p;
};

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 scale(V3 a, double s) { return V3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 unit(V3 a) { return scale(a, 1.0 / sqrt(dot(a, a))); }

// ---------------------------------------------------------------------------------------------- lift
__global__ __launch_bounds__(256) void ap_lift_kernel(const ApArgs a) {
  __shared__ int wcount[4];
  const int b = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int n = min(a.nmatch[b], a.p.cap);
  const size_t cap = a.p.cap;
  const int cols = a.p.cols, xi = a.p.kp_yx ? 1 : 0, yi = a.p.kp_yx ? 0 : 1;
  const float* K0 = a.K0 + b * 9;
  const double fx = (double)K0[0], fy = (double)K0[4], cx = (double)K0[2], cy = (double)K0[5];
  if (tid == 0) ransac_scan_init(a.w.scan[b], a.p.max_iters);
  int base = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + tid;
    bool ok = false;
    float x = 0.f, y = 0.f, d = 0.f;
    if (j < n) {
      const float* q0 = a.mk0 + ((size_t)b * cap + j) * cols;
      x = q0[xi];
      y = q0[yi];
      if (a.d_in) {
        d = a.d_in[b * cap + j];
        ok = a.valid_in[b * cap + j] != 0;
      } else {
        d = gt_sample_depth(a.depth0 + (size_t)b * a.p.H * a.p.W, a.p.H, a.p.W, x, y);
        ok = d == d && d > 0.0f;
      }
    }
    // stable compaction: a ballot inside each wave, the waves in order
    const unsigned long long m = __ballot(ok);
    __syncthreads();
    if (lane == 0) wcount[wv] = __popcll(m);
    __syncthreads();
    int off = base + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) off += wcount[w];
    if (ok) {
      const float* q1 = a.mk1 + ((size_t)b * cap + j) * cols;
      const double dd = (double)d;
      ApPoint pt;
      pt.X = dd * (((double)x - cx) / fx);
      pt.Y = dd * (((double)y - cy) / fy);
      pt.Z = dd;
      pt.x = (double)q1[xi];
      pt.y = (double)q1[yi];
      a.w.pts[b * cap + off] = pt;
      a.w.uidx[b * cap + off] = j;
    }
    base += wcount[0] + wcount[1] + wcount[2] + wcount[3];
  }
  if (tid == 0) a.w.nu[b] = base;
}

// ---------------------------------------------------------------------------------------------- P3P
struct P3pLds {
  double P[3][3];    // the 3-D points
  double f[3][3];    // the unit bearings
  double D[5][5];    // the quartic and its derivatives, coefficients ascending: D[k] = k-th derivative (degree n - k)
  double crit[6];    // sorted real roots of the level below, bracketed by -+bound
  double found[6];
  int has[6];
  int n, ncrit;
  double bound;
  double par[5];     // q = (a^2 - c^2) / b^2, cos alpha, cos beta, cos gamma, b^2
  double sol[MAXS][MODEL];
  int valid[MAXS];
};

__device__ __forceinline__ double horner(const double* c, int n, double x) {
  double v = c[n];
  for (int i = n - 1; i >= 0; --i) v = v * x + c[i];
  return v;
}

// Grunert's P3P for one sample, one 64-lane workgroup: L.P / L.f filled by the caller (a barrier after).  Writes the poses ordered
// by ascending v = s3 / s1 to out[MAXS][MODEL] and returns their count (uniform across the wave).
__device__ int p3p_solve(P3pLds& L, double* out) {
  const int lane = threadIdx.x;
  const V3 P1{L.P[0][0], L.P[0][1], L.P[0][2]}, P2{L.P[1][0], L.P[1][1], L.P[1][2]}, P3{L.P[2][0], L.P[2][1], L.P[2][2]};
  const V3 f1{L.f[0][0], L.f[0][1], L.f[0][2]}, f2{L.f[1][0], L.f[1][1], L.f[1][2]}, f3{L.f[2][0], L.f[2][1], L.f[2][2]};
  const V3 d21 = sub(P2, P1), d31 = sub(P3, P1), d23 = sub(P2, P3);
  const V3 cr = cross(d21, d31);
  const double a2 = dot(d23, d23), b2 = dot(d31, d31), c2 = dot(d21, d21);
  if (!(dot(cr, cr) > COLLINEAR_TOL2 * c2 * b2)) return 0;  // collinear or coincident points (NaN included)
  const V3 c12 = cross(f1, f2), c13 = cross(f1, f3), c23 = cross(f2, f3);
  if (!(dot(c12, c12) > BEARING_TOL2 && dot(c13, c13) > BEARING_TOL2 && dot(c23, c23) > BEARING_TOL2)) return 0;
  if (lane == 0) {
    const double ca = dot(f2, f3), cb = dot(f1, f3), cg = dot(f1, f2);
    const double q = (a2 - c2) / b2, p = (a2 + c2) / b2;
    double* A = L.D[0];
    A[4] = (q - 1.0) * (q - 1.0) - 4.0 * c2 / b2 * ca * ca;
    A[3] = 4.0 * (q * (1.0 - q) * cb - (1.0 - p) * ca * cg + 2.0 * c2 / b2 * ca * ca * cb);
    A[2] = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb * cb + 2.0 * (b2 - c2) / b2 * ca * ca - 4.0 * p * ca * cb * cg + 2.0 * (b2 - a2) / b2 * cg * cg);
    A[1] = 4.0 * (-q * (1.0 + q) * cb + 2.0 * a2 / b2 * cg * cg * cb - (1.0 - p) * ca * cg);
    A[0] = (1.0 + q) * (1.0 + q) - 4.0 * a2 / b2 * cg * cg;
    L.par[0] = q;
    L.par[1] = ca;
    L.par[2] = cb;
    L.par[3] = cg;
    L.par[4] = b2;
    double amax = 0.0;
    for (int i = 0; i < 5; ++i) amax = fmax(amax, fabs(A[i]));
    int n = 4;
    while (n > 0 && !(fabs(A[n]) > LEAD_TOL * amax)) --n;
    L.n = n;
    double cb_ = 0.0;
    for (int k = 1; k <= n; ++k) cb_ = fmax(cb_, pow(fabs(A[n - k] / A[n]), 1.0 / k));
    L.bound = 2.0 * cb_ + 1.0;  // Fujiwara: every root of p (and, by Gauss-Lucas, of its derivatives) lies inside
    for (int k = 1; k <= n; ++k)
      for (int i = 0; i <= n - k; ++i) L.D[k][i] = (i + 1) * L.D[k - 1][i + 1];
    L.ncrit = 0;
  }
  __syncthreads();
  // real roots level by level, from the linear derivative up to the quartic (as pose.hip finds the roots of its degree-10
  // polynomial): between two consecutive real roots of p^(k+1), p^(k) is monotonic and has a root there iff it changes sign
  const int n = L.n;
  if (n == 0 || !isfinite(L.bound)) return 0;
  for (int k = n - 1; k >= 0; --k) {
    const int m = L.ncrit;  // intervals: (-bound, c0], (c0, c1], ..., (c_{m-1}, bound]
    const double* c = L.D[k];
    const int dk = n - k;
    if (lane <= m) {
      double lo = lane == 0 ? -L.bound : L.crit[lane - 1];
      double hi = lane == m ? L.bound : L.crit[lane];
      const double flo = horner(c, dk, lo), fhi = horner(c, dk, hi);
      int got = 0;
      double r = hi;
      if (fhi == 0.0) {
        got = 1;
      } else if (flo != 0.0 && ((flo < 0.0) != (fhi < 0.0)) && lo < hi) {
        const bool neg_lo = flo < 0.0;
        for (int it = 0; it < 200; ++it) {
          const double mid = 0.5 * (lo + hi);
          if (!(mid > lo && mid < hi)) break;
          const double fm = horner(c, dk, mid);
          if (fm == 0.0) {
            lo = hi = mid;
            break;
          }
          if ((fm < 0.0) == neg_lo)
            lo = mid;
          else
            hi = mid;
        }
        r = 0.5 * (lo + hi);
        got = 1;
      }
      L.has[lane] = got;
      L.found[lane] = r;
    }
    __syncthreads();
    if (lane == 0) {
      int q = 0;
      for (int j = 0; j <= m; ++j)
        if (L.has[j] && (q == 0 || L.found[j] > L.crit[q - 1])) L.crit[q++] = L.found[j];
      L.ncrit = q;
    }
    __syncthreads();
  }
  const int nr = min(L.ncrit, MAXS);
  // Newton on the quartic from each root, then the roots closer than 1e-9 (relative, or absolute below 1) count once
  if (lane < nr) {
    const double* A = L.D[0];
    double v = L.crit[lane];
    for (int s = 0; s < 3; ++s) {
      const double pv = (((A[4] * v + A[3]) * v + A[2]) * v + A[1]) * v + A[0];
      const double dv = ((4.0 * A[4] * v + 3.0 * A[3]) * v + 2.0 * A[2]) * v + A[1];
      const double step = pv / dv;
      if (!isfinite(step)) break;
      v = v - step;
    }
    L.found[lane] = v;
  }
  __syncthreads();
  if (lane < nr) {
    const double v = L.found[lane];
    bool good = true;
    if (lane > 0) {
      // the restatement's walk: a root is dropped against the last root that was not dropped
      double last = L.found[0];
      for (int j = 1; j <= lane; ++j) {
        const double vj = L.found[j];
        const bool dup = fabs(vj - last) <= 1e-9 * fmax(1.0, fabs(vj));
        if (j == lane) good = !dup;
        if (!dup) last = vj;
      }
    }
    const double q = L.par[0], ca = L.par[1], cb = L.par[2], cg = L.par[3];
    const double u = ((q - 1.0) * v * v - 2.0 * q * cb * v + 1.0 + q) / (2.0 * (cg - v * ca));
    const double s1 = sqrt(L.par[4] / (1.0 + v * v - 2.0 * v * cb));
    const double s2 = u * s1, s3 = v * s1;
    good = good && isfinite(s1) && isfinite(s2) && isfinite(s3) && s1 > 0.0 && s2 > 0.0 && s3 > 0.0;
    // two orthonormal frames: e1 along 1 -> 2, e3 normal to the triangle, e2 = e3 x e1; R = F_Q F_P^T, t = Q1 - R P1
    const V3 Q1 = scale(f1, s1), Q2 = scale(f2, s2), Q3 = scale(f3, s3);
    const V3 p1 = unit(d21), p3 = unit(cross(p1, d31)), p2 = cross(p3, p1);
    const V3 g1 = unit(sub(Q2, Q1)), g3 = unit(cross(g1, sub(Q3, Q1))), g2 = cross(g3, g1);
    double R[9];
    R[0] = (g1.x * p1.x + g2.x * p2.x) + g3.x * p3.x;
    R[1] = (g1.x * p1.y + g2.x * p2.y) + g3.x * p3.y;
    R[2] = (g1.x * p1.z + g2.x * p2.z) + g3.x * p3.z;
    R[3] = (g1.y * p1.x + g2.y * p2.x) + g3.y * p3.x;
    R[4] = (g1.y * p1.y + g2.y * p2.y) + g3.y * p3.y;
    R[5] = (g1.y * p1.z + g2.y * p2.z) + g3.y * p3.z;
    R[6] = (g1.z * p1.x + g2.z * p2.x) + g3.z * p3.x;
    R[7] = (g1.z * p1.y + g2.z * p2.y) + g3.z * p3.y;
    R[8] = (g1.z * p1.z + g2.z * p2.z) + g3.z * p3.z;
    const double t0 = Q1.x - ((R[0] * P1.x + R[1] * P1.y) + R[2] * P1.z);
    const double t1 = Q1.y - ((R[3] * P1.x + R[4] * P1.y) + R[5] * P1.z);
    const double t2 = Q1.z - ((R[6] * P1.x + R[7] * P1.y) + R[8] * P1.z);
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      good = good && isfinite(R[e]);
      L.sol[lane][e] = R[e];
    }
    good = good && isfinite(t0) && isfinite(t1) && isfinite(t2);
    L.sol[lane][9] = t0;
    L.sol[lane][10] = t1;
    L.sol[lane][11] = t2;
    L.valid[lane] = good;
  }
  __syncthreads();
  int ns = 0;
  for (int k = 0; k < nr; ++k) {
    if (!L.valid[k]) continue;
    if (lane < MODEL) out[ns * MODEL + lane] = L.sol[k][lane];
    ++ns;
  }
  return ns;
}

// one round of iterations [it0, it0 + gridDim.x)
__global__ __launch_bounds__(64) void ap_solve_kernel(const ApArgs a, int it0) {
  __shared__ P3pLds L;
  const int it = it0 + blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = a.w.nu[b];
  const size_t h = (size_t)b * a.p.max_iters + it;
  int idx[3] = {0, 1, 2};
  // fewer than 4 usable matches: three points leave up to four poses and nothing to choose by
  if (n < 4 || !ransac_live(a.w.scan[b], it) || !ransac_draw<3>(a.p.seed, it, 0, n, idx)) {
    if (tid == 0) a.w.nsol[h] = 0;
    return;
  }
  if (tid < 3) {
    const int mine = tid == 0 ? idx[0] : tid == 1 ? idx[1] : idx[2];
    const ApPoint q = a.w.pts[(size_t)b * a.p.cap + mine];
    const float* K1 = a.K1 + b * 9;
    const double bx = (q.x - (double)K1[2]) / (double)K1[0], by = (q.y - (double)K1[5]) / (double)K1[4];
    const double nn = sqrt((bx * bx + by * by) + 1.0);
    L.P[tid][0] = q.X;
    L.P[tid][1] = q.Y;
    L.P[tid][2] = q.Z;
    L.f[tid][0] = bx / nn;
    L.f[tid][1] = by / nn;
    L.f[tid][2] = 1.0 / nn;
  }
  __syncthreads();
  const int ns = p3p_solve(L, a.w.models + h * MAXS * MODEL);
  if (tid == 0) a.w.nsol[h] = ns;
}

__global__ __launch_bounds__(64) void ap_p3p_kernel(const double* X, const double* f, double* R_out, double* t_out, int32_t* n_out) {
  __shared__ P3pLds L;
  __shared__ double sol[MAXS * MODEL];
  const int pb = blockIdx.x, tid = threadIdx.x;
  if (tid < 9) {
    L.P[tid / 3][tid % 3] = X[(size_t)pb * 9 + tid];
    L.f[tid / 3][tid % 3] = f[(size_t)pb * 9 + tid];
  }
  __syncthreads();
  const int ns = p3p_solve(L, sol);
  __syncthreads();
  if (tid < MAXS * MODEL) {
    const int k = tid / MODEL, e = tid % MODEL;
    const double v = k < ns ? sol[tid] : 0.0;
    if (e < 9)
      R_out[((size_t)pb * MAXS + k) * 9 + e] = v;
    else
      t_out[((size_t)pb * MAXS + k) * 3 + (e - 9)] = v;
  }
  if (tid == 0) n_out[pb] = ns;
}

// ---------------------------------------------------------------------------------------------- score
// inlier iff the point lies in front of view 1 and its projection falls within thr of the keypoint; a NaN is never an inlier
__device__ __forceinline__ bool ap_inlier(const double* m, const ApPoint q, double fx, double fy, double cx, double cy, double thr2) {
  const double Yx = ((m[0] * q.X + m[1] * q.Y) + m[2] * q.Z) + m[9];
  const double Yy = ((m[3] * q.X + m[4] * q.Y) + m[5] * q.Z) + m[10];
  const double Yz = ((m[6] * q.X + m[7] * q.Y) + m[8] * q.Z) + m[11];
  const double du = (fx * (Yx / Yz) + cx) - q.x, dv = (fy * (Yy / Yz) + cy) - q.y;
  return Yz > 0.0 && du * du + dv * dv <= thr2;
}

// inlier counts of one round's models: one point per thread, the sample's models read from LDS one at a time, every wave adds the
// popcount of its ballot to its own LDS counter
__global__ __launch_bounds__(256) void ap_score_kernel(const ApArgs a, int it0) {
  __shared__ double Ms[MAXS * MODEL];
  __shared__ int red[4][MAXS];
  const int it = it0 + blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = a.w.nu[b];
  if (n < 4 || !ransac_live(a.w.scan[b], it)) return;
  const size_t h = (size_t)b * a.p.max_iters + it;
  const int ns = a.w.nsol[h];
  if (ns == 0) return;
  if (tid < ns * MODEL) Ms[tid] = a.w.models[h * MAXS * MODEL + tid];
  if (tid < 4 * MAXS) red[tid / MAXS][tid % MAXS] = 0;
  __syncthreads();
  const float* K1 = a.K1 + b * 9;
  const double fx = (double)K1[0], fy = (double)K1[4], cx = (double)K1[2], cy = (double)K1[5];
  const double thr2 = a.p.thresh * a.p.thresh;
  const int wv = tid >> 6, lane = tid & 63;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + tid;
    const bool valid = j < n;
    const ApPoint q = a.w.pts[(size_t)b * a.p.cap + (valid ? j : 0)];
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
      const bool in = valid && ap_inlier(Ms + MODEL * s, q, fx, fy, cx, cy, thr2);
      const unsigned long long m = __ballot(in);
      if (lane == 0) red[wv][s] += __popcll(m);
    }
  }
  __syncthreads();
  if (tid < ns) a.w.cnt[h * MAXS + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// the models of one iteration for the selection scan
struct ApModels {
  const int32_t *nsol, *cnt;
  __device__ int count(size_t h) const { return nsol[h]; }
  __device__ int inliers(size_t h, int s) const { return cnt[h * MAXS + s]; }
};

// ---------------------------------------------------------------------------------------------- refit and errors
struct RefineLds {
  double red[4][28];
  double tot[28];
  double cur[28];   // J^T J (packed upper 6x6: 21), J^T r (6), |r|^2 of the accepted parameters
  double M[6][7];   // the damped system [A + lambda diag(A) | J^T r]
  double fac[6];
};

__device__ __forceinline__ int tri6(int j, int k) { return j * 6 - j * (j - 1) / 2 + (k - j); }  // packed upper triangle, j <= k

// J^T J (packed upper), J^T r and |r|^2 of the inliers' pixel residuals at (R, t) = m into L.tot: per thread over its points, a
// butterfly inside each wave, then the waves in order (a fixed order).  Parameters: R <- exp([w]x) R, t <- t + dt.  A point with
// Y_z <= 0 makes |r|^2 infinite.
__device__ void lm_pass(RefineLds& L, const ApPoint* pts, const uint8_t* inl, int n, const double* m, double fx, double fy, double cx,
                        double cy) {
  const int tid = threadIdx.x, wv = tid >> 6, nw = blockDim.x >> 6;
  double acc[28];
#pragma unroll
  for (int e = 0; e < 28; ++e) acc[e] = 0.0;
  for (int j = tid; j < n; j += blockDim.x) {
    if (!inl[j]) continue;
    const ApPoint q = pts[j];
    const double ax = (m[0] * q.X + m[1] * q.Y) + m[2] * q.Z;
    const double ay = (m[3] * q.X + m[4] * q.Y) + m[5] * q.Z;
    const double az = (m[6] * q.X + m[7] * q.Y) + m[8] * q.Z;
    const double Yx = ax + m[9], Yy = ay + m[10], Yz = az + m[11];
    if (!(Yz > 0.0)) {
      acc[27] += __longlong_as_double(0x7ff0000000000000LL);
      continue;
    }
    const double iz = 1.0 / Yz;
    const double r0 = (fx * (Yx / Yz) + cx) - q.x, r1 = (fy * (Yy / Yz) + cy) - q.y;
    // g = d(pixel) / dY; the row over w is a x g (g . (w x a) = w . (a x g)), the row over dt is g
    const double g0x = fx * iz, g0z = -fx * Yx * iz * iz;
    const double g1y = fy * iz, g1z = -fy * Yy * iz * iz;
    const double J0[6] = {ay * g0z, az * g0x - ax * g0z, -ay * g0x, g0x, 0.0, g0z};
    const double J1[6] = {ay * g1z - az * g1y, -ax * g1z, ax * g1y, 0.0, g1y, g1z};
    int e = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c, ++e) acc[e] += J0[r] * J0[c] + J1[r] * J1[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[21 + r] += J0[r] * r0 + J1[r] * r1;
    acc[27] += r0 * r0 + r1 * r1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 28; ++k) {
    double x = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if ((tid & 63) == 0) L.red[wv][k] = x;
  }
  __syncthreads();
  if (tid < 28) {
    double s = L.red[0][tid];
    for (int w = 1; w < nw; ++w) s += L.red[w][tid];
    L.tot[tid] = s;
  }
  __syncthreads();
}

// (exp([w]x) R, t + dt) into mn: exp = I + A [w]x + B [w]x^2, A = sin(th) / th, B = 2 (sin(th / 2) / th)^2; A = 1, B = 1/2 at th = 0
__device__ void apply_step(const double* m, const double* w, const double* dt, double* mn) {
  const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  double A = 1.0, Bc = 0.5;
  if (th > 0.0) {
    A = sin(th) / th;
    const double h = sin(0.5 * th) / th;
    Bc = 2.0 * h * h;
  }
  const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double E[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double w2 = (W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j]) + W[3 * i + 2] * W[6 + j];
      E[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * W[3 * i + j]) + Bc * w2;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) mn[3 * i + j] = (E[3 * i] * m[j] + E[3 * i + 1] * m[3 + j]) + E[3 * i + 2] * m[6 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i) mn[9 + i] = m[9 + i] + dt[i];
}

__global__ __launch_bounds__(256) void ap_refine_kernel(const ApArgs a) {
  __shared__ RefineLds L;
  __shared__ int red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(a.nmatch[b], a.p.cap);
  const int nu = a.w.nu[b];
  const size_t cap = a.p.cap;
  uint8_t* mout = a.mask_out + b * cap;
  uint8_t* inl = a.w.inl + b * cap;
  const ApPoint* pts = a.w.pts + b * cap;
  const int32_t* uidx = a.w.uidx + b * cap;
  for (size_t j = tid; j < cap; j += 256) mout[j] = 0;
  __syncthreads();
  int status = nu < 4 ? -1 : -2, ninl = 0;
  double m[MODEL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int bi = nu >= 4 ? a.w.scan[b].best : -1;
  if (bi >= 0) {  // uniform across the workgroup
    const double* mb = a.w.models + (((size_t)b * a.p.max_iters + (bi >> 2)) * MAXS + (bi & 3)) * MODEL;
#pragma unroll
    for (int e = 0; e < MODEL; ++e) m[e] = mb[e];
    const float* K1 = a.K1 + b * 9;
    const double fx = (double)K1[0], fy = (double)K1[4], cx = (double)K1[2], cy = (double)K1[5];
    const double thr2 = a.p.thresh * a.p.thresh;
    int c = 0;
    for (int j0 = 0; j0 < nu; j0 += 256) {  // thread tid owns the usable matches tid, tid + 256, ...
      const int j = j0 + tid;
      const bool in = j < nu && ap_inlier(m, pts[j < nu ? j : 0], fx, fy, cx, cy, thr2);
      if (j < nu) {
        inl[j] = in;
        mout[uidx[j]] = in;
      }
      c += __popcll(__ballot(in));
    }
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    ninl = red[0] + red[1] + red[2] + red[3];
    status = bi;
    if (a.p.refine) {
      lm_pass(L, pts, inl, nu, m, fx, fy, cx, cy);
      if (tid < 28) L.cur[tid] = L.tot[tid];
      __syncthreads();
      double lambda = 1e-3;
      for (int iter = 0; iter < LM_ITERS; ++iter) {
        if (tid < 42) {
          const int r = tid / 7, k = tid % 7;
          L.M[r][k] = k == 6 ? L.cur[21 + r] : L.cur[r <= k ? tri6(r, k) : tri6(k, r)] + (r == k ? lambda * L.cur[tri6(r, r)] : 0.0);
        }
        __syncthreads();
        if (!gauss_jordan<6, 7>(L.M, L.fac, 0.0)) break;
        double d[6], mn[MODEL], dmax = 0.0;
        bool fin = true;
#pragma unroll
        for (int e = 0; e < 6; ++e) {
          d[e] = -L.M[e][6];
          fin &= isfinite(d[e]);
          dmax = fmax(dmax, fabs(d[e]));
        }
        if (!fin) break;
        apply_step(m, d, d + 3, mn);
        lm_pass(L, pts, inl, nu, mn, fx, fy, cx, cy);
        const double S = L.cur[27], Sd = L.tot[27];
        __syncthreads();
        if (Sd < S) {
#pragma unroll
          for (int e = 0; e < MODEL; ++e) m[e] = mn[e];
          if (tid < 28) L.cur[tid] = L.tot[tid];
          lambda = lambda / 10.0;
        } else {
          lambda = lambda * 10.0;
        }
        __syncthreads();
        if (dmax < FLT_EPS) break;
      }
    }
  }
  if (tid != 0) return;
  a.status[b] = status;
  double* Ro = a.R_out + (size_t)b * 9;
  double* to = a.t_out + (size_t)b * 3;
  const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
  double* rows = a.rows_out ? a.rows_out + (size_t)b * 5 : nullptr;
  if (rows) rows[4] = (double)nu / (double)n;  // NaN for a pair without matches
  if (status < 0) {
    for (int i = 0; i < 9; ++i) Ro[i] = 0.0;
    for (int i = 0; i < 3; ++i) to[i] = 0.0;
    if (rows) {
      rows[0] = rows[1] = rows[2] = inf;
      rows[3] = 0.0;
    }
    return;
  }
  for (int i = 0; i < 9; ++i) Ro[i] = m[i];
  for (int i = 0; i < 3; ++i) to[i] = m[9 + i];
  if (!rows) return;
  rows[3] = (double)ninl / (double)nu;
  if (!a.T) {
    rows[0] = rows[1] = rows[2] = nan;
    return;
  }
  // pose.hip's error rules (8b), with the metric distance between them
  const double* T = a.T + (size_t)b * 16;
  const double* R = m;
  const double* t = m + 9;
  const double tg0 = T[3], tg1 = T[7], tg2 = T[11];
  const double ngt = sqrt(tg0 * tg0 + tg1 * tg1 + tg2 * tg2);
  const double nrm = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) * ngt;
  const double rad2deg = 57.29577951308232;
  double c = (t[0] * tg0 + t[1] * tg1 + t[2] * tg2) / nrm;
  if (!isnan(c)) c = fmin(fmax(c, -1.0), 1.0);
  double t_ang = acos(c) * rad2deg;
  t_ang = isnan(t_ang) ? t_ang : fmin(t_ang, 180.0 - t_ang);
  if (!isfinite(ngt)) t_ang = 0.0;
  double tr = 0.0;
  for (int i = 0; i < 3; ++i) {
    double d = 0.0;
    for (int k = 0; k < 3; ++k) d += R[3 * k + i] * T[4 * k + i];
    tr += d;
  }
  double cs = (tr - 1.0) / 2.0;
  if (!isnan(cs)) cs = fmin(fmax(cs, -1.0), 1.0);
  const double e0 = t[0] - tg0, e1 = t[1] - tg1, e2 = t[2] - tg2;
  rows[0] = fabs(acos(cs)) * rad2deg;
  rows[1] = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
  rows[2] = t_ang;
}

bool shape_ok(const einx_abs_pose_params* p) {
  return p && p->struct_size == sizeof(einx_abs_pose_params) && p->B > 0 && p->cap > 0 && (p->cols == 2 || p->cols == 3) &&
         p->max_iters > 0 && p->max_iters <= 65535;
}

}  // namespace

EINX_EXPORT size_t einx_absolute_pose_ws_bytes(const einx_abs_pose_params* p) {
  if (!shape_ok(p)) return 0;
  size_t bytes = 0;
  carve(p, nullptr, &bytes);
  return bytes;
}

EINX_EXPORT int einx_absolute_pose(const einx_abs_pose_params* p, const float* mk0, const float* mk1, const int32_t* nmatch,
                                   const float* depth0, const float* d_in, const uint8_t* valid_in, const float* K0, const float* K1,
                                   const double* T_0to1, void* ws, double* R_out, double* t_out, uint8_t* mask_out, int32_t* status,
                                   double* rows_out, void* stream) {
  EINX_CHECK_ARG(p && p->struct_size == sizeof(einx_abs_pose_params), "einx_abs_pose_params.struct_size mismatch");
  EINX_CHECK_ARG(mk0 && mk1 && nmatch && K0 && K1 && ws && R_out && t_out && mask_out && status, "null pointer");
  EINX_CHECK_ARG(p->B > 0 && p->cap > 0 && (p->cols == 2 || p->cols == 3), "bad shape");
  EINX_CHECK_ARG(p->max_iters > 0 && p->max_iters <= 65535, "max_iters out of range");
  EINX_CHECK_ARG(p->kp_yx == 0 || p->kp_yx == 1, "kp_yx is 0 or 1");
  EINX_CHECK_ARG((d_in != nullptr) == (valid_in != nullptr), "d_in and valid_in come together");
  EINX_CHECK_ARG((depth0 != nullptr) != (d_in != nullptr), "exactly one of depth0 and (d_in, valid_in)");
  EINX_CHECK_ARG(!depth0 || (p->H > 0 && p->W > 0), "depth0 needs H > 0 and W > 0");
  hipStream_t s = (hipStream_t)stream;
  ApArgs a;
  a.mk0 = mk0;
  a.mk1 = mk1;
  a.nmatch = nmatch;
  a.depth0 = depth0;
  a.d_in = d_in;
  a.valid_in = valid_in;
  a.K0 = K0;
  a.K1 = K1;
  a.T = T_0to1;
  a.R_out = R_out;
  a.t_out = t_out;
  a.rows_out = rows_out;
  a.mask_out = mask_out;
  a.status = status;
  a.p = *p;
  a.w = carve(p, ws);
  const unsigned B = (unsigned)p->B;
  hipLaunchKernelGGL(ap_lift_kernel, dim3(B), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  // a failed launch ends the rounds and stays pending for the check below; the scan runs over the usable counts
  ransac_rounds(p->max_iters, [&](int it0, int it1) {
    hipLaunchKernelGGL(ap_solve_kernel, dim3((unsigned)(it1 - it0), B), dim3(64), 0, s, a, it0);
    if (hipPeekAtLastError() != hipSuccess) return false;
    hipLaunchKernelGGL(ap_score_kernel, dim3((unsigned)(it1 - it0), B), dim3(256), 0, s, a, it0);
    if (hipPeekAtLastError() != hipSuccess) return false;
    hipLaunchKernelGGL((ransac_select_kernel<3, MAXS, ApModels>), dim3((unsigned)einx_cdiv(p->B, 64)), dim3(64), 0, s, a.w.scan, a.w.nu,
                       p->B, p->cap, p->max_iters, p->conf, it0, it1, ApModels{a.w.nsol, a.w.cnt});
    return hipPeekAtLastError() == hipSuccess;
  });
  EINX_CHECK_LAUNCH();
  hipLaunchKernelGGL(ap_refine_kernel, dim3(B), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_p3p(const double* X, const double* f, int n, double* R_out, double* t_out, int32_t* n_solutions, void* stream) {
  EINX_CHECK_ARG(X && f && R_out && t_out && n_solutions, "null pointer");
  EINX_CHECK_ARG(n > 0, "n > 0");
  hipLaunchKernelGGL(ap_p3p_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, X, f, R_out, t_out, n_solutions);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
