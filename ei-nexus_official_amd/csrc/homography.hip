// homography.hip -- homography of a batch of matched pairs on the device: RANSAC over the normalised 4-point DLT, a DLT refit on the
// inliers, a Levenberg-Marquardt polish, and the corner-error epilogue of HomographyEstimation.update_one.  The contract (generator,
// checkSubset, inlier rule, selection scan, damping rule) is DESIGN.md section 8c; tests/homography_f64.py restates it in float64
// numpy.
//
// Replaces (reference file:line): core/metrics/matching_metrics.py:188-345 (cv2.findHomography(RANSAC) + the corner distances), which
// ran on the host after a device-to-host copy.
//
// Launch sequence for B pairs with ragged nmatch, all on the caller's stream, no host synchronisation:
//   hg_init_kernel    the selection scan's state
//   in rounds of iterations (32, 32, 64, 128, ...), each pair skipping the iterations at or past its current scan bound:
//   hg_solve_kernel   one wave per (iteration, pair): four draws that pass checkSubset, the DLT -> one H per sample
//   hg_score_kernel   one workgroup per (iteration, pair): reprojection inlier count of the sample's H
//   ransac_select_kernel  one lane per pair: OpenCV's sequential scan with its shrinking iteration bound, resumed per round
//   hg_refine_kernel  one workgroup per pair: mask, DLT refit on the inliers, LM polish, corner errors
#include "einx_common.h"
#include "ransac.h"

namespace {

constexpr int ATTEMPTS = 16;  // samples drawn for one iteration until one passes checkSubset
constexpr int SWEEPS = 12;    // cyclic Jacobi sweeps over the 9x9
constexpr int LM_ITERS = 10;
constexpr double DBL_EPS = 2.220446049250313e-16;
constexpr double FLT_EPS = 1.1920928955078125e-07;

struct HgWs {
  double* H;         // [B,iters,9]
  int32_t* cnt;      // [B,iters] inlier count of the iteration's H, -1: no model
  RansacScan* scan;  // [B] best = iteration
};

// the workspace's regions; ws == nullptr: only their total size in *bytes
HgWs carve(const einx_homography_params* p, void* ws, size_t* bytes = nullptr) {
  const size_t B = p->B, it = p->max_iters;
  WsCarver c{(char*)ws};
  HgWs w;
  w.H = c.take<double>(B * it * 9);
  w.cnt = c.take<int32_t>(B * it);
  w.scan = c.take<RansacScan>(B);
  if (bytes) *bytes = c.bytes;
  return w;
}

struct HgArgs {
  const float *mk0, *mk1;
  const int32_t* nmatch;
  const int32_t* img_shape;
  const float* H_true;
  double *H_out, *rows_out;
  uint8_t* mask_out;
  int32_t* status;
  HgWs w;
  einx_homography_params p;
};

struct Pt {
  float X, Y, x, y;  // (x, y) of the first image, of the second image
};

__device__ __forceinline__ Pt load_pt(const HgArgs& a, int b, int j) {
  const int cols = a.p.cols, xi = a.p.kp_yx ? 1 : 0, yi = a.p.kp_yx ? 0 : 1;
  const float* q0 = a.mk0 + ((size_t)b * a.p.cap + j) * cols;
  const float* q1 = a.mk1 + ((size_t)b * a.p.cap + j) * cols;
  return Pt{q0[xi], q0[yi], q1[xi], q1[yi]};
}

// haveCollinearPoints' test for the triplet (a, b, c), a < b < c, based at c
__device__ __forceinline__ bool collinear3(double ax, double ay, double bx, double by, double cx, double cy) {
  const double d1x = bx - cx, d1y = by - cy, d2x = ax - cx, d2y = ay - cy;
  return fabs(d2x * d1y - d1x * d2y) <= FLT_EPS * (fabs(d1x) + fabs(d1y) + fabs(d2x) + fabs(d2y));
}

__device__ __forceinline__ double det3(double x0, double y0, double x1, double y1, double x2, double y2) {
  return x0 * (y1 - y2) - y0 * (x1 - x2) + (x1 * y2 - x2 * y1);
}

// HomographyEstimatorCallback::checkSubset for four points: no collinear triplet in either image, and every triplet keeps its
// orientation (OpenCV also lets a sample through whose four triplets all flip, a reflection: 8c does not)
__device__ __forceinline__ bool check_subset(const Pt* q) {
  constexpr int TT[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
  bool col = false;
  int negative = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const Pt &a = q[TT[t][0]], &b = q[TT[t][1]], &c = q[TT[t][2]];
    col |= collinear3(a.X, a.Y, b.X, b.Y, c.X, c.Y) || collinear3(a.x, a.y, b.x, b.y, c.x, c.y);
    negative += det3(a.X, a.Y, b.X, b.Y, c.X, c.Y) * det3(a.x, a.y, b.x, b.y, c.x, c.y) < 0.0;
  }
  return !col && negative == 0;
}

struct DltLds {
  double red[4][45];
  double tot[45];
  double S[9][9];
  double V[9][9];
};

// sum of v[k] over the workgroup into L.tot[k]: a butterfly inside each wave, then the waves in order (a fixed order: the result
// does not depend on where the pair sits in the batch)
template <int K>
__device__ __forceinline__ void block_sum(DltLds& L, double (&v)[K]) {
  const int tid = threadIdx.x, wv = tid >> 6, nw = blockDim.x >> 6;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double x = v[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if ((tid & 63) == 0) L.red[wv][k] = x;
  }
  __syncthreads();
  if (tid < K) {
    double s = L.red[0][tid];
    for (int w = 1; w < nw; ++w) s += L.red[w][tid];
    L.tot[tid] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ int tri(int j, int k) { return j * 9 - j * (j - 1) / 2 + (k - j); }  // packed upper triangle of a 9x9, j <= k

// OpenCV's HomographyEstimatorCallback::runKernel over the points j of [0, n) that `get(j, pt)` keeps: per image the centroid and
// the mean absolute deviation per axis, LtL from the two rows per point, its smallest eigenvector by cyclic Jacobi, de-normalised
// and scaled to H[2,2] = 1.  Every thread of the workgroup calls it and gets H; false: no model.
template <class F>
__device__ bool dlt_fit(DltLds& L, int n, F get, double* H) {
  const int tid = threadIdx.x, nt = blockDim.x;
  double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < n; j += nt) {
    Pt q;
    if (!get(j, q)) continue;
    s5[0] += 1.0;
    s5[1] += (double)q.X;
    s5[2] += (double)q.Y;
    s5[3] += (double)q.x;
    s5[4] += (double)q.y;
  }
  block_sum<5>(L, s5);
  const double cnt = L.tot[0];
  if (!(cnt >= 4.0)) return false;
  const double cX = L.tot[1] / cnt, cY = L.tot[2] / cnt, cx = L.tot[3] / cnt, cy = L.tot[4] / cnt;
  double s4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < n; j += nt) {
    Pt q;
    if (!get(j, q)) continue;
    s4[0] += fabs((double)q.X - cX);
    s4[1] += fabs((double)q.Y - cY);
    s4[2] += fabs((double)q.x - cx);
    s4[3] += fabs((double)q.y - cy);
  }
  block_sum<4>(L, s4);
  if (!(fabs(L.tot[0]) >= DBL_EPS && fabs(L.tot[1]) >= DBL_EPS && fabs(L.tot[2]) >= DBL_EPS && fabs(L.tot[3]) >= DBL_EPS)) return false;
  const double sX = cnt / L.tot[0], sY = cnt / L.tot[1], sx = cnt / L.tot[2], sy = cnt / L.tot[3];
  double acc[45];
#pragma unroll
  for (int e = 0; e < 45; ++e) acc[e] = 0.0;
  for (int j = tid; j < n; j += nt) {
    Pt q;
    if (!get(j, q)) continue;
    const double X = ((double)q.X - cX) * sX, Y = ((double)q.Y - cY) * sY, x = ((double)q.x - cx) * sx, y = ((double)q.y - cy) * sy;
    const double Lx[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x};
    const double Ly[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y};
    int e = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c, ++e) acc[e] += Lx[r] * Lx[c] + Ly[r] * Ly[c];
  }
  block_sum<45>(L, acc);
  for (int e = tid; e < 81; e += nt) {
    const int r = e / 9, c = e % 9;
    L.S[r][c] = L.tot[r <= c ? tri(r, c) : tri(c, r)];
    L.V[r][c] = r == c ? 1.0 : 0.0;
  }
  __syncthreads();
  // cyclic Jacobi, the classical one-rotation update: lanes 0..8 hold the rows of S, lanes 9..17 the rows of V.  All working
  // lanes sit in wave 0, which reads (p,p), (q,q), (p,q) before any of its lanes writes them.
  for (int sweep = 0; sweep < SWEEPS; ++sweep)
    for (int p = 0; p < 8; ++p)
      for (int q = p + 1; q < 9; ++q) {
        const double apq = L.S[p][q], app = L.S[p][p], aqq = L.S[q][q];
        if (fabs(apq) > 1e-22 * (fabs(app) + fabs(aqq))) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          if (tid < 9) {
            const int k = tid;
            if (k == p) {
              L.S[p][p] = app - t * apq;
              L.S[q][q] = aqq + t * apq;
              L.S[p][q] = 0.0;
              L.S[q][p] = 0.0;
            } else if (k != q) {
              const double skp = L.S[k][p], skq = L.S[k][q];
              const double n1 = c * skp - s * skq, n2 = s * skp + c * skq;
              L.S[k][p] = n1;
              L.S[p][k] = n1;
              L.S[k][q] = n2;
              L.S[q][k] = n2;
            }
          } else if (tid < 18) {
            const int k = tid - 9;
            const double vkp = L.V[k][p], vkq = L.V[k][q];
            L.V[k][p] = c * vkp - s * vkq;
            L.V[k][q] = s * vkp + c * vkq;
          }
        }
        __syncthreads();
      }
  int m = 0;
  double ev = L.S[0][0];
  for (int i = 1; i < 9; ++i)
    if (L.S[i][i] < ev) {
      ev = L.S[i][i];
      m = i;
    }
  double h[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) h[i] = L.V[i][m];
  // invHnorm * H0 * Hnorm2
  double g[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    g[c] = h[c] / sx + cx * h[6 + c];
    g[3 + c] = h[3 + c] / sy + cy * h[6 + c];
    g[6 + c] = h[6 + c];
  }
  bool ok = true;
  double big = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    H[3 * r] = g[3 * r] * sX;
    H[3 * r + 1] = g[3 * r + 1] * sY;
    H[3 * r + 2] = (g[3 * r + 2] - g[3 * r] * (cX * sX)) - g[3 * r + 1] * (cY * sY);
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    ok &= isfinite(H[i]);
    big = fmax(big, fabs(H[i]));
  }
  if (!ok || !(fabs(H[8]) > 1e-12 * big)) return false;
  const double inv = 1.0 / H[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) H[i] = H[i] * inv;
  H[8] = 1.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) ok &= isfinite(H[i]);
  return ok;
}

__global__ void hg_init_kernel(const HgArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.p.B) return;
  ransac_scan_init(a.w.scan[b], a.p.max_iters);
}

// one round of iterations [it0, it0 + gridDim.x)
__global__ __launch_bounds__(64) void hg_solve_kernel(const HgArgs a, int it0) {
  __shared__ DltLds L;
  const int it = it0 + blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = min(a.nmatch[b], a.p.cap);
  const size_t h = (size_t)b * a.p.max_iters + it;
  // n == 4: OpenCV solves the one sample directly (iteration 0 holds it); n < 4: no homography
  if (n < 4 || (n == 4 && it > 0) || !ransac_live(a.w.scan[b], it)) {
    if (tid == 0) a.w.cnt[h] = -1;
    return;
  }
  int idx[4] = {0, 1, 2, 3};
  bool ok = n == 4;
  for (int att = 0; att < ATTEMPTS && !ok; ++att) {
    if (!ransac_draw<4>(a.p.seed, it, att, n, idx)) continue;
    Pt q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = load_pt(a, b, idx[e]);
    ok = check_subset(q);
  }
  if (!ok) {
    if (tid == 0) a.w.cnt[h] = -1;
    return;
  }
  const int i0 = idx[0], i1 = idx[1], i2 = idx[2], i3 = idx[3];
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  ok = dlt_fit(L, 4, [&](int j, Pt& q) {
    q = load_pt(a, b, j == 0 ? i0 : j == 1 ? i1 : j == 2 ? i2 : i3);
    return true;
  }, H);
  if (tid < 9) {
    double v = H[0];
#pragma unroll
    for (int e = 1; e < 9; ++e) v = tid == e ? H[e] : v;
    a.w.H[h * 9 + tid] = ok ? v : 0.0;
  }
  if (tid == 0) a.w.cnt[h] = ok ? 4 : -1;
}

// OpenCV HomographyEstimatorCallback::computeError: H rounded to float, float arithmetic
__device__ __forceinline__ float reproj_err(const float* Hf, const Pt q) {
  const float ww = 1.f / ((Hf[6] * q.X + Hf[7] * q.Y) + 1.f);
  const float dx = ((Hf[0] * q.X + Hf[1] * q.Y) + Hf[2]) * ww - q.x;
  const float dy = ((Hf[3] * q.X + Hf[4] * q.Y) + Hf[5]) * ww - q.y;
  return dx * dx + dy * dy;
}

// inlier count of one iteration's H: one point per thread, every wave adds the popcount of its ballot
__global__ __launch_bounds__(256) void hg_score_kernel(const HgArgs a, int it0) {
  __shared__ int red[4];
  const int it = it0 + blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = min(a.nmatch[b], a.p.cap);
  if (n <= 4 || !ransac_live(a.w.scan[b], it)) return;
  const size_t h = (size_t)b * a.p.max_iters + it;
  if (a.w.cnt[h] < 0) return;
  float Hf[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) Hf[e] = (float)a.w.H[h * 9 + e];
  const float thr2 = (float)(a.p.thresh * a.p.thresh);
  int c = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + tid;
    const bool valid = j < n;
    const Pt q = load_pt(a, b, valid ? j : 0);
    const bool in = valid && reproj_err(Hf, q) <= thr2;  // a NaN error is never an inlier
    c += __popcll(__ballot(in));
  }
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) a.w.cnt[h] = red[0] + red[1] + red[2] + red[3];
}

// the one model of an iteration for the selection scan (an iteration without a model counts -1 inliers)
struct HgModels {
  const int32_t* cnt;
  __device__ int count(size_t) const { return 1; }
  __device__ int inliers(size_t h, int) const { return cnt[h]; }
};

struct RefineLds {
  DltLds D;
  double cur[45];   // A (packed upper 8x8: 36), v (8), S of the accepted parameters
  double M[8][9];   // the damped system [A + lambda diag(A) | v]
  double fac[8];
};

__device__ __forceinline__ int tri8(int j, int k) { return j * 8 - j * (j - 1) / 2 + (k - j); }

// HomographyRefineCallback at h (H[2,2] = 1) over the inliers: JtJ (packed upper), Jtr and |r|^2 into L.D.tot[0..44]
template <class F>
__device__ void lm_pass(DltLds& L, int n, F get, const double* h) {
  double acc[45];
#pragma unroll
  for (int e = 0; e < 45; ++e) acc[e] = 0.0;
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    Pt q;
    if (!get(j, q)) continue;
    const double Mx = (double)q.X, My = (double)q.Y;
    double ww = (h[6] * Mx + h[7] * My) + 1.0;
    ww = fabs(ww) > DBL_EPS ? 1.0 / ww : 0.0;
    const double xi = ((h[0] * Mx + h[1] * My) + h[2]) * ww, yi = ((h[3] * Mx + h[4] * My) + h[5]) * ww;
    const double r0 = xi - (double)q.x, r1 = yi - (double)q.y;
    const double J0[8] = {Mx * ww, My * ww, ww, 0.0, 0.0, 0.0, -Mx * ww * xi, -My * ww * xi};
    const double J1[8] = {0.0, 0.0, 0.0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
    int e = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = r; c < 8; ++c, ++e) acc[e] += J0[r] * J0[c] + J1[r] * J1[c];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[36 + r] += J0[r] * r0 + J1[r] * r1;
    acc[44] += r0 * r0 + r1 * r1;
  }
  block_sum<45>(L, acc);
}

__global__ __launch_bounds__(256) void hg_refine_kernel(const HgArgs a) {
  __shared__ RefineLds L;
  __shared__ int red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(a.nmatch[b], a.p.cap);
  const size_t cap = a.p.cap;
  uint8_t* mout = a.mask_out + b * cap;
  for (size_t j = tid; j < cap; j += 256) mout[j] = 0;
  int status = n < 4 ? -1 : -2, ninl = 0;
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int bi = n == 4 ? 0 : (n > 4 ? a.w.scan[b].best : -1);
  if (bi >= 0 && a.w.cnt[(size_t)b * a.p.max_iters + bi] >= 0) {  // uniform across the workgroup
    const double* Hb = a.w.H + ((size_t)b * a.p.max_iters + bi) * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) H[e] = Hb[e];
    if (n == 4) {
      for (int j = tid; j < n; j += 256) mout[j] = 1;
      status = 0;
      ninl = 4;
    } else {
      float Hf[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) Hf[e] = (float)H[e];
      const float thr2 = (float)(a.p.thresh * a.p.thresh);
      int c = 0;
      for (int j0 = 0; j0 < n; j0 += 256) {  // thread tid owns the points tid, tid + 256, ...: it alone writes and reads their mask
        const int j = j0 + tid;
        const bool in = j < n && reproj_err(Hf, load_pt(a, b, j < n ? j : 0)) <= thr2;
        if (j < n) mout[j] = in;
        c += __popcll(__ballot(in));
      }
      if ((tid & 63) == 0) red[tid >> 6] = c;
      __syncthreads();
      ninl = red[0] + red[1] + red[2] + red[3];
      auto get = [&](int j, Pt& q) {
        if (!mout[j]) return false;
        q = load_pt(a, b, j);
        return true;
      };
      // the refit on the inliers, then the polish of its first 8 entries
      bool ok = dlt_fit(L.D, n, get, H);
      if (ok) {
        double h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = H[e];
        lm_pass(L.D, n, get, h);
        if (tid < 45) L.cur[tid] = L.D.tot[tid];
        __syncthreads();
        double lambda = 1e-3;
        for (int iter = 0; iter < LM_ITERS; ++iter) {
          if (tid < 72) {
            const int r = tid / 9, k = tid % 9;
            L.M[r][k] = k == 8 ? L.cur[36 + r] : L.cur[r <= k ? tri8(r, k) : tri8(k, r)] + (r == k ? lambda * L.cur[tri8(r, r)] : 0.0);
          }
          __syncthreads();
          double d[8], hd[8], dmax = 0.0;
          if (!gauss_jordan<8, 9>(L.M, L.fac, 0.0)) break;
#pragma unroll
          for (int e = 0; e < 8; ++e) d[e] = L.M[e][8];
          bool fin = true;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            fin &= isfinite(d[e]);
            dmax = fmax(dmax, fabs(d[e]));
            hd[e] = h[e] - d[e];
          }
          if (!fin) break;
          lm_pass(L.D, n, get, hd);
          const double S = L.cur[44], Sd = L.D.tot[44];
          __syncthreads();
          if (Sd < S) {
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = hd[e];
            if (tid < 45) L.cur[tid] = L.D.tot[tid];
            lambda = lambda / 10.0;
          } else {
            lambda = lambda * 10.0;
          }
          __syncthreads();
          if (dmax < FLT_EPS) break;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) H[e] = h[e];
        H[8] = 1.0;
        status = bi;
      } else {
        for (int j = tid; j < n; j += 256) mout[j] = 0;
      }
    }
  }
  if (tid != 0) return;
  a.status[b] = status;
  double* Ho = a.H_out + (size_t)b * 9;
  const int nt = a.p.n_thr;
  double* rows = a.rows_out ? a.rows_out + (size_t)b * (2 + nt) : nullptr;
  if (status < 0) {
    for (int i = 0; i < 9; ++i) Ho[i] = 0.0;
    if (rows) {
      for (int i = 0; i < nt; ++i) rows[i] = 0.0;
      rows[nt] = __longlong_as_double(0x7ff0000000000000LL);
      rows[nt + 1] = 0.0;
    }
    return;
  }
  for (int i = 0; i < 9; ++i) Ho[i] = H[i];
  if (!rows) return;
  rows[nt + 1] = (double)ninl / (double)n;  // mask.mean()
  if (!a.img_shape || !a.H_true) {
    for (int i = 0; i <= nt; ++i) rows[i] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  // update_one (matching_metrics.py:265-297): the four corners through both homographies in float32
  const float wm = (float)(a.img_shape[2 * b + 1] - 1), hm = (float)(a.img_shape[2 * b] - 1);
  const float* T = a.H_true + (size_t)b * 9;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float cx = (k & 1) ? wm : 0.f, cy = (k & 2) ? hm : 0.f;
    float pt[2][2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      float m[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) m[e] = w == 0 ? T[e] : (float)H[e];
      const float u = (cx * m[0] + cy * m[1]) + m[2], v = (cx * m[3] + cy * m[4]) + m[5], z = (cx * m[6] + cy * m[7]) + m[8];
      pt[w][0] = u / z;
      pt[w][1] = v / z;
    }
    const float dx = pt[0][0] - pt[1][0], dy = pt[0][1] - pt[1][1];
    sum += sqrtf(dx * dx + dy * dy);
  }
  const float mean_dist = sum / 4.f;
  for (int i = 0; i < nt; ++i) rows[i] = mean_dist <= a.p.he_thr[i] ? 1.0 : 0.0;
  rows[nt] = (double)mean_dist;
}

// the fit alone on double points (test aid): x1 / x2 [n_points, 2] of problem blockIdx.x, rounded to the float32 the estimator stores
__global__ __launch_bounds__(256) void hg_dlt_kernel(const double* x1, const double* x2, int n_points, double* H_out, int32_t* ok_out) {
  __shared__ DltLds L;
  const int pb = blockIdx.x;
  const double* p1 = x1 + (size_t)pb * n_points * 2;
  const double* p2 = x2 + (size_t)pb * n_points * 2;
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool ok = dlt_fit(L, n_points, [&](int j, Pt& q) {
    q = Pt{(float)p1[2 * j], (float)p1[2 * j + 1], (float)p2[2 * j], (float)p2[2 * j + 1]};
    return true;
  }, H);
  if (threadIdx.x == 0) {
    for (int e = 0; e < 9; ++e) H_out[(size_t)pb * 9 + e] = ok ? H[e] : 0.0;
    ok_out[pb] = ok;
  }
}

}  // namespace

EINX_EXPORT size_t einx_homography_ws_bytes(const einx_homography_params* p) {
  if (!p || p->struct_size != sizeof(einx_homography_params) || p->B <= 0 || p->cap <= 0 || p->max_iters <= 0) return 0;
  size_t bytes = 0;
  carve(p, nullptr, &bytes);
  return bytes;
}

EINX_EXPORT int einx_homography(const einx_homography_params* p, const float* mk0, const float* mk1, const int32_t* nmatch,
                                const int32_t* img_shape, const float* H_true, void* ws, double* H_out, uint8_t* mask_out, int32_t* status,
                                double* rows_out, void* stream) {
  EINX_CHECK_ARG(p && p->struct_size == sizeof(einx_homography_params), "einx_homography_params.struct_size mismatch");
  EINX_CHECK_ARG(mk0 && mk1 && nmatch && ws && H_out && mask_out && status, "null pointer");
  EINX_CHECK_ARG(p->B > 0 && p->cap > 0 && (p->cols == 2 || p->cols == 3), "bad shape");
  EINX_CHECK_ARG(p->max_iters > 0 && p->max_iters <= 65535, "max_iters out of range");
  EINX_CHECK_ARG(p->n_thr >= 0 && p->n_thr <= 4, "n_thr is 0..4");
  EINX_CHECK_ARG(p->kp_yx == 0 || p->kp_yx == 1, "kp_yx is 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  HgArgs a;
  a.mk0 = mk0;
  a.mk1 = mk1;
  a.nmatch = nmatch;
  a.img_shape = img_shape;
  a.H_true = H_true;
  a.H_out = H_out;
  a.rows_out = rows_out;
  a.mask_out = mask_out;
  a.status = status;
  a.p = *p;
  a.w = carve(p, ws);
  const unsigned B = (unsigned)p->B;
  hipLaunchKernelGGL(hg_init_kernel, dim3((unsigned)einx_cdiv(p->B, 64)), dim3(64), 0, s, a);
  EINX_CHECK_LAUNCH();
  // a failed launch ends the rounds and stays pending for the check below
  ransac_rounds(p->max_iters, [&](int it0, int it1) {
    hipLaunchKernelGGL(hg_solve_kernel, dim3((unsigned)(it1 - it0), B), dim3(64), 0, s, a, it0);
    if (hipPeekAtLastError() != hipSuccess) return false;
    hipLaunchKernelGGL(hg_score_kernel, dim3((unsigned)(it1 - it0), B), dim3(256), 0, s, a, it0);
    if (hipPeekAtLastError() != hipSuccess) return false;
    hipLaunchKernelGGL((ransac_select_kernel<4, 1, HgModels>), dim3((unsigned)einx_cdiv(p->B, 64)), dim3(64), 0, s, a.w.scan, nmatch, p->B,
                       p->cap, p->max_iters, p->conf, it0, it1, HgModels{a.w.cnt});
    return hipPeekAtLastError() == hipSuccess;
  });
  EINX_CHECK_LAUNCH();
  hipLaunchKernelGGL(hg_refine_kernel, dim3(B), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_homography_dlt(const double* x1, const double* x2, int n_problems, int n_points, double* H_out, int32_t* ok,
                                    void* stream) {
  EINX_CHECK_ARG(x1 && x2 && H_out && ok, "null pointer");
  EINX_CHECK_ARG(n_problems > 0 && n_points >= 4, "n_problems > 0, n_points >= 4");
  hipLaunchKernelGGL(hg_dlt_kernel, dim3((unsigned)n_problems), dim3(256), 0, (hipStream_t)stream, x1, x2, n_points, H_out, ok);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
