// The RANSAC skeleton shared by the estimators (pose.hip: DESIGN.md 8b, homography.hip: 8c, abs_pose.hip: 8u): the counter-based
// generator and its distinct-index draws, the selection scan with OpenCV's shrinking iteration bound and the state it keeps between rounds, the
// host's round schedule, and the cooperative Gauss-Jordan elimination.  An estimator adds its minimal solver, its error function,
// its inlier count, its epilogue and the carve of its workspace (WsCarver: einx_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr int RANSAC_RETRIES = 64;  // tries of one draw for an index not drawn before

// M distinct indices of [0, n) for attempt `att` of iteration `it` (an estimator that draws once per iteration passes att = 0);
// false when a draw finds no new index within RANSAC_RETRIES tries
template <int M>
__device__ __forceinline__ bool ransac_draw(unsigned long long seed, int it, int att, int n, int* idx) {
#pragma unroll
  for (int d = 0; d < M; ++d) {
    bool got = false;
    for (int r = 0; r < RANSAC_RETRIES && !got; ++r) {
      const unsigned long long key =
          ((unsigned long long)att << 32) | ((unsigned long long)it << 16) | ((unsigned long long)d << 8) | (unsigned long long)r;
      const int v = (int)(splitmix64(seed ^ key) % (unsigned long long)n);
      bool dup = false;
#pragma unroll
      for (int e = 0; e < M - 1; ++e) dup |= e < d && idx[e] == v;
      if (!dup) {
        idx[d] = v;
        got = true;
      }
    }
    if (!got) return false;
  }
  return true;
}

// RANSACUpdateNumIters for a model of M points, with (1 - ep)^M as M - 1 products
template <int M>
__device__ int ransac_update_iters(double conf, double ep, int bound) {
  const double p = fmin(fmax(conf, 0.0), 1.0);
  ep = fmin(fmax(ep, 0.0), 1.0);
  double num = fmax(1.0 - p, 2.2250738585072014e-308);
  const double q = 1.0 - ep;
  double pw = q;
#pragma unroll
  for (int k = 1; k < M; ++k) pw = pw * q;
  double denom = 1.0 - pw;
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num);
  denom = log(denom);
  return denom >= 0 || -num >= bound * (-denom) ? bound : (int)floor(num / denom + 0.5);
}

// the selection scan's state of one pair between rounds
struct RansacScan {
  int32_t best;   // the RANSAC model so far (iteration * SLOTS + model of the iteration), -1 none
  int32_t count;  // its inlier count
  int32_t bound;  // the iteration bound: it only shrinks
};

__device__ __forceinline__ void ransac_scan_init(RansacScan& s, int max_iters) {
  s.best = -1;
  s.count = 0;
  s.bound = max_iters;
}

// the solve and score kernels of a round skip an iteration at or past the pair's current bound: the bound only shrinks, so the
// selection scan never reaches it
__device__ __forceinline__ bool ransac_live(const RansacScan& s, int it) { return it < s.bound; }

// OpenCV's sequential scan over one round [it0, it1), resumed from the state the previous round left; one lane per pair.  For the
// iteration at h = pair * max_iters + it, models.count(h) is the number of its models and models.inliers(h, k) the inlier count of
// model k; a model replaces the best one when it has more inliers and at least M of them.  SLOTS spaces the iterations in `best`.
template <int M, int SLOTS, class F>
__global__ void ransac_select_kernel(RansacScan* scan, const int32_t* nmatch, int B, int cap, int max_iters, double conf, int it0, int it1,
                                     const F models) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = min(nmatch[b], cap);
  if (n <= M) return;
  RansacScan s = scan[b];
  for (int it = it0; it < it1 && ransac_live(s, it); ++it) {
    const size_t h = (size_t)b * max_iters + it;
    const int nm = models.count(h);
    for (int k = 0; k < nm; ++k) {
      const int c = models.inliers(h, k);
      // a new best is rare (a handful per pair); unlikely keeps the bound's update, ~100 double-precision instructions, behind a branch
      if (__builtin_expect(c > max(s.count, M - 1), 0)) {
        s.best = it * SLOTS + k;
        s.count = c;
        s.bound = ransac_update_iters<M>(conf, (double)(n - c) / (double)n, s.bound);
      }
    }
  }
  scan[b] = s;
}

// The host's round schedule: f(it0, it1) for rounds of 32, 32, 64, 128, 256, 512.. iterations up to max_iters, stopping after the
// first round for which f returns false (a launch failed).  A round is solve, score, then the scan; each pair's workgroups past
// its bound exit at once.  The schedule is fixed (no host sync, capturable); the scan's result does not depend on it.
template <class F>
void ransac_rounds(int max_iters, F f) {
  for (int it0 = 0, len = 32; it0 < max_iters;) {
    const int it1 = it0 + len < max_iters ? it0 + len : max_iters;
    if (!f(it0, it1)) return;
    if (it1 >= 64) len *= 2;
    it0 = it1;
  }
}

// Gauss-Jordan with partial pivoting over the first R columns of the LDS matrix A[R][C], by the whole workgroup (fac[R] in LDS
// too; at least C threads).  false: a pivot that is not above tol (uniform across the workgroup).
template <int R, int C>
__device__ bool gauss_jordan(double (*A)[C], double* fac, double tol) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int c = 0; c < R; ++c) {
    int p = c;
    for (int r = c + 1; r < R; ++r)
      if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
    if (!(fabs(A[p][c]) > tol)) return false;
    __syncthreads();
    if (tid < C && p != c) {
      const double t = A[c][tid];
      A[c][tid] = A[p][tid];
      A[p][tid] = t;
    }
    __syncthreads();
    const double piv = A[c][c];
    __syncthreads();
    if (tid < C) A[c][tid] = A[c][tid] / piv;
    if (tid < R) fac[tid] = A[tid][c];
    __syncthreads();
    for (int q = tid; q < R * C; q += nt) {
      const int r = q / C, k = q % C;
      if (r != c) A[r][k] = A[r][k] - fac[r] * A[c][k];
    }
    __syncthreads();
  }
  return true;
}
