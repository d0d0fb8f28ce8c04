// Device helpers shared by the RANSAC estimators (pose.hip: DESIGN.md 8b, homography.hip: 8c): the counter-based generator and
// OpenCV's shrinking iteration bound.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
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
