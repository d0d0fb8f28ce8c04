// posetrack.hip -- a recording's pose track on gfx950: the step between "arrays of a recording" and "a batch the
// evaluator takes", which the reference runs on the host once per view of every sample.
//
// Replaces (reference file:line): datasets/Interpolator.py:27-69 (PoseInterpolator: scipy Slerp + three linear interp1d +
// np.linalg.inv per query), called from datasets/MVSEC.py:795 and datasets/EC.py:264-289; datasets/MVSEC.py:818-830
// (get_relative_pose: pose1 @ inv(pose0)) as used by :1081-1085; datasets/MVSEC.py:362-369 (nearest image per depth frame through an
// F_image x F_depth outer difference).
//
// One thread per query (or per pair), everything in float64: stamps are epoch seconds (~1.5e9) a few milliseconds apart, which
// float32 (spacing 128 s there) cannot hold.  -ffp-contract=off: every operation is rounded as it is written, so the float64 host
// restatement of the same expressions (tests/poses_f64.py) differs only where sin / atan2 / sqrt of the two platforms do.  The
// kernels are a binary search and some fifty dependent double operations per thread: latency-bound and microsecond-scale at any
// realistic Q, so they are kept plain (no LDS staging of the knots, no vector stores).  No workspace, no host synchronisation;
// the one atomic is an integer add of the out-of-range count, which is order-free.
#include "einx_common.h"

#include <math.h>

namespace {

constexpr int PT_THREADS = 64;  // one wave per workgroup: Q is a few thousand at most, this spreads it over more CUs

struct Track {
  const double* stamps;  // [N] strictly increasing
  const double* trans;   // [N,3]
  const double* quats;   // [N,4] unit, (x, y, z, w)
  int N;
};

struct Rigid {
  double R[9];  // row-major
  double p[3];
};

// first index in [0, n) whose element is not below q (n when there is none): np.searchsorted(a, q, side="left")
__device__ __forceinline__ long long lower_bound(const double* a, long long n, double q) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (a[mid] < q)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// T_W_j at q (Interpolator.py:64-68).  False (and nothing written) for a query outside [t_0, t_{N-1}] or NaN.
__device__ bool world_from_camera(const Track& k, double q, Rigid* o) {
  if (!(q >= k.stamps[0] && q <= k.stamps[k.N - 1])) return false;
  // the interval of Slerp.__call__ and of linear interp1d: a query on a knot belongs to the interval on its left (alpha = 1), the
  // first knot to interval 0 (alpha = 0)
  long long i = lower_bound(k.stamps, k.N, q) - 1;
  i = i < 0 ? 0 : (i > k.N - 2 ? k.N - 2 : i);
  const double t0 = k.stamps[i], dt = k.stamps[i + 1] - t0, dq = q - t0;
  const double alpha = dq / dt;
  // interp1d's order: slope = (y_hi - y_lo) / (x_hi - x_lo); y = slope * (x - x_lo) + y_lo
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double lo = k.trans[3 * i + c], hi = k.trans[3 * (i + 1) + c];
    o->p[c] = (hi - lo) / dt * dq + lo;
  }
  double q0[4], q1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    q0[c] = k.quats[4 * i + c];
    q1[c] = k.quats[4 * (i + 1) + c];
  }
  double d = ((q0[0] * q1[0] + q0[1] * q1[1]) + q0[2] * q1[2]) + q0[3] * q1[3];
  if (d < 0.0) {  // the shorter arc
    d = -d;
#pragma unroll
    for (int c = 0; c < 4; ++c) q1[c] = -q1[c];
  }
  // the angle between the two from atan2(|q1 - d q0|, d): well conditioned at both ends, where acos(d) is not
  double r[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) r[c] = q1[c] - d * q0[c];
  const double s = sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);
  const double theta = atan2(s, d);
  double w0, w1;
  if (theta < 1e-12) {  // sin(theta) has no digits left to divide by: normalised lerp
    w0 = 1.0 - alpha;
    w1 = alpha;
  } else {
    const double st = sin(theta);
    w0 = sin((1.0 - alpha) * theta) / st;
    w1 = sin(alpha * theta) / st;
  }
  double u[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) u[c] = w0 * q0[c] + w1 * q1[c];
  const double nrm = sqrt(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3]);
  const double x = u[0] / nrm, y = u[1] / nrm, z = u[2] / nrm, w = u[3] / nrm;
  const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
  const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
  o->R[0] = x2 - y2 - z2 + w2;
  o->R[3] = 2.0 * (xy + zw);
  o->R[6] = 2.0 * (xz - yw);
  o->R[1] = 2.0 * (xy - zw);
  o->R[4] = -x2 + y2 - z2 + w2;
  o->R[7] = 2.0 * (yz + xw);
  o->R[2] = 2.0 * (xz + yw);
  o->R[5] = 2.0 * (yz - xw);
  o->R[8] = -x2 - y2 + z2 + w2;
  return true;
}

// the inverse of a rigid transform in closed form: [R^T | -R^T p]
__device__ __forceinline__ Rigid rigid_inverse(const Rigid& a) {
  Rigid o;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o.R[3 * r + c] = a.R[3 * c + r];
    o.p[r] = -((a.R[r] * a.p[0] + a.R[3 + r] * a.p[1]) + a.R[6 + r] * a.p[2]);
  }
  return o;
}

// a b
__device__ __forceinline__ Rigid compose(const Rigid& a, const Rigid& b) {
  Rigid o;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o.R[3 * r + c] = (a.R[3 * r] * b.R[c] + a.R[3 * r + 1] * b.R[3 + c]) + a.R[3 * r + 2] * b.R[6 + c];
    o.p[r] = ((a.R[3 * r] * b.p[0] + a.R[3 * r + 1] * b.p[1]) + a.R[3 * r + 2] * b.p[2]) + a.p[r];
  }
  return o;
}

// one [4,4] row-major matrix; ok == false: sixteen NaNs
template <typename T>
__device__ __forceinline__ void store_pose(T* out, const Rigid& a, bool ok) {
  const T nan = (T)__builtin_nan("");
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[4 * r + c] = ok ? (T)a.R[3 * r + c] : nan;
    out[4 * r + 3] = ok ? (T)a.p[r] : nan;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) out[12 + c] = ok ? (T)(c == 3 ? 1.0 : 0.0) : nan;
}

template <typename T>
__global__ __launch_bounds__(PT_THREADS) void pose_interp_kernel(const Track k, const double* queries, int Q, int inverse, T* out,
                                                                 int32_t* out_of_range) {
  const long long j = (long long)blockIdx.x * PT_THREADS + threadIdx.x;  // Q may come within 63 of 2^31
  if (j >= Q) return;
  Rigid a{};
  const bool ok = world_from_camera(k, queries[j], &a);
  if (ok && inverse) a = rigid_inverse(a);
  store_pose(out + (size_t)j * 16, a, ok);
  if (!ok) atomicAdd(out_of_range, 1);
}

__global__ __launch_bounds__(PT_THREADS) void pose_relative_kernel(const Track k, const double* q0, const double* q1, int P, float* T_0to1,
                                                                   float* T_1to0, int32_t* out_of_range) {
  const long long j = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
  if (j >= P) return;
  Rigid a{}, b{};  // T_W_0, T_W_1
  const bool ok0 = world_from_camera(k, q0[j], &a), ok1 = world_from_camera(k, q1[j], &b);
  const bool ok = ok0 && ok1;
  Rigid ab{}, ba{};
  if (ok) {
    ab = compose(rigid_inverse(b), a);  // T_1_W T_W_0
    ba = compose(rigid_inverse(a), b);  // T_0_W T_W_1
  }
  store_pose(T_0to1 + (size_t)j * 16, ab, ok);
  store_pose(T_1to0 + (size_t)j * 16, ba, ok);
  const int bad = (int)!ok0 + (int)!ok1;
  if (bad) atomicAdd(out_of_range, bad);
}

// The first index that minimises fabs(stamps[i] - q) as float64 rounds it.  With j the first stamp that is not below q, the rounded
// difference stamps[i] - q does not decrease in i (rounding is monotone), so the rounded distance does not increase over [0, j) and
// does not decrease over [j, F): the minimum is at j - 1 or at j.  Left of the query DIFFERENT stamps can round to the same
// distance (and equal stamps do), so when the minimum lies there its first occurrence is bisected for: dist(i) <= m is monotone
// on [0, j).  A tie between the two sides goes to the left one, the lower index.  NaN: every comparison fails, j = 0, index 0.
__global__ __launch_bounds__(PT_THREADS) void nearest_stamp_kernel(const double* stamps, long long F, const double* queries, long long Q,
                                                                   int64_t* out) {
  const long long k = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
  if (k >= Q) return;
  const double q = queries[k];
  const long long j = lower_bound(stamps, F, q);
  long long best;
  if (j == 0 || (j < F && fabs(stamps[j] - q) < fabs(stamps[j - 1] - q))) {
    best = j;  // (j == 0 < F)
  } else {
    const double m = fabs(stamps[j - 1] - q);
    long long lo = 0, hi = j - 1;
    while (lo < hi) {
      const long long mid = lo + ((hi - lo) >> 1);
      if (fabs(stamps[mid] - q) <= m)
        hi = mid;
      else
        lo = mid + 1;
    }
    best = lo;
  }
  out[k] = best;
}

int check_track(const char* name, const double* stamps, const double* trans, const double* quats, int N) {
  if (!(stamps && trans && quats)) {
    einx_set_error("%s: null track pointer", name);
    return EINX_ERR_ARG;
  }
  if (N < 2) {
    einx_set_error("%s: a track needs at least two knots", name);
    return EINX_ERR_ARG;
  }
  return EINX_OK;
}

int zero_counter(const char* name, int32_t* out_of_range, hipStream_t s) {
  if (hipMemsetAsync(out_of_range, 0, sizeof(int32_t), s) != hipSuccess) {
    einx_set_error("%s: memset failed", name);
    return EINX_ERR_LAUNCH;
  }
  return EINX_OK;
}

}  // namespace

EINX_EXPORT int einx_pose_interp(const double* stamps, const double* trans, const double* quats, int N, const double* queries, int Q,
                                 int inverse, int out_type, void* out, int32_t* out_of_range, void* stream) {
  if (int e = check_track(__func__, stamps, trans, quats, N)) return e;
  EINX_CHECK_ARG(Q >= 0, "Q is negative");
  EINX_CHECK_ARG(out_of_range && (Q == 0 || (queries && out)), "null pointer");
  EINX_CHECK_ARG(out_type == EINX_POSE_F32 || out_type == EINX_POSE_F64, "out_type must be EINX_POSE_F32 or EINX_POSE_F64");
  hipStream_t s = (hipStream_t)stream;
  if (int e = zero_counter(__func__, out_of_range, s)) return e;
  if (Q == 0) return EINX_OK;
  const Track k{stamps, trans, quats, N};
  const dim3 grid((unsigned)einx_cdiv(Q, PT_THREADS));
  if (out_type == EINX_POSE_F32)
    hipLaunchKernelGGL(pose_interp_kernel<float>, grid, dim3(PT_THREADS), 0, s, k, queries, Q, inverse != 0, (float*)out, out_of_range);
  else
    hipLaunchKernelGGL(pose_interp_kernel<double>, grid, dim3(PT_THREADS), 0, s, k, queries, Q, inverse != 0, (double*)out, out_of_range);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_pose_relative(const double* stamps, const double* trans, const double* quats, int N, const double* q0, const double* q1,
                                   int P, float* T_0to1, float* T_1to0, int32_t* out_of_range, void* stream) {
  if (int e = check_track(__func__, stamps, trans, quats, N)) return e;
  EINX_CHECK_ARG(P >= 0, "P is negative");
  EINX_CHECK_ARG(out_of_range && (P == 0 || (q0 && q1 && T_0to1 && T_1to0)), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (int e = zero_counter(__func__, out_of_range, s)) return e;
  if (P == 0) return EINX_OK;
  const Track k{stamps, trans, quats, N};
  hipLaunchKernelGGL(pose_relative_kernel, dim3((unsigned)einx_cdiv(P, PT_THREADS)), dim3(PT_THREADS), 0, s, k, q0, q1, P, T_0to1, T_1to0,
                     out_of_range);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_nearest_stamp(const double* stamps, int64_t F, const double* queries, int64_t Q, int64_t* out, void* stream) {
  EINX_CHECK_ARG(F > 0, "F must be positive: there is no nearest stamp among none");
  EINX_CHECK_ARG(Q >= 0, "Q is negative");
  EINX_CHECK_ARG(stamps && (Q == 0 || (queries && out)), "null pointer");
  const long long blocks = ((long long)Q + PT_THREADS - 1) / PT_THREADS;
  EINX_CHECK_ARG(blocks < (1ll << 31), "Q too large for one launch");
  if (Q == 0) return EINX_OK;
  hipLaunchKernelGGL(nearest_stamp_kernel, dim3((unsigned)blocks), dim3(PT_THREADS), 0, (hipStream_t)stream, stamps, (long long)F, queries,
                     (long long)Q, out);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
