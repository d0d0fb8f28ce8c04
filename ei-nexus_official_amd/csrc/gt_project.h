// gt_project.h -- the depth sampler and the pinhole projection of DESIGN.md 8e, stage A, for every file that projects a keypoint
// through a depth map: gt_matches.hip (ground-truth labels) and metrics.hip (einx_pair_metrics_pose).  One text, so
// that both produce the same bits.  fp32, unfused (-ffp-contract=off).
//
// Replaces (reference file:line): core/geometry/depth.py:9-69 (sample_fmap, sample_depth, project), core/geometry/wrappers.py:337-385
// (pinhole cam2image).
#pragma once
#include "einx_common.h"

namespace {

// sample_depth (depth.py:9-25): bilinear with zero padding at ix = x - 0.5; a hole (<= 0 or NaN) under a tap of non-zero weight
// sends the whole sample to the nearest pixel (half to even), NaN when that is a hole, 0 outside the map
// NAN_HOLE: the same sampler for a feature map (depth.py:9-17, sample_fmap): a hole is a NaN and nothing else
template <bool NAN_HOLE>
__device__ __forceinline__ float gt_sample_map(const float* dm, int H, int W, float x, float y) {
  const float nan = einx_u2f(0x7fc00000u);
  const float ix = x - 0.5f, iy = y - 0.5f;
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const float tx = ix - fx0, ty = iy - fy0;
  // floorf of anything outside the int range (or NaN) is clamped so that the casts are defined: every tap is then outside the map
  const int x0 = fx0 >= -2.0f && fx0 <= (float)W ? (int)fx0 : -2;
  const int y0 = fy0 >= -2.0f && fy0 <= (float)H ? (int)fy0 : -2;
  const float wx[2] = {(fx0 + 1.0f) - ix, tx};
  const float wy[2] = {(fy0 + 1.0f) - iy, ty};
  float acc = 0.0f;
  bool hole = false;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {  // nw, ne, sw, se
      const int xx = x0 + dx, yy = y0 + dy;
      if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
      const float w = wx[dx] * wy[dy];
      const float v = dm[(size_t)yy * W + xx];
      if (NAN_HOLE ? v != v : !(v > 0.0f)) {
        if (w != 0.0f) hole = true;
        continue;
      }
      acc = acc + v * w;
    }
  }
  if (!hole && ix == ix && iy == iy) return acc;
  const float nx = nearbyintf(ix), ny = nearbyintf(iy);  // round half to even (the default rounding mode)
  if (!(nx >= 0.0f && nx < (float)W && ny >= 0.0f && ny < (float)H)) return 0.0f;
  const float v = dm[(size_t)(int)ny * W + (int)nx];
  if (NAN_HOLE) return v;
  return v > 0.0f ? v : nan;
}

__device__ __forceinline__ float gt_sample_depth(const float* dm, int H, int W, float x, float y) {
  return gt_sample_map<false>(dm, H, W, x, y);
}

// (R, t) of the motion this view -> the other: T's, or with T null (R^T, -R^T t) of T_other
__device__ __forceinline__ void gt_pose_rt(const float* T, const float* T_other, float* R, float* t) {
  if (T) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * q + c] = T[4 * q + c];
      t[q] = T[4 * q + 3];
    }
  } else {  // (R^T, -R^T t) of the other direction
    T = T_other;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * q + c] = T[4 * c + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = -((R[3 * q] * T[3] + R[3 * q + 1] * T[7]) + R[3 * q + 2] * T[11]);
  }
}

// image2cam of camera Ks, scale by the depth, transform by (R, t), cam2image (pinhole) of camera Ko
__device__ __forceinline__ bool gt_transform_project(float x, float y, float d, const float* Ks, const float* Ko, const float* R,
                                                     const float* t, float* u_out, float* v_out) {
  const float px = ((x - Ks[2]) / Ks[0]) * d, py = ((y - Ks[5]) / Ks[4]) * d, pz = d;
  const float qx = ((px * R[0] + py * R[1]) + pz * R[2]) + t[0];
  const float qy = ((px * R[3] + py * R[4]) + pz * R[5]) + t[1];
  const float qz = ((px * R[6] + py * R[7]) + pz * R[8]) + t[2];
  const bool front = qz > 1e-4f;
  const float z = qz < 1e-4f ? 1e-4f : qz;  // clamp(min=eps): NaN stays NaN
  const float u = (qx / z) * Ko[0] + Ko[2];
  const float v = (qy / z) * Ko[4] + Ko[5];
  // the camera's size is (2 cx, 2 cy) (Camera.from_calibration_matrix), not the depth map's
  const float wmax = 2.0f * Ko[2] - 1.0f, hmax = 2.0f * Ko[5] - 1.0f;
  *u_out = u;
  *v_out = v;
  return front && u >= 0.0f && u <= wmax && v >= 0.0f && v <= hmax;
}

// depth.py:37-60 with ccth=None for one point (x, y) of depth d: image2cam, scale by the depth, transform by T (this view -> the
// other; null: (R^T, -R^T t) of T_other), pinhole cam2image of the other camera Ko.  (u, v) is the projection, NaN where d is; the
// return value is "in front of the other camera and inside its image"
__device__ __forceinline__ bool gt_project_point(float x, float y, float d, const float* Ks, const float* Ko, const float* T,
                                                 const float* T_other, float* u_out, float* v_out) {
  float R[9], t[3];
  gt_pose_rt(T, T_other, R, t);
  return gt_transform_project(x, y, d, Ks, Ko, R, t, u_out, v_out);
}

// The other view's depth under a projection, for the cycle check of gt_project_cc: the map dm [H,W] is sampled at (u, v) with
// gt_sample_depth, or (dm null) the caller sampled it already: dj with its validity
struct GtOtherDepth {
  const float* dm;
  int H, W;
  float dj;
  bool validj;
};

// depth.py:37-69 for one point: gt_project_point, bit for bit, for (u, v) and -- without `cc` -- for the return value.  With
// `cc` (ccth given) the point must also survive the way back: the other view's depth dj at (u, v) must be valid (not NaN, > 0),
// (u, v) at depth dj taken through the INVERSE OF THE FORWARD MOTION (depth.py:65 T_itoj.inv(): (R^T, -R^T t) of the (R, t) used
// above, whichever way that was obtained; not the caller's pose of the other direction) must land in front of and inside this
// view's camera (2c - 1 bounds), and (x - x')^2 + (y - y')^2 < bound, strictly; a NaN fails.  The bound is compared with the
// SQUARED distance as given (the reference compares squared pixels with its unsquared ccth).  *dj_out: the depth that was used.
__device__ __forceinline__ bool gt_project_cc(float x, float y, float d, const float* Ks, const float* Ko, const float* T,
                                              const float* T_other, bool cc, float bound, const GtOtherDepth& od, float* u_out,
                                              float* v_out, float* dj_out) {
  float R[9], t[3];
  gt_pose_rt(T, T_other, R, t);
  float u, v;
  const bool seen = gt_transform_project(x, y, d, Ks, Ko, R, t, &u, &v);
  *u_out = u;
  *v_out = v;
  if (!cc) return seen;
  float dj = od.dj;
  bool validj = od.validj;
  if (od.dm) {
    dj = gt_sample_depth(od.dm, od.H, od.W, u, v);
    validj = dj == dj && dj > 0.0f;
  }
  *dj_out = dj;
  float Ri[9], ti[3];  // Pose.inv of (R, t)
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int c = 0; c < 3; ++c) Ri[3 * q + c] = R[3 * c + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) ti[q] = -((Ri[3 * q] * t[0] + Ri[3 * q + 1] * t[1]) + Ri[3 * q + 2] * t[2]);
  float bx, by;
  const bool back = gt_transform_project(u, v, dj, Ko, Ks, Ri, ti, &bx, &by);
  const float ex = x - bx, ey = y - by;
  const bool consistent = (ex * ex + ey * ey) < bound;
  return seen && consistent && back && validj;
}

// q.z of gt_project_point alone: the same products in the same order, so `gt_point_qz(...) > 1e-4f` is that function's `front`
// for a caller whose image bound is not the camera's (2 cx, 2 cy)
__device__ __forceinline__ float gt_point_qz(float x, float y, float d, const float* Ks, const float* T, const float* T_other) {
  const float px = ((x - Ks[2]) / Ks[0]) * d, py = ((y - Ks[5]) / Ks[4]) * d, pz = d;
  if (T) return ((px * T[8] + py * T[9]) + pz * T[10]) + T[11];
  // row 2 of R^T is column 2 of T_other's rotation; t.z = -(that row . T_other's translation)
  const float r0 = T_other[2], r1 = T_other[6], r2 = T_other[10];
  const float tz = -((r0 * T_other[3] + r1 * T_other[7]) + r2 * T_other[11]);
  return ((px * r0 + py * r1) + pz * r2) + tz;
}

}  // namespace
