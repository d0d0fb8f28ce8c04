// warp.hip -- batched perspective warp on gfx950: view 1 of a homographic pair is view 0's image under a known
// homography, so that every correspondence of the pair is exact and no depth is needed (the protocol SuperPoint, SiLK and
// LightGlue are validated with).  The reference ships the sampler of such homographies (core/geometry/homography.py) and never
// calls it; nothing in it warps an image.
//
// One thread per destination pixel, threads consecutive along x (the stores are dense, the four taps of neighbouring threads lie
// on neighbouring source addresses for every homography near the identity).  The source point and the weights are float64 /
// float32 expressions evaluated once per pixel and reused over the C channels; -ffp-contract=off: every operation is rounded as
// it is written, which is what tests/warp_ref.py restates.  The nine entries of a sample's matrix depend on blockIdx alone.
#include "einx_common.h"

#include <math.h>

namespace {

__device__ __forceinline__ float warp_load(const uint8_t* p) { return (float)*p; }
__device__ __forceinline__ float warp_load(const float* p) { return *p; }
__device__ __forceinline__ void warp_store(uint8_t* p, float v) { *p = (uint8_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }
__device__ __forceinline__ void warp_store(float* p, float v) { *p = v; }

template <typename T, bool NEAREST>
__global__ __launch_bounds__(256) void warp_perspective_kernel(const T* src, int B, int C, int Hs, int Ws, const double* Hinv, int Hd, int Wd,
                                                               T* dst, uint8_t* valid) {
  const long long HW = (long long)Hd * Wd;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const double x = (double)(i % Wd) + 0.5, y = (double)(i / Wd) + 0.5;  // the pixel's centre
  const size_t plane = (size_t)Hs * Ws;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const double* h = Hinv + 9 * (size_t)b;
    const double X = (h[0] * x + h[1] * y) + h[2];
    const double Y = (h[3] * x + h[4] * y) + h[5];
    const double w = (h[6] * x + h[7] * y) + h[8];
    const double qx = X / w, qy = Y / w;
    // all four taps inside the source; NaN fails every comparison
    const bool ok = isfinite(w) && w > 0.0 && qx >= 0.5 && qx <= (double)Ws - 0.5 && qy >= 0.5 && qy <= (double)Hs - 0.5;
    if (valid) valid[(size_t)b * HW + i] = ok ? 1 : 0;
    const double sx = qx - 0.5, sy = qy - 0.5;  // index coordinates: 0 <= sx <= Ws - 1 where ok
    const T* s = src + (size_t)b * C * plane;
    T* d = dst + (size_t)b * C * HW + i;
    if (!ok) {
      for (int c = 0; c < C; ++c) warp_store(d + (size_t)c * HW, 0.0f);
    } else if (NEAREST) {
      const size_t at = (size_t)rint(sy) * Ws + (size_t)rint(sx);  // half to even
      for (int c = 0; c < C; ++c) d[(size_t)c * HW] = s[(size_t)c * plane + at];
    } else {
      const double x0d = floor(sx), y0d = floor(sy);
      const float fx = (float)(sx - x0d), fy = (float)(sy - y0d);
      const float gx = 1.0f - fx, gy = 1.0f - fy;
      const float w00 = gx * gy, w01 = fx * gy, w10 = gx * fy, w11 = fx * fy;
      const int x0 = (int)x0d, y0 = (int)y0d;
      // sx == Ws - 1 (sy == Hs - 1): the right (lower) taps have weight 0 and lie outside: they read as 0, they are not loaded
      const bool r = x0 + 1 < Ws, lo = y0 + 1 < Hs;
      const size_t at = (size_t)y0 * Ws + x0;
      for (int c = 0; c < C; ++c) {
        const T* p = s + (size_t)c * plane + at;
        const float i00 = warp_load(p), i01 = r ? warp_load(p + 1) : 0.0f;
        const float i10 = lo ? warp_load(p + Ws) : 0.0f, i11 = lo && r ? warp_load(p + Ws + 1) : 0.0f;
        warp_store(d + (size_t)c * HW, ((w00 * i00 + w01 * i01) + w10 * i10) + w11 * i11);
      }
    }
  }
}

template <typename T>
void warp_launch(int mode, dim3 grid, hipStream_t s, const void* src, int B, int C, int Hs, int Ws, const double* Hinv, int Hd, int Wd, void* dst,
                 uint8_t* valid) {
  if (mode == EINX_WARP_NEAREST)
    hipLaunchKernelGGL((warp_perspective_kernel<T, true>), grid, dim3(256), 0, s, (const T*)src, B, C, Hs, Ws, Hinv, Hd, Wd, (T*)dst, valid);
  else
    hipLaunchKernelGGL((warp_perspective_kernel<T, false>), grid, dim3(256), 0, s, (const T*)src, B, C, Hs, Ws, Hinv, Hd, Wd, (T*)dst, valid);
}

}  // namespace

EINX_EXPORT int einx_warp_perspective(const void* src, int src_type, int B, int C, int Hs, int Ws, const double* Hinv, int Hd, int Wd, int mode,
                                      void* dst, uint8_t* valid, void* stream) {
  EINX_CHECK_ARG(src_type == EINX_REMAP_U8 || src_type == EINX_REMAP_F32, "src_type must be EINX_REMAP_U8 or EINX_REMAP_F32");
  EINX_CHECK_ARG(mode == EINX_WARP_BILINEAR || mode == EINX_WARP_NEAREST, "mode must be EINX_WARP_BILINEAR or EINX_WARP_NEAREST");
  EINX_CHECK_ARG(B >= 0 && C >= 0 && Hs >= 0 && Ws >= 0 && Hd >= 0 && Wd >= 0, "a size is negative");
  const long long HW = (long long)Hd * Wd, gx = (HW + 255) / 256;
  if (B == 0 || HW == 0 || (C == 0 && !valid)) return EINX_OK;  // nothing to write
  EINX_CHECK_ARG(Hinv && (C == 0 || dst) && (C == 0 || (long long)Hs * Ws == 0 || src), "null pointer");
  EINX_CHECK_ARG(gx < (1ll << 31), "a destination of 2^39 pixels or more");
  const dim3 grid((unsigned)gx, (unsigned)(B < 65535 ? B : 65535));
  if (src_type == EINX_REMAP_U8)
    warp_launch<uint8_t>(mode, grid, (hipStream_t)stream, src, B, C, Hs, Ws, Hinv, Hd, Wd, dst, valid);
  else
    warp_launch<float>(mode, grid, (hipStream_t)stream, src, B, C, Hs, Ws, Hinv, Hd, Wd, dst, valid);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
