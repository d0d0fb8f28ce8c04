// subpixel.hip -- opt-in sub-pixel keypoints on gfx950: a separable parabola through a selected peak of the
// score map and its two neighbours per axis, and the bilinear descriptor sampler of desc.hip at a FLOAT position (the
// reference's sparsify_low_resolution_descriptors for any position: core/modules/utils/descriptor_util.py:74-128, grid_sample
// with align_corners=False and zero padding, then F.normalize * scale).
//
// One launch, shaped like desc_sample_kernel: one wave per keypoint, four keypoints per workgroup, blockIdx.y = image.  The
// per-element operation order of the sampling and of the normalisation is desc_sample_kernel's, so a refined keypoint with
// offset (0, 0), or a given position (y + 0.5, x + 0.5), reproduces its row bit for bit.
#include "einx_common.h"

namespace {

__device__ __forceinline__ float wave_butterfly_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// |offset| <= 0.5 - 2^-10: for map sides up to 8192 (13 integer bits, 10 fraction bits left of float32's 24 after the 0.5)
// fl(fl(y + 0.5) + offset) stays strictly below y + 1, so floor() of a refined position is still the detected pixel
constexpr float SUBPIX_DMAX = 0.5f - 0x1p-10f;
constexpr int SUBPIX_MAX_SIDE = 8192;

// vertex of the parabola through (-1, l), (0, c), (+1, r), relative to the centre; 0 unless c is a strict maximum of the three
// (ties and NaN included).  Every operation rounds once, in this order; the division is IEEE.
__device__ __forceinline__ float subpixel_offset(float l, float c, float r) {
  if (!(l < c && r < c)) return 0.0f;
  const float a = l - c, b = r - c;
  const float den = a + b, num = l - r;
  const float delta = (0.5f * num) / den;
  return fminf(fmaxf(delta, -SUBPIX_DMAX), SUBPIX_DMAX);
}

// the four taps of the [hc,wc] map and their weights for the padded-frame position (posy, posx) (pixel centres at .5), with
// desc_sample_kernel's formula and operation order from py = posy - 0.5 on.  The un-normalised map coordinate is compared AS A
// FLOAT against (-1, size) before anything is converted to int: outside that window (NaN included) all four taps lie outside
// the map anyway, so they are declared invalid with zero weights and no integer, let alone an address, is formed from it.
struct SubpixTaps {
  float nw, ne, sw, se;
  int x0, y0, x1, y1;
  bool vx0, vx1, vy0, vy1;
};

__device__ __forceinline__ SubpixTaps subpixel_taps(float posy, float posx, int hc, int wc, int Hp, int Wp) {
  SubpixTaps t;
  const float py = posy - 0.5f, px = posx - 0.5f;
  const float gy = 2.0f * (py / (float)(Hp - 1)) - 1.0f;
  const float gx = 2.0f * (px / (float)(Wp - 1)) - 1.0f;
  const float iy = ((gy + 1.0f) * (float)hc - 1.0f) / 2.0f;
  const float ix = ((gx + 1.0f) * (float)wc - 1.0f) / 2.0f;
  const bool ok = iy > -1.0f && iy < (float)hc && ix > -1.0f && ix < (float)wc;
  if (!ok) {
    t.nw = t.ne = t.sw = t.se = 0.0f;
    t.x0 = t.y0 = t.x1 = t.y1 = 0;
    t.vx0 = t.vx1 = t.vy0 = t.vy1 = false;
    return t;
  }
  const float fx = floorf(ix), fy = floorf(iy);
  const float w = ix - fx, e = 1.0f - w, n = iy - fy, s = 1.0f - n;
  t.nw = s * e;
  t.ne = s * w;
  t.sw = n * e;
  t.se = n * w;
  t.x0 = (int)fx;
  t.y0 = (int)fy;
  t.x1 = t.x0 + 1;
  t.y1 = t.y0 + 1;
  t.vx0 = t.x0 >= 0 && t.x0 < wc;
  t.vx1 = t.x1 >= 0 && t.x1 < wc;
  t.vy0 = t.y0 >= 0 && t.y0 < hc;
  t.vy1 = t.y1 >= 0 && t.y1 < hc;
  return t;
}

struct SubpixArgs {
  const float* score;  // [B,Hp,Wp] (REFINE)
  int Hp, Wp, h0, w0, xy;
  const int32_t* indices;  // [B,cap] (REFINE)
  const int32_t* counts;   // [B]
  int cap;
  float* positions;  // REFINE: [B,cap,3], columns 0 and 1 rewritten; otherwise read, [B,cap,pos_stride]
  int pos_stride;
  const float* raw;  // [B,D,hc,wc], or [B,hc*wc,D] with CL (BILINEAR)
  int D, hc, wc;
  float scale;
  float* out;  // [B,cap,D] (BILINEAR)
};

// REFINE: the keypoint's position comes from its flat index and the parabola offsets and is written back; otherwise it is read.
// BILINEAR: the keypoint's descriptor row is (re)sampled at that position.
template <bool REFINE, bool BILINEAR, bool CL>
__global__ __launch_bounds__(256) void refine_describe_kernel(const SubpixArgs a) {
  const int b = blockIdx.y;
  const int kp = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  int cnt = a.counts[b];
  cnt = cnt < a.cap ? cnt : a.cap;
  if (kp >= cnt) return;
  float posy, posx;  // padded frame
  if (REFINE) {
    const int fi = a.indices[(size_t)b * a.cap + kp];
    if ((unsigned)fi >= (unsigned)(a.Hp * a.Wp)) return;  // not an index of this map: nothing is read or written for it
    const int y = fi / a.Wp, x = fi % a.Wp;
    const float* s = a.score + (size_t)b * a.Hp * a.Wp;  // wave-uniform addresses
    const float c = s[fi];
    float dy = 0.0f, dx = 0.0f;
    if (x > 0 && x < a.Wp - 1) dx = subpixel_offset(s[fi - 1], c, s[fi + 1]);
    if (y > 0 && y < a.Hp - 1) dy = subpixel_offset(s[fi - a.Wp], c, s[fi + a.Wp]);
    posy = ((float)y + 0.5f) + dy;
    posx = ((float)x + 0.5f) + dx;
    if (lane == 0) {
      const float oy = posy - (float)a.h0, ox = posx - (float)a.w0;
      float* o = a.positions + ((size_t)b * a.cap + kp) * 3;
      o[0] = a.xy ? ox : oy;
      o[1] = a.xy ? oy : ox;
    }
  } else {
    const float* p = a.positions + ((size_t)b * a.cap + kp) * a.pos_stride;
    posy = a.xy ? p[1] : p[0];
    posx = a.xy ? p[0] : p[1];
  }
  if (!BILINEAR) return;
  const SubpixTaps t = subpixel_taps(posy, posx, a.hc, a.wc, a.Hp, a.Wp);
  const int D = a.D, wc = a.wc;
  const size_t plane = (size_t)a.hc * wc;
  const float* rb = a.raw + (size_t)b * D * plane;
  float vals[8];  // D <= 512
  float part = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + 64 * i;
    float v = 0.0f;
    if (c < D) {
      float ta, tb, tc, td;
      if (CL) {
        ta = (t.vy0 && t.vx0) ? rb[(size_t)(t.y0 * wc + t.x0) * D + c] : 0.0f;
        tb = (t.vy0 && t.vx1) ? rb[(size_t)(t.y0 * wc + t.x1) * D + c] : 0.0f;
        tc = (t.vy1 && t.vx0) ? rb[(size_t)(t.y1 * wc + t.x0) * D + c] : 0.0f;
        td = (t.vy1 && t.vx1) ? rb[(size_t)(t.y1 * wc + t.x1) * D + c] : 0.0f;
      } else {
        const float* p = rb + (size_t)c * plane;
        ta = (t.vy0 && t.vx0) ? p[t.y0 * wc + t.x0] : 0.0f;
        tb = (t.vy0 && t.vx1) ? p[t.y0 * wc + t.x1] : 0.0f;
        tc = (t.vy1 && t.vx0) ? p[t.y1 * wc + t.x0] : 0.0f;
        td = (t.vy1 && t.vx1) ? p[t.y1 * wc + t.x1] : 0.0f;
      }
      v = ta * t.nw;
      v = v + tb * t.ne;
      v = v + tc * t.sw;
      v = v + td * t.se;
      part = fmaf(v, v, part);
    }
    vals[i] = v;
  }
  const float nrm = sqrtf(wave_butterfly_sum(part));
  const float den = fmaxf(nrm, 1e-12f);
  float* o = a.out + ((size_t)b * a.cap + kp) * D;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + 64 * i;
    if (c < D) o[c] = a.scale * (vals[i] / den);
  }
}

}  // namespace

EINX_EXPORT int einx_refine_keypoints(const float* score, int B, int Hp, int Wp, int H, int W, int h0, int w0, int ordering_xy,
                                      const int32_t* indices, const int32_t* counts, int cap, float* positions, const float* raw, int D, int hc,
                                      int wc, int bilinear, int channels_last, float scale, float* sparse_desc, void* stream) {
  EINX_CHECK_ARG(score && indices && counts && positions, "null pointer");
  EINX_CHECK_ARG(B > 0 && B < 65536 && Hp > 0 && Wp > 0 && H > 0 && W > 0 && cap > 0, "bad shape");
  EINX_CHECK_ARG(Hp <= SUBPIX_MAX_SIDE && Wp <= SUBPIX_MAX_SIDE, "map sides above 8192 are refused (the offset clamp keeps floor() on the detected pixel only up to there)");
  EINX_CHECK_ARG(h0 >= 0 && w0 >= 0 && h0 + H <= Hp && w0 + W <= Wp, "crop window outside the padded map");
  EINX_CHECK_ARG(!channels_last || bilinear, "the channels-last layout is implemented for bilinear sampling");
  if (bilinear) {
    EINX_CHECK_ARG(raw && sparse_desc, "null pointer (bilinear resampling needs the raw map and the descriptor rows)");
    EINX_CHECK_ARG(D > 0 && D <= 512 && hc > 0 && wc > 0, "bad shape (D must be <= 512)");
  }
  SubpixArgs a{score, Hp, Wp, h0, w0, ordering_xy ? 1 : 0, indices, counts, cap, positions, 3, raw, D, hc, wc, scale, sparse_desc};
  const dim3 grid((unsigned)einx_cdiv(cap, 4), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  EINX_PROF("refine_describe_kernel", s);
  if (bilinear && channels_last)
    hipLaunchKernelGGL((refine_describe_kernel<true, true, true>), grid, dim3(256), 0, s, a);
  else if (bilinear)
    hipLaunchKernelGGL((refine_describe_kernel<true, true, false>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((refine_describe_kernel<true, false, false>), grid, dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_desc_sample_pos(const float* raw, int B, int D, int hc, int wc, int Hp, int Wp, int channels_last, const float* positions,
                                     int pos_stride, int ordering_xy, const int32_t* counts, int cap, float scale, float* out, void* stream) {
  EINX_CHECK_ARG(raw && positions && counts && out, "null pointer");
  EINX_CHECK_ARG(B > 0 && B < 65536 && D > 0 && D <= 512 && hc > 0 && wc > 0 && Hp > 0 && Wp > 0 && cap > 0, "bad shape (D must be <= 512)");
  EINX_CHECK_ARG(pos_stride >= 2, "a position row holds at least two coordinates");
  SubpixArgs a{nullptr, Hp, Wp, 0, 0, ordering_xy ? 1 : 0, nullptr, counts, cap, const_cast<float*>(positions), pos_stride, raw, D, hc, wc, scale, out};
  const dim3 grid((unsigned)einx_cdiv(cap, 4), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  EINX_PROF("desc_sample_pos_kernel", s);
  if (channels_last)
    hipLaunchKernelGGL((refine_describe_kernel<false, true, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((refine_describe_kernel<false, true, false>), grid, dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
