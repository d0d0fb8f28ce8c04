// loss.hip -- forward values of the extractor losses on gfx950 (validation under no_grad; no autograd).
//
// Replaces (reference file:line): core/loss/extractor_loss.py:6-69 (ScoreLoss), :72-143 (LogitsLoss), :146-354 (DescriptorsLoss,
// modes mse / mae / cosine_similarity) and :357-383 (FeatureLoss).  Every op writes one (sum, count) pair of float64 per image,
// out [B,2]: a loss value is weight * sum_b(sum) / sum_b(count), a per-pair value weight * sum_b / count_b.
//
//   einx_desc_loss   DescriptorsLoss on `normalized_descriptors` WITHOUT the two [B,D,H,W] maps (2.95 GB each at B = 32): every
//                    element is a function of the coarse raw map, so it is formed in registers exactly as einx_upsample_normalize
//                    (cell 8) / einx_normalize_map + crop (cell 1) would have stored it (bit for bit: same operations, same order,
//                    same correctly rounded division) and goes straight into the reduction.
//   einx_map_loss    masked pair reduction over tensors that exist ([B,C,P]; scores, features, raw / coarse descriptors, resolved maps)
//   einx_logits_loss the same over the pixel-shuffled, cropped detector logits
//
// Reductions: every term is added in float64, per lane; a workgroup adds its lanes in a fixed order and writes one partial pair
// to the workspace, one workgroup per image adds the partials in a fixed order.  No atomics: bit-identical run to run.
#include "einx_common.h"
#include "upsample.h"

namespace {

__device__ __forceinline__ double mask_weight(const void* mask, int type, size_t i) {
  if (type == EINX_MASK_U8) return ((const uint8_t*)mask)[i] ? 1.0 : 0.0;
  if (type == EINX_MASK_F32) return (double)((const float*)mask)[i];
  return 1.0;
}

// (s, c) of every thread of the workgroup -> dst[0..1]: lane l of wave 0 adds the entries l, l + 64, ... in order, then the xor
// butterfly (every lane forms the same sums).  red: 2 * blockDim.x doubles of LDS.
__device__ __forceinline__ void block_pair_store(double s, double c, double* red, double* dst) {
  const int tid = threadIdx.x, n = blockDim.x;
  red[tid] = s;
  red[n + tid] = c;
  __syncthreads();
  if (tid < 64) {
    double a = 0.0, b = 0.0;
    for (int i = tid; i < n; i += 64) {
      a += red[i];
      b += red[n + i];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off, 64);
      b += __shfl_xor(b, off, 64);
    }
    if (tid == 0) {
      dst[0] = a;
      dst[1] = b;
    }
  }
}

// one workgroup per image: its nparts partial pairs, added in a fixed order -> out[b][0..1]
__global__ __launch_bounds__(256) void loss_finish_kernel(const double* part, int nparts, double* out) {
  __shared__ double red[2 * 256];
  const int b = blockIdx.x;
  const double* p = part + (size_t)b * nparts * 2;
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) {
    s += p[2 * i];
    c += p[2 * i + 1];
  }
  block_pair_store(s, c, red, out + (size_t)b * 2);
}

// ---- DescriptorsLoss, desc_type "normalized", cell 8 --------------------------------------------------------------------------
// Built like upsample_den_kernel: (sweep, image, block of 64 NW columns) per workgroup, one column per lane, the coarse rows
// (j, y1) of 4 NW channels of BOTH sides staged in LDS per round, the horizontal lerps of a channel shared by the rows of the
// sweep.  Element a of the event map and b of the image map: scale * RN(v / den) with den from upsample_den_kernel (run once
// per side before this kernel), the division as in upsample_store_kernel (up_div, IEEE divisions for a channel with an element
// outside its range).  The float64 additions (one per element, three for COS) sit after the fp32 chain of an element, per row
// of the sweep, so the mask weight is applied once per pixel.
template <int NW, int MODE>
__global__ __launch_bounds__(64 * NW) void desc_loss_kernel(const float* raw_a, const float* raw_b, const float* den_a, const float* rden_a,
                                                            const float* den_b, const float* rden_b, UpGeom g, float scale_a, float scale_b,
                                                            const void* mask, int mask_type, double* part) {
  constexpr int CHR = UPD_PAIRS * NW / 2;  // channels per LDS round: every wave stages UPD_PAIRS (channel, row) pairs per side
  constexpr int NACC = MODE == EINX_LOSS_COS ? 3 : 1, IA = NACC > 1 ? 1 : 0, IB = NACC > 1 ? 2 : 0;
  extern __shared__ float rows[];  // [2][CHR][2][wc + 1]
  __shared__ double red[2 * 64 * NW];
  const int b = blockIdx.y;
  double* dst = part + (((size_t)b * gridDim.x + blockIdx.x) * gridDim.z + blockIdx.z) * 2;
  int j, s;
  up_unit(g, blockIdx.x, j, s);
  float ly[UP_ROWS], hy[UP_ROWS];
  int Y;
  const int nrow = up_sweep(g, j, s, Y, ly, hy);
  if (nrow == 0) {  // uniform (a band without rows in the crop window): an empty partial
    if (threadIdx.x == 0) dst[0] = dst[1] = 0.0;
    return;
  }
  const int tid = threadIdx.x, x = (int)blockIdx.z * 64 * NW + tid, lane = tid & 63, wv = tid >> 6;
  const bool xv = x < g.W;
  const int xc = xv ? x : g.W - 1;
  const int pw = g.wc + 1;
  int x0;
  float lx, hx;
  up_column(g, xc, x0, lx, hx);
  const int y1 = j + (j < g.hc - 1 ? 1 : 0);
  const size_t img = (size_t)b * g.D * g.hc * g.wc;
  const float *ra = raw_a + img, *rb = raw_b + img;
  float* rows_a = rows;
  float* rows_b = rows + CHR * 2 * pw;
  // per-pixel norms of the sweep; rows past nrow / columns past W re-read a valid pixel's norm and are dropped at the end
  float da[UP_ROWS], ya[UP_ROWS], db[UP_ROWS], yb[UP_ROWS];
  bool big = false;  // a norm beyond the fast division's range: IEEE divisions for the whole sweep
#pragma unroll
  for (int r = 0; r < UP_ROWS; ++r) {
    const size_t o = ((size_t)b * g.H + (Y - g.h0 + (r < nrow ? r : nrow - 1))) * g.W + xc;
    da[r] = den_a[o];
    ya[r] = rden_a[o];
    db[r] = den_b[o];
    yb[r] = rden_b[o];
    big |= !(da[r] < 0x1p20f) || !(db[r] < 0x1p20f);
  }
  big = __any(big);
  double acc[NACC][UP_ROWS];
#pragma unroll
  for (int k = 0; k < NACC; ++k)
#pragma unroll
    for (int r = 0; r < UP_ROWS; ++r) acc[k][r] = 0.0;
  for (int c0 = 0; c0 < g.D; c0 += CHR) {
    const int n = g.D - c0 < CHR ? g.D - c0 : CHR;
    {
      UpStage<UPD_PAIRS> sa, sb;
      up_stage_issue(sa, ra, g, j, y1, c0, n, lane, wv, NW);
      up_stage_issue(sb, rb, g, j, y1, c0, n, lane, wv, NW);
      __syncthreads();  // the previous round's reads are done
      up_stage_commit(sa, g, n, rows_a, lane, wv, NW);
      up_stage_commit(sb, g, n, rows_b, lane, wv, NW);
    }
    __syncthreads();
    const float* pa = rows_a + x0;
    const float* pb = rows_b + x0;
#pragma unroll 1
    for (int cl = 0; cl < n; ++cl, pa += 2 * pw, pb += 2 * pw) {
      const float ta0 = hx * pa[0] + lx * pa[1];
      const float ta1 = hx * pa[pw] + lx * pa[pw + 1];
      const float tb0 = hx * pb[0] + lx * pb[1];
      const float tb1 = hx * pb[pw] + lx * pb[pw + 1];
      float qa[UP_ROWS], qb[UP_ROWS];
      float vmin = 0x1p20f;  // lower end of the fast division's range, tested once per channel
#pragma unroll
      for (int r = 0; r < UP_ROWS; ++r) {
        const float va = hy[r] * ta0 + ly[r] * ta1;
        const float vb = hy[r] * tb0 + ly[r] * tb1;
        vmin = fminf(vmin, fminf(fabsf(va), fabsf(vb)));
        qa[r] = scale_a * up_div(va, da[r], ya[r]);
        qb[r] = scale_b * up_div(vb, db[r], yb[r]);
      }
      if (__builtin_expect(__any(big || !(vmin >= 0x1p-80f)), 0)) {  // the same values with IEEE divisions
#pragma unroll
        for (int r = 0; r < UP_ROWS; ++r) {
          qa[r] = scale_a * ((hy[r] * ta0 + ly[r] * ta1) / da[r]);
          qb[r] = scale_b * ((hy[r] * tb0 + ly[r] * tb1) / db[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < UP_ROWS; ++r) {
        if (MODE == EINX_LOSS_COS) {
          const double a = (double)qa[r], bb = (double)qb[r];
          acc[0][r] += a * bb;
          acc[IA][r] += a * a;
          acc[IB][r] += bb * bb;
        } else if (MODE == EINX_LOSS_MSE) {
          const float d = qa[r] - qb[r];
          acc[0][r] += (double)(d * d);
        } else {
          acc[0][r] += (double)fabsf(qa[r] - qb[r]);
        }
      }
    }
  }
  double sum = 0.0, cnt = 0.0;
  if (xv) {
#pragma unroll
    for (int r = 0; r < UP_ROWS; ++r)
      if (r < nrow) {
        const size_t pix = ((size_t)b * g.H + (Y - g.h0 + r)) * g.W + x;
        const double w = mask_weight(mask, mask_type, pix);
        if (MODE == EINX_LOSS_COS) {
          const double t = acc[0][r] / (fmax(sqrt(acc[IA][r]), 1e-8) * fmax(sqrt(acc[IB][r]), 1e-8));
          sum += w * t;
          cnt += w;
        } else {
          sum += w * acc[0][r];
          cnt += w * (double)g.D;
        }
      }
  }
  block_pair_store(sum, cnt, red, dst);
}

// ---- the same for cell 1 (raw maps at the padded full resolution, the normalised map cropped by the pads) -----------------------
// one pixel of the crop window per thread; pass 1: the norm as normalize_map_kernel's sequential fmaf chain c = 0..D-1, pass 2: the terms
template <int MODE>
__global__ __launch_bounds__(256) void desc_loss_cell1_kernel(const float* raw_a, const float* raw_b, int D, int Hp, int Wp, int h0, int w0, int H,
                                                              int W, float scale_a, float scale_b, const void* mask, int mask_type, double* part) {
  __shared__ double red[2 * 256];
  const int b = blockIdx.y;
  const int P = H * W;
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const bool pv = p < P;
  const int pc = pv ? p : P - 1;
  const size_t plane = (size_t)Hp * Wp;
  const size_t off = (size_t)b * D * plane + (size_t)(pc / W + h0) * Wp + (pc % W + w0);
  const float *pa = raw_a + off, *pb = raw_b + off;
  float sa = 0.0f, sb = 0.0f;
  for (int c = 0; c < D; ++c) {
    const float va = pa[(size_t)c * plane], vb = pb[(size_t)c * plane];
    sa = fmaf(va, va, sa);
    sb = fmaf(vb, vb, sb);
  }
  const float da = fmaxf(sqrtf(sa), 1e-12f), db = fmaxf(sqrtf(sb), 1e-12f);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int c = 0; c < D; ++c) {
    const float qa = scale_a * (pa[(size_t)c * plane] / da);
    const float qb = scale_b * (pb[(size_t)c * plane] / db);
    if (MODE == EINX_LOSS_COS) {
      const double a = (double)qa, bb = (double)qb;
      a0 += a * bb;
      a1 += a * a;
      a2 += bb * bb;
    } else if (MODE == EINX_LOSS_MSE) {
      const float d = qa - qb;
      a0 += (double)(d * d);
    } else {
      a0 += (double)fabsf(qa - qb);
    }
  }
  double sum = 0.0, cnt = 0.0;
  if (pv) {
    const double w = mask_weight(mask, mask_type, (size_t)b * P + p);
    if (MODE == EINX_LOSS_COS) {
      sum = w * (a0 / (fmax(sqrt(a1), 1e-8) * fmax(sqrt(a2), 1e-8)));
      cnt = w;
    } else {
      sum = w * a0;
      cnt = w * (double)D;
    }
  }
  block_pair_store(sum, cnt, red, part + ((size_t)b * gridDim.x + blockIdx.x) * 2);
}

// ---- generic pair reduction over existing tensors [B,C,P] ---------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ double map_term(float a, float b) {
  if (MODE == EINX_MAP_SQ) {
    const float d = a - b;
    return (double)(d * d);
  }
  if (MODE == EINX_MAP_ABS) return (double)fabsf(a - b);
  // BCE: a = probability, b = target score (> 0 is a keypoint); the logarithms in double, clamped at -100 like torch
  const double t = b > 0.0f ? 1.0 : 0.0;
  const double lp = fmax(log((double)a), -100.0), lq = fmax(log(1.0 - (double)a), -100.0);
  return -(t * lp + (1.0 - t) * lq);
}

// one position p per thread, channels walked in order.  mask: [B,P] (broadcast over the channels: weight applied once per
// position, count = C * weight) or, with mask_full, [B,C,P].  COS: cosine over the channels per position, count = weight.
template <int MODE>
__global__ __launch_bounds__(256) void map_loss_kernel(const float* x, const float* y, int C, int P, const void* mask, int mask_type, int mask_full,
                                                       double* part) {
  __shared__ double red[2 * 256];
  const int b = blockIdx.y;
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  double sum = 0.0, cnt = 0.0;
  if (p < P) {
    const size_t base = (size_t)b * C * P + p;
    const float *xp = x + base, *yp = y + base;
    if (MODE == EINX_MAP_COS) {
      double d = 0.0, aa = 0.0, bb = 0.0;
      for (int c = 0; c < C; ++c) {
        const double a = (double)xp[(size_t)c * P], v = (double)yp[(size_t)c * P];
        d += a * v;
        aa += a * a;
        bb += v * v;
      }
      const double w = mask_weight(mask, mask_type, (size_t)b * P + p);
      sum = w * (d / (fmax(sqrt(aa), 1e-8) * fmax(sqrt(bb), 1e-8)));
      cnt = w;
    } else if (mask_full && mask_type != EINX_MASK_NONE) {
      for (int c = 0; c < C; ++c) {
        const double w = mask_weight(mask, mask_type, base + (size_t)c * P);
        sum += w * map_term<MODE>(xp[(size_t)c * P], yp[(size_t)c * P]);
        cnt += w;
      }
    } else {
      double acc = 0.0;
      for (int c = 0; c < C; ++c) acc += map_term<MODE>(xp[(size_t)c * P], yp[(size_t)c * P]);
      const double w = mask_weight(mask, mask_type, (size_t)b * P + p);
      sum = w * acc;
      cnt = w * (double)C;
    }
  }
  block_pair_store(sum, cnt, red, part + ((size_t)b * gridDim.x + blockIdx.x) * 2);
}

// LogitsLoss: channels 0 .. cell^2 - 1 of [B,C,hc,wc]; element (c, yc, xc) is pixel (cell yc + c / cell, cell xc + c % cell) of
// the padded frame (pixel_shuffle), kept when it lies in the crop window [h0, h0 + H) x [w0, w0 + W) and weighted by the mask
// [B,H,W] at its cropped position.  count = elements in the window (the reference's mean runs over all of them, masked or not).
__global__ __launch_bounds__(256) void logits_loss_kernel(const float* x, const float* y, int C, int cell, int hc, int wc, int h0, int w0, int H,
                                                          int W, const void* mask, int mask_type, double* part) {
  __shared__ double red[2 * 256];
  const int b = blockIdx.y;
  const int plane = hc * wc;
  const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
  double sum = 0.0, cnt = 0.0;
  if (q < plane) {
    const int yc = q / wc, xc = q % wc;
    const size_t base = (size_t)b * C * plane + q;
    for (int c = 0; c < cell * cell; ++c) {
      const int py = cell * yc + c / cell - h0, px = cell * xc + c % cell - w0;
      if (py >= 0 && py < H && px >= 0 && px < W) {
        const float d = x[base + (size_t)c * plane] - y[base + (size_t)c * plane];
        sum += mask_weight(mask, mask_type, ((size_t)b * H + py) * W + px) * (double)(d * d);
        cnt += 1.0;
      }
    }
  }
  block_pair_store(sum, cnt, red, part + ((size_t)b * gridDim.x + blockIdx.x) * 2);
}

// ---- workspaces: one carve per op, walked by the size query and by the call -------------------------------------------------------
struct PartWs {
  double* part;  // [B][nblk][2]
  int nblk;
};
PartWs part_carve(WsCarver& c, int B, int positions) {
  PartWs w;
  w.nblk = einx_cdiv(positions, 256);
  w.part = c.take<double>((size_t)B * w.nblk * 2);
  return w;
}

enum { DL_FUSED = 0, DL_CELL1 = 1, DL_MAPS = 2 };
struct DescLossWs {
  int path;
  float *den_a, *den_b;  // DL_FUSED: [2,B,H,W] each (den, 1 / den)
  double* part;          // DL_FUSED: [B][units * column blocks][2]
  int nparts;
  float *map_a, *map_b;  // DL_MAPS: the two materialised maps [B,D,H,W]
  void* up_ws;           // DL_MAPS: einx_upsample_normalize's own
  size_t up_bytes;
  PartWs tail;           // DL_CELL1, DL_MAPS
};
// fills g.units / g.extra_* on the fused path
DescLossWs desc_loss_carve(WsCarver& c, UpGeom& g, int B, int cell) {
  DescLossWs w{};
  const size_t HW = (size_t)g.H * g.W;
  if (cell == 1) {
    w.path = DL_CELL1;
    w.tail = part_carve(c, B, g.H * g.W);
  } else if (up_two_kernel_geometry(g)) {
    w.path = DL_FUSED;
    w.den_a = c.take<float>(2 * B * HW);
    w.den_b = c.take<float>(2 * B * HW);
    w.nparts = g.units * einx_cdiv(g.W, 64 * up_den_waves(einx_cdiv(g.W, 64)));
    w.part = c.take<double>((size_t)B * w.nparts * 2);
  } else {  // the geometries einx_upsample_normalize gives to its band kernel: materialise, then reduce
    w.path = DL_MAPS;
    w.map_a = c.take<float>((size_t)B * g.D * HW);
    w.map_b = c.take<float>((size_t)B * g.D * HW);
    w.up_bytes = einx_upsample_ws_bytes(B, g.H, g.W);
    w.up_ws = c.take<char>(w.up_bytes);
    w.tail = part_carve(c, B, g.H * g.W);
  }
  return w;
}

int finish(const double* part, int nparts, int B, double* out, hipStream_t s) {
  hipLaunchKernelGGL(loss_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, part, nparts, out);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

template <int NIT, int MODE>
void launch_desc_loss(const float* raw_a, float scale_a, const float* raw_b, float scale_b, int B, const UpGeom& g, const DescLossWs& w,
                      const void* mask, int mask_type, hipStream_t s) {
  const size_t n = (size_t)B * g.H * g.W;
  up_launch_den<NIT>(raw_a, B, g, w.den_a, s);
  up_launch_den<NIT>(raw_b, B, g, w.den_b, s);
  EINX_PROF("desc_loss_kernel", s);
  constexpr int NW = up_den_waves(NIT);
  const size_t lds = (size_t)2 * (UPD_PAIRS * NW / 2) * 2 * (g.wc + 1) * sizeof(float);
  hipLaunchKernelGGL((desc_loss_kernel<NW, MODE>), dim3((unsigned)g.units, (unsigned)B, (unsigned)einx_cdiv(g.W, 64 * NW)), dim3(64 * NW), lds, s,
                     raw_a, raw_b, w.den_a, w.den_a + n, w.den_b, w.den_b + n, g, scale_a, scale_b, mask, mask_type, w.part);
}

template <int MODE>
void launch_desc_loss_mode(const float* raw_a, float scale_a, const float* raw_b, float scale_b, int B, const UpGeom& g, const DescLossWs& w,
                           const void* mask, int mask_type, hipStream_t s) {
  switch (einx_cdiv(g.W, 64)) {
    case 1: launch_desc_loss<1, MODE>(raw_a, scale_a, raw_b, scale_b, B, g, w, mask, mask_type, s); break;
    case 2: launch_desc_loss<2, MODE>(raw_a, scale_a, raw_b, scale_b, B, g, w, mask, mask_type, s); break;
    case 3: launch_desc_loss<3, MODE>(raw_a, scale_a, raw_b, scale_b, B, g, w, mask, mask_type, s); break;
    case 4: launch_desc_loss<4, MODE>(raw_a, scale_a, raw_b, scale_b, B, g, w, mask, mask_type, s); break;
    case 5: launch_desc_loss<5, MODE>(raw_a, scale_a, raw_b, scale_b, B, g, w, mask, mask_type, s); break;
    default: launch_desc_loss<6, MODE>(raw_a, scale_a, raw_b, scale_b, B, g, w, mask, mask_type, s); break;
  }
}

void launch_map_loss(const float* x, const float* y, int B, int C, int P, const void* mask, int mask_type, int mask_full, int mode,
                     const PartWs& w, hipStream_t s) {
  EINX_PROF("map_loss_kernel", s);
  const dim3 grid((unsigned)w.nblk, (unsigned)B);
  switch (mode) {
    case EINX_MAP_SQ: hipLaunchKernelGGL(map_loss_kernel<EINX_MAP_SQ>, grid, dim3(256), 0, s, x, y, C, P, mask, mask_type, mask_full, w.part); break;
    case EINX_MAP_ABS: hipLaunchKernelGGL(map_loss_kernel<EINX_MAP_ABS>, grid, dim3(256), 0, s, x, y, C, P, mask, mask_type, mask_full, w.part); break;
    case EINX_MAP_BCE: hipLaunchKernelGGL(map_loss_kernel<EINX_MAP_BCE>, grid, dim3(256), 0, s, x, y, C, P, mask, mask_type, mask_full, w.part); break;
    default: hipLaunchKernelGGL(map_loss_kernel<EINX_MAP_COS>, grid, dim3(256), 0, s, x, y, C, P, mask, mask_type, mask_full, w.part); break;
  }
}

bool mask_args_ok(const void* mask, int mask_type) {
  return mask_type == EINX_MASK_NONE ? mask == nullptr : ((mask_type == EINX_MASK_U8 || mask_type == EINX_MASK_F32) && mask != nullptr);
}

}  // namespace

#define EINX_DESC_LOSS_SHAPE_CHECKS()                                                                                      \
  EINX_CHECK_ARG(B > 0 && D > 0 && hc > 0 && wc > 0 && H > 0 && W > 0, "bad shape");                                     \
  EINX_CHECK_ARG(h0 >= 0 && w0 >= 0 && h0 + H <= Hp && w0 + W <= Wp, "crop window outside the padded map");              \
  EINX_CHECK_ARG(B < 65536, "batch too large");                                                                            \
  EINX_CHECK_ARG(cell == 8 || cell == 1, "cell must be 8 or 1");                                                           \
  EINX_CHECK_ARG(cell != 1 || (hc == Hp && wc == Wp), "cell 1 needs raw maps at the padded resolution");                   \
  EINX_CHECK_ARG((size_t)H * W < ((size_t)1 << 31), "map too large")

EINX_EXPORT size_t einx_desc_loss_ws_bytes(int B, int D, int hc, int wc, int Hp, int Wp, int h0, int w0, int H, int W, int cell) {
  if (B <= 0 || D <= 0 || hc <= 0 || wc <= 0 || H <= 0 || W <= 0 || (cell != 8 && cell != 1)) return 0;
  UpGeom g{D, hc, wc, Hp, Wp, h0, w0, H, W, 0, 0, {0}, {0}};
  WsCarver c{nullptr};
  desc_loss_carve(c, g, B, cell);
  return c.bytes;
}

EINX_EXPORT int einx_desc_loss(const float* raw_a, float scale_a, const float* raw_b, float scale_b, int B, int D, int hc, int wc, int Hp, int Wp,
                               int h0, int w0, int H, int W, int cell, const void* mask, int mask_type, int mode, double* out, void* ws,
                               size_t ws_bytes, void* stream) {
  EINX_CHECK_ARG(raw_a && raw_b && out, "null pointer");
  EINX_DESC_LOSS_SHAPE_CHECKS();
  EINX_CHECK_ARG(mask_args_ok(mask, mask_type), "mask and mask_type disagree");
  EINX_CHECK_ARG(mode == EINX_LOSS_MAE || mode == EINX_LOSS_MSE || mode == EINX_LOSS_COS, "unknown mode");
  EINX_CHECK_ARG(ws && ((size_t)ws & 255) == 0, "workspace missing or not aligned to 256 bytes");
  hipStream_t s = (hipStream_t)stream;
  UpGeom g{D, hc, wc, Hp, Wp, h0, w0, H, W, 0, 0, {0}, {0}};
  WsCarver c{(char*)ws};
  const DescLossWs w = desc_loss_carve(c, g, B, cell);
  EINX_CHECK_ARG(ws_bytes >= c.bytes, "workspace smaller than einx_desc_loss_ws_bytes");
  if (w.path == DL_FUSED) {
    switch (mode) {
      case EINX_LOSS_MAE: launch_desc_loss_mode<EINX_LOSS_MAE>(raw_a, scale_a, raw_b, scale_b, B, g, w, mask, mask_type, s); break;
      case EINX_LOSS_MSE: launch_desc_loss_mode<EINX_LOSS_MSE>(raw_a, scale_a, raw_b, scale_b, B, g, w, mask, mask_type, s); break;
      default: launch_desc_loss_mode<EINX_LOSS_COS>(raw_a, scale_a, raw_b, scale_b, B, g, w, mask, mask_type, s); break;
    }
    EINX_CHECK_LAUNCH();
    return finish(w.part, w.nparts, B, out, s);
  }
  if (w.path == DL_CELL1) {
    EINX_PROF("desc_loss_cell1_kernel", s);
    const dim3 grid((unsigned)w.tail.nblk, (unsigned)B);
    switch (mode) {
      case EINX_LOSS_MAE:
        hipLaunchKernelGGL(desc_loss_cell1_kernel<EINX_LOSS_MAE>, grid, dim3(256), 0, s, raw_a, raw_b, D, Hp, Wp, h0, w0, H, W, scale_a, scale_b, mask, mask_type, w.tail.part);
        break;
      case EINX_LOSS_MSE:
        hipLaunchKernelGGL(desc_loss_cell1_kernel<EINX_LOSS_MSE>, grid, dim3(256), 0, s, raw_a, raw_b, D, Hp, Wp, h0, w0, H, W, scale_a, scale_b, mask, mask_type, w.tail.part);
        break;
      default:
        hipLaunchKernelGGL(desc_loss_cell1_kernel<EINX_LOSS_COS>, grid, dim3(256), 0, s, raw_a, raw_b, D, Hp, Wp, h0, w0, H, W, scale_a, scale_b, mask, mask_type, w.tail.part);
        break;
    }
    EINX_CHECK_LAUNCH();
    return finish(w.tail.part, w.tail.nblk, B, out, s);
  }
  // materialise both maps with the existing kernels, then the generic reduction: same result contract
  int r = einx_upsample_normalize(raw_a, B, D, hc, wc, Hp, Wp, h0, w0, H, W, scale_a, w.map_a, w.up_ws, w.up_bytes, stream);
  if (r != EINX_OK) return r;
  r = einx_upsample_normalize(raw_b, B, D, hc, wc, Hp, Wp, h0, w0, H, W, scale_b, w.map_b, w.up_ws, w.up_bytes, stream);
  if (r != EINX_OK) return r;
  const int map_mode = mode == EINX_LOSS_MAE ? EINX_MAP_ABS : mode == EINX_LOSS_MSE ? EINX_MAP_SQ : EINX_MAP_COS;
  launch_map_loss(w.map_a, w.map_b, B, D, H * W, mask, mask_type, 0, map_mode, w.tail, s);
  EINX_CHECK_LAUNCH();
  return finish(w.tail.part, w.tail.nblk, B, out, s);
}

EINX_EXPORT size_t einx_map_loss_ws_bytes(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  WsCarver c{nullptr};
  part_carve(c, B, P);
  return c.bytes;
}

EINX_EXPORT int einx_map_loss(const float* x, const float* y, int B, int C, int P, const void* mask, int mask_type, int mask_full, int mode,
                              double* out, void* ws, size_t ws_bytes, void* stream) {
  EINX_CHECK_ARG(x && y && out, "null pointer");
  EINX_CHECK_ARG(B > 0 && B < 65536 && C > 0 && P > 0, "bad shape");
  EINX_CHECK_ARG(mask_args_ok(mask, mask_type), "mask and mask_type disagree");
  EINX_CHECK_ARG(mode == EINX_MAP_SQ || mode == EINX_MAP_ABS || mode == EINX_MAP_BCE || mode == EINX_MAP_COS, "unknown mode");
  EINX_CHECK_ARG(!(mode == EINX_MAP_COS && mask_full), "COS takes a [B,P] mask");
  EINX_CHECK_ARG(ws && ((size_t)ws & 255) == 0, "workspace missing or not aligned to 256 bytes");
  WsCarver c{(char*)ws};
  const PartWs w = part_carve(c, B, P);
  EINX_CHECK_ARG(ws_bytes >= c.bytes, "workspace smaller than einx_map_loss_ws_bytes");
  hipStream_t s = (hipStream_t)stream;
  launch_map_loss(x, y, B, C, P, mask, mask_type, mask_full, mode, w, s);
  EINX_CHECK_LAUNCH();
  return finish(w.part, w.nblk, B, out, s);
}

EINX_EXPORT int einx_logits_loss(const float* x, const float* y, int B, int C, int cell, int hc, int wc, int h0, int w0, int H, int W,
                                 const void* mask, int mask_type, double* out, void* ws, size_t ws_bytes, void* stream) {
  EINX_CHECK_ARG(x && y && out, "null pointer");
  EINX_CHECK_ARG(B > 0 && B < 65536 && hc > 0 && wc > 0 && cell > 0 && C >= cell * cell && H > 0 && W > 0, "bad shape");
  EINX_CHECK_ARG((long)cell * hc < (1L << 30) && (long)cell * wc < (1L << 30) && (long)hc * wc < (1L << 31), "map too large");
  EINX_CHECK_ARG(h0 >= 0 && w0 >= 0 && h0 + H <= cell * hc && w0 + W <= cell * wc, "crop window outside the shuffled map");
  EINX_CHECK_ARG(mask_args_ok(mask, mask_type), "mask and mask_type disagree");
  EINX_CHECK_ARG(ws && ((size_t)ws & 255) == 0, "workspace missing or not aligned to 256 bytes");
  WsCarver c{(char*)ws};
  const PartWs w = part_carve(c, B, hc * wc);
  EINX_CHECK_ARG(ws_bytes >= c.bytes, "workspace smaller than einx_map_loss_ws_bytes(B, hc * wc)");
  hipStream_t s = (hipStream_t)stream;
  {
    EINX_PROF("logits_loss_kernel", s);
    hipLaunchKernelGGL(logits_loss_kernel, dim3((unsigned)w.nblk, (unsigned)B), dim3(256), 0, s, x, y, C, cell, hc, wc, h0, w0, H, W, mask, mask_type,
                       w.part);
  }
  EINX_CHECK_LAUNCH();
  return finish(w.part, w.nblk, B, out, s);
}
