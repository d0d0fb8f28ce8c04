// upsample.h -- what the dense descriptor kernels share: the geometry of upsample_descriptors + normalize (sweeps of up to UP_ROWS
// output rows between the same two coarse rows), the LDS staging of the coarse rows, the per-pixel norm pass and the correctly
// rounded division.  desc.hip writes the map with them (einx_upsample_normalize); loss.hip forms the same elements in registers
// and reduces them (einx_desc_loss), so the two cannot drift apart.
#pragma once
#include "einx_common.h"

namespace {

constexpr int UP_ROWS = 8;               // rows per sweep: a band of the usual 1/8 scale (the first band takes two sweeps)
constexpr int UPS_CC = 32;  // channels per workgroup of the store kernel: 64 (channel, row) pairs = 16 per wave
constexpr int UPS_WAVES = 4;
constexpr int UP_PAIRS = 16;  // (channel, coarse row) pairs a wave of the store kernel stages (once)
constexpr int UPD_PAIRS = 8;  // ... and a wave of the den kernel per round (registers: five of its workgroups per CU)

constexpr int UP_MAX_EXTRA = 8;
struct UpGeom {
  int D, hc, wc, Hp, Wp, h0, w0, H, W;
  int units;  // hc first sweeps + n_extra further sweeps of bands taller than UP_ROWS (band 0 at the shipped size)
  int n_extra;
  short extra_j[UP_MAX_EXTRA], extra_s[UP_MAX_EXTRA];
};

__host__ __device__ inline int up_coarse_row(const UpGeom& g, int Y, float& ly) {  // y0 and the vertical weight of padded row Y
  const float sy = (float)g.hc / (float)g.Hp;
  float fy = ((float)Y + 0.5f) * sy - 0.5f;
  if (fy < 0.0f) fy = 0.0f;
  const int y0 = (int)fy;
  ly = fy - (float)y0;
  return y0;
}
// first padded row (>= h0) whose source row is j; rows are monotone in y0, band 0 also owns the rows clamped to source row 0
__device__ __forceinline__ int up_band_start(const UpGeom& g, int j) {
  const float sy = (float)g.hc / (float)g.Hp;
  int Y = j == 0 ? g.h0 : (int)(((float)j + 0.5f) / sy - 0.5f) - 2;
  if (Y < g.h0) Y = g.h0;
  float t;
  while (Y < g.h0 + g.H && up_coarse_row(g, Y, t) < j) ++Y;
  return Y;
}
// rows of sweep s of band j: first row Y, count nrow (0: nothing to do), vertical weights
__device__ __forceinline__ int up_sweep(const UpGeom& g, int j, int s, int& Y, float* ly, float* hy) {
  Y = up_band_start(g, j) + s * UP_ROWS;
  int nrow = 0;
#pragma unroll
  for (int r = 0; r < UP_ROWS; ++r) {
    float l = 0.0f;
    const bool in = Y + r < g.h0 + g.H && up_coarse_row(g, Y + r, l) == j && nrow == r;
    if (in) nrow = r + 1;
    ly[r] = l;
    hy[r] = 1.0f - l;
  }
  return nrow;
}
__device__ __forceinline__ void up_unit(const UpGeom& g, int unit, int& j, int& s) {
  j = unit;
  s = 0;
  if (unit >= g.hc) {
#pragma unroll
    for (int e = 0; e < UP_MAX_EXTRA; ++e)  // constant indices: the arrays stay in SGPRs
      if (e == unit - g.hc) {
        j = g.extra_j[e];
        s = g.extra_s[e];
      }
  }
}
__device__ __forceinline__ void up_column(const UpGeom& g, int x, int& x0, float& lx, float& hx) {
  const float sx = (float)g.wc / (float)g.Wp;
  float fx = ((float)(x + g.w0) + 0.5f) * sx - 0.5f;
  if (fx < 0.0f) fx = 0.0f;
  x0 = (int)fx;
  lx = fx - (float)x0;
  hx = 1.0f - lx;
}
// Coarse rows j and y1 of channels [c0, c0 + n) -> LDS [n][2][wc + 1] (wc + 1 <= 64); element wc repeats element wc - 1, so
// that the right neighbour x1 = min(x0 + 1, wc - 1) is always the word after x0.  (channel, row) pairs are dealt to the
// waves (at most UP_PAIRS each), lane = x: coalesced row reads, no index divisions, all of a wave's loads in flight at once;
// split in issue / commit so that a round's loads can fly under the previous round's arithmetic.
template <int PAIRS>
struct UpStage {
  float v[PAIRS];
};
template <int PAIRS>
__device__ __forceinline__ void up_stage_issue(UpStage<PAIRS>& st, const float* rb, const UpGeom& g, int j, int y1, int c0, int n, int lane, int wv, int nw) {
  const unsigned plane = (unsigned)(g.hc * g.wc);
  const int np = 2 * n;
  // 32-bit element offsets from one uniform base: the loads address as scalar base + vector offset
  const float* base = rb + (size_t)c0 * plane + (size_t)j * g.wc;
  const unsigned lo = (unsigned)(lane < g.wc ? lane : g.wc - 1);
  const unsigned d1 = (unsigned)((y1 - j) * g.wc);
#pragma unroll
  for (int u = 0; u < PAIRS; ++u) {
    const int q = wv + u * nw;
    const int qc = q < np ? q : np - 1;
    st.v[u] = base[(unsigned)(qc >> 1) * plane + ((qc & 1) ? d1 : 0u) + lo];
  }
}
template <int PAIRS>
__device__ __forceinline__ void up_stage_commit(const UpStage<PAIRS>& st, const UpGeom& g, int n, float* rows, int lane, int wv, int nw) {
  const int pw = g.wc + 1;
  if (lane < pw) {
#pragma unroll
    for (int u = 0; u < PAIRS; ++u) {
      const int q = wv + u * nw;
      if (q < 2 * n) rows[q * pw + lane] = st.v[u];
    }
  }
}

// ws layout: den [B,H,W] then 1/den [B,H,W] (the reciprocal correctly rounded: IEEE division)
// NW waves per workgroup; blockIdx.z walks the column blocks of 64 NW (two half-width workgroups per sweep at W = 346:
// twice as many, half as long workgroups load the CUs more evenly than 34 x B whole-row ones)
template <int NW>
__global__ __launch_bounds__(64 * NW, 8) void upsample_den_kernel(const float* raw, UpGeom g, float* den, float* rden) {
  constexpr int NIT = NW;
  constexpr int CHR = UPD_PAIRS * NIT / 2;  // channels per LDS round: every wave stages UPD_PAIRS (channel, row) pairs
  extern __shared__ float rows[];          // [CHR][2][wc + 1]
  const int b = blockIdx.y;
  int j, s;
  up_unit(g, blockIdx.x, j, s);
  float ly[UP_ROWS], hy[UP_ROWS], ssq[UP_ROWS];
  int Y;
  const int nrow = up_sweep(g, j, s, Y, ly, hy);
  if (nrow == 0) return;  // uniform (a band without rows in the crop window)
  const int tid = threadIdx.x, x = (int)blockIdx.z * 64 * NW + tid, lane = tid & 63, wv = tid >> 6;
  const bool xv = x < g.W;
  const int pw = g.wc + 1;
  int x0;
  float lx, hx;
  up_column(g, xv ? x : g.W - 1, x0, lx, hx);
  const int y1 = j + (j < g.hc - 1 ? 1 : 0);
  const float* rb = raw + (size_t)b * g.D * g.hc * g.wc;
#pragma unroll
  for (int r = 0; r < UP_ROWS; ++r) ssq[r] = 0.0f;
  for (int c0 = 0; c0 < g.D; c0 += CHR) {
    const int n = g.D - c0 < CHR ? g.D - c0 : CHR;
    // the staging registers are not kept across the arithmetic: with <= 64 registers five of these workgroups share a CU and
    // hide each other's load latency (a register prefetch across the loop cost two of them: 217 -> 307 us at B=32)
    UpStage<UPD_PAIRS> st;
    up_stage_issue(st, rb, g, j, y1, c0, n, lane, wv, NIT);
    __syncthreads();  // the previous round's reads are done
    up_stage_commit(st, g, n, rows, lane, wv, NIT);
    __syncthreads();
    const float* rp = rows + x0;
#pragma unroll 1  // (2 / 4 measured the same)
    for (int cl = 0; cl < n; ++cl, rp += 2 * pw) {
      const float t0 = hx * rp[0] + lx * rp[1];
      const float t1 = hx * rp[pw] + lx * rp[pw + 1];
#pragma unroll
      for (int r = 0; r < UP_ROWS; ++r) {
        const float v = hy[r] * t0 + ly[r] * t1;
        ssq[r] = fmaf(v, v, ssq[r]);
      }
    }
  }
  if (xv) {
    const size_t o = ((size_t)b * g.H + (Y - g.h0)) * g.W + x;
#pragma unroll
    for (int r = 0; r < UP_ROWS; ++r)
      if (r < nrow) {
        const float d = fmaxf(sqrtf(ssq[r]), 1e-12f);
        den[o + (size_t)r * g.W] = d;
        rden[o + (size_t)r * g.W] = 1.0f / d;
      }
  }
}

// v / d for the store kernel.  d >= 1e-12 and y = RN(1 / d) come from the den kernel.  Two Newton corrections of
// q = v * y with exact fma remainders give the correctly rounded quotient (after the first step q is faithful, then
// Markstein's theorem applies) as long as nothing under- or overflows and the quotient is a normal number: the kernel
// takes this path for 2^-80 <= |v| <= d < 2^20 only (|q| >= 2^-100).  Checked against IEEE division on 2.5e9 random and boundary-mantissa operands (tools/div_check.c).  Elements
// outside that range (exact zeros among them) make the wave redo the channel with IEEE divisions.
__device__ __forceinline__ float up_div(float v, float d, float y) {
  const float q0 = v * y;
  const float r0 = fmaf(-d, q0, v);
  const float q1 = fmaf(r0, y, q0);
  const float r1 = fmaf(-d, q1, v);
  return fmaf(r1, y, q1);
}

// lists the sweeps beyond the first of every band (the same float arithmetic as the kernels: IEEE, no contraction);
// false if there are more than UP_MAX_EXTRA of them (unusual scales: the band kernel handles those)
static bool up_plan_units(UpGeom& g) {
  g.n_extra = 0;
  for (int e = 0; e < UP_MAX_EXTRA; ++e) g.extra_j[e] = g.extra_s[e] = 0;
  int run = 0, prev = -1;
  for (int Y = g.h0; Y < g.h0 + g.H; ++Y) {
    float l;
    const int y0 = up_coarse_row(g, Y, l);
    run = y0 == prev ? run + 1 : 1;
    prev = y0;
    if (run > UP_ROWS && (run - 1) % UP_ROWS == 0) {  // row number UP_ROWS k + 1 of this band opens sweep k
      if (g.n_extra == UP_MAX_EXTRA) return false;
      g.extra_j[g.n_extra] = (short)y0;
      g.extra_s[g.n_extra] = (short)((run - 1) / UP_ROWS);
      ++g.n_extra;
    }
  }
  g.units = g.hc + g.n_extra;
  return true;
}

// the two-kernel path (the shipped geometries) applies: fills g.units / g.extra_*.  The dynamic LDS of the store kernel (four
// wave slabs + the staged coarse rows) must stay within the 64 KB a launch gets without hipFuncSetAttribute
static bool up_two_kernel_geometry(UpGeom& g) {
  const size_t store_lds = ((size_t)UPS_WAVES * (UP_ROWS * 64 * einx_cdiv(g.W, 64) + 4) + (size_t)UPS_CC * 2 * (g.wc + 1)) * sizeof(float);
  return g.W <= 384 && g.wc <= 63 && g.hc < 32768 && store_lds <= 65536 && up_plan_units(g);
}

constexpr int up_den_waves(int NIT) { return NIT >= 4 ? (NIT + 1) / 2 : NIT; }  // waves per den workgroup

template <int NIT>
static void up_launch_den(const float* raw, int B, const UpGeom& g, float* den, hipStream_t s) {
  float* rden = den + (size_t)B * g.H * g.W;
  EINX_PROF("upsample_den_kernel", s);
  constexpr int NWD = up_den_waves(NIT);
  hipLaunchKernelGGL(upsample_den_kernel<NWD>, dim3((unsigned)g.units, (unsigned)B, (unsigned)einx_cdiv(g.W, 64 * NWD)), dim3(64 * NWD),
                     (size_t)(UPD_PAIRS * NWD / 2) * 2 * (g.wc + 1) * sizeof(float), s, raw, g, den, rden);
}

}  // namespace
