// conv_f16.hip -- the conv blocks of conv.hip with binary16 operands on v_mfma_f32_32x32x16_f16 (opt-in).
//
// One kernel = Conv2d(3x3 pad 1 | 1x1) + bias -> [ReLU] -> [BN(eval) affine] -> [MaxPool 2x2] for layers with cin % 8 == 0:
//   every input activation and every weight is rounded to binary16 (round to nearest even, overflow to infinity: tensor.half()),
//   the products are exact in fp32 and accumulated in fp32 (in the instruction's order: the freedom the contract takes), and the
//   epilogue is conv_block_kernel's, operation for operation, in fp32.  Activations stay fp32 NCHW in HBM on both sides.
// Implicit GEMM: M = output channels (A = weights, 64 per workgroup), N = the 256 pixels of a TH x TW tile on the MFMA column
// (= lane) index (NCHW stores stay 128-byte coalesced), K = (chunk of CK input channels, tap, channel inside the chunk).  A lane's
// 8-element fragment is 8 consecutive input channels of one halo position at one tap (B) or of one output channel at one tap (A):
// ONE 16-byte LDS read each.
//
// LDS images and their pitch.  Input: position-major, channel-innermost [halo position][CK halves + 8]; weights: [output channel]
// [TAPS CK halves + 8].  A 32-lane N-tile is one tile row (TW == 32) or a flat run (1x1), so the lanes j = 0..31 of a fragment read
// sit on 32 CONSECUTIVE positions (rows) at the same tap, lanes 32..63 eight halves further along the same rows.  ds_read_b128 is
// served in four groups of 16 lanes -- {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same +32 -- over 64 banks of 4 bytes; the row
// numbers of a group are, mod 16, every residue once.  With a pitch of P dwords per row, row r starts on the 4-bank slot
// (r P / 4) mod 16, so the 16 reads of a group cover the 64 banks exactly once iff P / 4 is odd:
//   3x3, CK 16: 24 halves = 12 dwords (4 x 3) per position, 152 halves = 76 dwords (4 x 19) per weight row;
//   1x1, CK 64: 72 halves = 36 dwords (4 x 9) for both.
// (8l's pitch of 40 halves = 20 dwords is the same rule.)  The staging stores are 16-byte ds_write_b128 (groups of 8 consecutive
// lanes over 32 banks): 8 consecutive positions at 12 dwords start on the banks 0, 12, 24, 4, 16, 28, 8, 20 -- once each.
// Derived from the documented banking; NOT confirmed with an LDS bank-conflict counter run.
//
// Staging follows conv_block_kernel: a thread owns ONE halo position and brings in that position of the chunk's channels from the
// fp32 NCHW planes through a buffer descriptor that spans the channels that exist (channels past cin load as 0), converts with
// v_cvt_f16_f32 / v_cvt_pk_f16_f32 (nearest even, never the round-toward-zero pack convert) and writes 16-byte LDS stores;
// positions outside the image are zeroed once.  The next chunk's global loads are issued before the current chunk's MFMAs.
// The binary16 weight image (einx_conv_repack_f16) is [cout tile][chunk][64 output channels][tap][CK channels], zero-filled past
// cin and cout, so a workgroup's chunk is one contiguous block.  65 output channels (the detector) are padded to 128.
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "einx_common.h"

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

constexpr int kCoutTile = 64;  // output channels per workgroup
constexpr int kThreads = 512;  // 8 waves: 2 channel groups x 4 pixel groups, a wave owns 32 channels x 64 pixels

constexpr int conv_f16_ck(int ks) { return ks == 1 ? 64 : 16; }  // input channels per LDS round (part of the weight image's layout)

struct ConvF16Args {
  const float* in;
  const _Float16* w;  // binary16 image
  const float* bias;
  const float* scale;
  const float* shift;
  float* out;
  int B, Cin, Cout, CoutPad;
  int H, W;
  int tilesX, tilesY, nchunks;
  int relu;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t f16_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

// max(v, v of lane ^ 1): DPP quad_perm [1,0,3,2]
__device__ __forceinline__ float max_lane_xor1(float v) {
  const int i = __builtin_bit_cast(int, v);
  return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, i, 0xB1, 0xF, 0xF, true)));
}

// channel groups among the staging threads: the most groups of `npos` threads that fit and split the chunk into runs of 8 channels
constexpr int f16_stage_groups(int npos, int ck) {
  int ng = kThreads / npos;
  while (ng > 1 && (ck / 8) % ng != 0) --ng;
  return ng < 1 ? 1 : ng;
}

// KS: 1|3.  TH x TW: spatial tile of 256 pixels (KS == 1: a flat run).  CK: input channels per LDS round.  POOL: fuse MaxPool2d(2,2).
template <int KS, int TH, int TW, int CK, bool POOL>
__global__ __launch_bounds__(kThreads) void conv_f16_kernel(const ConvF16Args a) {
  constexpr int WN = 4, NT = 2;
  constexpr int TAPS = KS * KS;
  constexpr int HALO = KS / 2;
  constexpr int PW = TW + 2 * HALO, PH = TH + 2 * HALO;
  constexpr int NPOS = PH * PW;  // halo positions = LDS rows of the input image
  constexpr int NPIX = TH * TW;
  constexpr int KC = TAPS * CK;  // K of one chunk
  constexpr int PITCH_IN = CK + 8, PITCH_W = KC + 8;  // halves
  static_assert(NPIX == WN * NT * 32, "eight waves of 32 channels x 64 pixels");
  static_assert(KS == 1 || TW == 32, "an N-tile is one tile row: 32 consecutive halo positions");
  static_assert(CK % 16 == 0, "whole 16-deep MFMA steps per tap");
  static_assert((PITCH_IN / 2) % 8 == 4 && (PITCH_W / 2) % 8 == 4, "pitch in dwords = 4 x odd (conflict-free 16-byte fragment reads)");
  static_assert(NPOS <= kThreads, "one staging thread per halo position");
  static_assert(!POOL || (KS == 3 && TH % 2 == 0), "pooling: 2x2 windows inside the tile, rows in neighbouring N-tiles");
  constexpr int NG = f16_stage_groups(NPOS, CK);
  constexpr int CPT = CK / NG;  // channels a staging thread brings in per chunk
  static_assert(CPT % 8 == 0, "whole 16-byte LDS stores");
  constexpr int W_U = kCoutTile * KC / 8;  // 16-byte units of a chunk's weight block
  constexpr int W_PER = (W_U + kThreads - 1) / kThreads;

  __shared__ __attribute__((aligned(16))) _Float16 in_tile[NPOS * PITCH_IN];
  __shared__ __attribute__((aligned(16))) _Float16 w_tile[kCoutTile * PITCH_W];
  __shared__ __attribute__((aligned(16))) float s_bias[kCoutTile], s_scale[kCoutTile], s_shift[kCoutTile];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int lane = tid & 63;
  const int half = lane >> 5;
  const int j = lane & 31;

  // work item = (pixel tile, output-channel tile), channel tile fastest (conv_block_kernel's order)
  const int ncot = (int)gridDim.y;
  const int item = xcd_contiguous((int)(blockIdx.x + blockIdx.y * gridDim.x), (int)gridDim.x * ncot);
  const int cot = item % ncot;
  const int co0 = cot * kCoutTile;
  int bid = item / ncot;
  const int tx_i = bid % a.tilesX;
  bid /= a.tilesX;
  const int ty_i = bid % a.tilesY;
  const int b = bid / a.tilesY;

  if (tid < kCoutTile) {  // visible to everyone after the main loop's first barrier
    const int co = co0 + tid;
    const bool cv = co < a.Cout;
    s_bias[tid] = (cv && a.bias) ? a.bias[co] : 0.0f;
    s_scale[tid] = (cv && a.scale) ? a.scale[co] : 1.0f;
    s_shift[tid] = (cv && a.scale) ? a.shift[co] : 0.0f;
  }
  const int HW = a.H * a.W;
  const int y0 = KS == 1 ? 0 : ty_i * TH, x0 = KS == 1 ? 0 : tx_i * TW;
  const int p0 = KS == 1 ? tx_i * NPIX : 0;  // flat pixel run

  // ---- per-lane pixel bookkeeping: fragment offsets (halves) and output pixels
  int bOff[NT], opix[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int q = (wn * NT + nt) * 32 + j;
    if (KS == 1) {
      bOff[nt] = q * PITCH_IN + 8 * half;
      opix[nt] = p0 + q < HW ? p0 + q : -1;
    } else {
      const int ty = q / TW, tx = q % TW;
      bOff[nt] = (ty * PW + tx) * PITCH_IN + 8 * half;
      const int y = y0 + ty, x = x0 + tx;
      opix[nt] = (y < a.H && x < a.W) ? y * a.W + x : -1;
    }
  }
  const int aOff = (wm * 32 + j) * PITCH_W + 8 * half;

  // ---- staging plan: this thread's halo position, the same in every chunk
  const unsigned plane = (unsigned)HW;
  const float* in_b = a.in + (size_t)b * a.Cin * plane;
  const int pos = NG == 1 ? tid : tid % NPOS;
  const int grp = NG == 1 ? 0 : tid / NPOS;
  const bool s_active = tid < NG * NPOS;
  int src_off = -1;
  if (KS == 1) {
    if (p0 + pos < HW) src_off = p0 + pos;
  } else {
    const int y = y0 - HALO + pos / PW, x = x0 - HALO + pos % PW;
    if (y >= 0 && y < a.H && x >= 0 && x < a.W) src_off = y * a.W + x;
  }
  const bool s_ok = s_active && src_off >= 0;
  _Float16* const in_dst = in_tile + pos * PITCH_IN + grp * CPT;
  // byte offset of this thread's element of the chunk's channel grp CPT: the chunk itself is stepped in the descriptor's base
  const unsigned in_voff = ((unsigned)(src_off >= 0 ? src_off : 0) + (unsigned)(grp * CPT) * plane) * 4u;
  const unsigned plane4 = plane * 4u;
  if (s_active && src_off < 0) {  // zero padding: written once, never again
    const h16x8 z = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
#pragma unroll
    for (int u = 0; u < CPT / 8; ++u) *reinterpret_cast<h16x8*>(in_dst + 8 * u) = z;
  }
  // the weight blocks of this channel tile: [chunk][64][KC] halves, whole (the image is zero-filled past cin and cout)
  const _Float16* w_cot = a.w + (size_t)cot * a.nchunks * (kCoutTile * KC);

  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;

  // register image of one chunk in flight (global -> registers -> convert -> LDS)
  float rin[CPT];
  f32x4 rw[W_PER];
  auto issue_loads = [&](int c) {
    if (s_ok) {
      const int ci0 = c * CK;
      // the descriptor spans channels ci0 .. Cin - 1 of this image: channels past Cin lie outside it and load as 0
      const __amdgpu_buffer_rsrc_t rs = f16_rsrc(in_b + (size_t)ci0 * plane, (unsigned)(a.Cin - ci0) * plane4);
#pragma unroll
      for (int i = 0; i < CPT; ++i) rin[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, in_voff + (unsigned)i * plane4, 0, 0));
    }
    const f32x4* wsrc = reinterpret_cast<const f32x4*>(w_cot + (size_t)c * (kCoutTile * KC));
#pragma unroll
    for (int i = 0; i < W_PER; ++i)
      if ((i + 1) * kThreads <= W_U || tid + i * kThreads < W_U) rw[i] = wsrc[tid + i * kThreads];
  };
  auto commit_loads = [&]() {
    if (s_ok) {
#pragma unroll
      for (int u = 0; u < CPT / 8; ++u) {
        h16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (_Float16)rin[8 * u + e];  // v_cvt_f16_f32 / v_cvt_pk_f16_f32: round to nearest even
        *reinterpret_cast<h16x8*>(in_dst + 8 * u) = v;
      }
    }
#pragma unroll
    for (int i = 0; i < W_PER; ++i)
      if ((i + 1) * kThreads <= W_U || tid + i * kThreads < W_U) {
        const int f = tid + i * kThreads;
        *reinterpret_cast<f32x4*>(w_tile + (f / (KC / 8)) * PITCH_W + (f % (KC / 8)) * 8) = rw[i];
      }
  };
  issue_loads(0);
  for (int c = 0; c < a.nchunks; ++c) {
    __syncthreads();  // the previous chunk's fragment reads are done
    commit_loads();
    __syncthreads();
    if (c + 1 < a.nchunks) issue_loads(c + 1);  // in flight under this chunk's MFMAs
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      const int shift = ((tap / KS) * PW + tap % KS) * PITCH_IN;
#pragma unroll
      for (int s = 0; s < CK / 16; ++s) {
        const h16x8 av = *reinterpret_cast<const h16x8*>(w_tile + aOff + tap * CK + s * 16);
        h16x8 bv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const h16x8*>(in_tile + bOff[nt] + shift + s * 16);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv[nt], acc[nt], 0, 0, 0);
      }
    }
  }

  // ---- epilogue (conv_block_kernel's): bias -> ReLU -> BN affine -> (pool) -> NCHW store through range-checked descriptors
  const int Ho = POOL ? a.H / 2 : a.H, Wo = POOL ? a.W / 2 : a.W;
  const unsigned plane_o = (unsigned)(Ho * Wo);
  float* out_b = a.out + (size_t)b * a.Cout * plane_o;
  // byte offset of each output this lane stores inside the descriptor of one accumulator row (lanes 32-63: four channels up);
  // all ones = nothing to store (dropped by the range check)
  constexpr int NO = POOL ? NT / 2 : NT;
  unsigned ovoff[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    int pix;
    if (POOL) {  // N-tiles 2o, 2o + 1 are tile rows 2k, 2k + 1; the window's top-left lane stores
      const int q = (wn * NT + 2 * o) * 32 + j;
      const int ty = q / TW, tx = q % TW;
      const int yo = (y0 + ty) >> 1, xo = (x0 + tx) >> 1;
      pix = (!(tx & 1) && yo < Ho && xo < Wo) ? yo * Wo + xo : -1;
    } else {
      pix = opix[o];
    }
    ovoff[o] = pix >= 0 ? ((unsigned)pix + (unsigned)(4 * half) * plane_o) * 4u : 0xFFFFFFFFu;
  }
  auto epilogue = [&](auto relu_c, auto aff_c) {
    constexpr bool RELU = decltype(relu_c)::value, AFF = decltype(aff_c)::value;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // accumulator rows 4g .. 4g+3 are channels cl0 + 4 half + (0..3) of the workgroup's 64
      const int cl0 = wm * 32 + 8 * g;
      const f32x4 bi = *reinterpret_cast<const f32x4*>(&s_bias[cl0 + 4 * half]);
      f32x4 sc, sh;
      if (AFF) {
        sc = *reinterpret_cast<const f32x4*>(&s_scale[cl0 + 4 * half]);
        sh = *reinterpret_cast<const f32x4*>(&s_shift[cl0 + 4 * half]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * g + i;
        const int co_r = co0 + cl0 + i;  // channel of lanes 0-31; lanes 32-63 hold channel co_r + 4
        const int nch = a.Cout - co_r > 0 ? a.Cout - co_r : 0;  // channels co_r .. Cout - 1 (none: every store of the row is dropped)
        const __amdgpu_buffer_rsrc_t ro = f16_rsrc(out_b + (size_t)co_r * plane_o, (unsigned)nch * plane_o * 4u);
        float pv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          float v = acc[nt][r] + bi[i];
          if (RELU) v = fmaxf(v, 0.0f);
          if (AFF) v = fmaf(v, sc[i], sh[i]);
          pv[nt] = v;
        }
        if (!POOL) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, pv[nt]), ro, ovoff[nt], 0, 0);
        } else {
#pragma unroll
          for (int o = 0; o < NO; ++o) {
            float m = fmaxf(pv[2 * o], pv[2 * o + 1]);  // rows 2k, 2k+1
            m = max_lane_xor1(m);                       // columns 2c, 2c+1
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, m), ro, ovoff[o], 0, 0);
          }
        }
      }
    }
  };
  using T_ = std::integral_constant<bool, true>;
  using F_ = std::integral_constant<bool, false>;
  if (a.relu) {
    if (a.scale) epilogue(T_{}, T_{});
    else epilogue(T_{}, F_{});
  } else {
    if (a.scale) epilogue(F_{}, T_{});
    else epilogue(F_{}, F_{});
  }
}

// OIHW fp32 -> binary16 image [cout tile][chunk][64][tap][ck]; the one rounding of the weights (v_cvt_f16_f32)
__global__ void conv_repack_f16_kernel(const float* __restrict__ w, int cin, int cout, int taps, int ck, int nchunks, size_t n, _Float16* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int cc = (int)(i % ck);
    size_t r = i / ck;
    const int tap = (int)(r % taps);
    r /= taps;
    const int col = (int)(r % kCoutTile);
    r /= kCoutTile;
    const int chunk = (int)(r % nchunks);
    const int cot = (int)(r / nchunks);
    const int ci = chunk * ck + cc, co = cot * kCoutTile + col;
    float v = 0.0f;
    if (ci < cin && co < cout) v = w[((size_t)co * cin + ci) * taps + tap];
    out[i] = (_Float16)v;
  }
}

thread_local const char* g_last_conv_f16_kernel = "";

// the dispatcher's instantiations: variant, KS, TH, TW, CK, POOL
#define EINX_CONV_F16_VARIANTS(X)      \
  X(CF_3X3, 3, 8, 32, 16, false)       \
  X(CF_3X3_POOL, 3, 8, 32, 16, true)   \
  X(CF_1X1, 1, 1, 256, 64, false)

enum ConvF16Variant {
#define X(V, ...) V,
  EINX_CONV_F16_VARIANTS(X)
#undef X
};

const char* conv_f16_name(int variant) {
  switch (variant) {
#define X(V, KS, TH, TW, CK, POOL) \
  case V: return "conv_f16_kernel<" #KS "," #TH "," #TW "," #CK "," #POOL ">";
    EINX_CONV_F16_VARIANTS(X)
#undef X
  }
  return "";
}

// why einx_conv_block_f16 does not take this layer and call (nullptr: it does); shared with einx_conv_f16_plan
const char* conv_f16_refused(int cin, int cout, int ks, int pool, int B, int H, int W) {
  if (!(ks == 1 || ks == 3)) return "kernel size must be 1 or 3";
  if (!(B > 0 && H > 0 && W > 0 && cin > 0 && cout > 0)) return "bad shape";
  if (cin % 8 != 0) return "cin must be a multiple of 8 (other layers stay on einx_conv_block)";
  if (pool && ((H & 1) || (W & 1))) return "pooling needs even H and W";
  if (pool && ks == 1) return "pooled 1x1 not supported";
  // byte offsets inside one image's [C,H,W] tensor are 32-bit, a staged chunk may name up to 64 channels past cin
  if (!((size_t)(cin + 64) * H * W < (1u << 30) && (size_t)(cout + 64) * H * W < (1u << 30))) return "image too large (2^30 elements per image and tensor)";
  return nullptr;
}

int conv_f16_variant(int ks, int pool) { return ks == 1 ? CF_1X1 : (pool ? CF_3X3_POOL : CF_3X3); }

}  // namespace

EINX_EXPORT const char* einx_conv_f16_last_kernel(void) { return g_last_conv_f16_kernel; }

EINX_EXPORT const char* einx_conv_f16_plan(int cin, int cout, int ks, int pool, int B, int H, int W) {
  if (const char* refused = conv_f16_refused(cin, cout, ks, pool, B, H, W)) {
    einx_set_error("%s: %s", __func__, refused);
    return nullptr;
  }
  return conv_f16_name(conv_f16_variant(ks, pool));
}

EINX_EXPORT size_t einx_conv_weight_elems_f16(int cin, int cout, int ks) {
  if (!(ks == 1 || ks == 3) || cin <= 0 || cout <= 0) return 0;
  const int ck = conv_f16_ck(ks);
  return (size_t)einx_cdiv(cout, kCoutTile) * einx_cdiv(cin, ck) * kCoutTile * (ks * ks) * ck;
}

EINX_EXPORT int einx_conv_repack_f16(const float* w_oihw, int cin, int cout, int ks, void* w_f16, void* stream) {
  EINX_CHECK_ARG(w_oihw && w_f16, "null pointer");
  EINX_CHECK_ARG(ks == 1 || ks == 3, "kernel size must be 1 or 3");
  EINX_CHECK_ARG(cin > 0 && cout > 0, "bad channel count");
  const int ck = conv_f16_ck(ks);
  const size_t n = einx_conv_weight_elems_f16(cin, cout, ks);
  const int blocks = (int)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256);
  hipLaunchKernelGGL(conv_repack_f16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w_oihw, cin, cout, ks * ks, ck, einx_cdiv(cin, ck), n,
                     (_Float16*)w_f16);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_conv_block_f16(const float* in, int B, int H, int W, const einx_conv_desc_f16* d, float* out, void* stream) {
  EINX_CHECK_ARG(in && out && d, "null pointer");
  EINX_CHECK_ARG(d->struct_size == sizeof(einx_conv_desc_f16), "einx_conv_desc_f16::struct_size does not match this library (ABI mismatch)");
  EINX_CHECK_ARG(d->w_f16, "null pointer");
  EINX_CHECK_ARG((d->scale == nullptr) == (d->shift == nullptr), "scale and shift go together");
  const char* refused = conv_f16_refused(d->cin, d->cout, d->ks, d->pool, B, H, W);
  EINX_CHECK_ARG(!refused, refused);
  ConvF16Args a;
  a.in = in;
  a.w = (const _Float16*)d->w_f16;
  a.bias = d->bias;
  a.scale = d->scale;
  a.shift = d->shift;
  a.out = out;
  a.B = B;
  a.Cin = d->cin;
  a.Cout = d->cout;
  a.CoutPad = einx_cdiv(d->cout, kCoutTile) * kCoutTile;
  a.H = H;
  a.W = W;
  a.relu = d->relu;
  a.nchunks = einx_cdiv(d->cin, conv_f16_ck(d->ks));
  const int variant = conv_f16_variant(d->ks, d->pool);
  hipStream_t s = (hipStream_t)stream;
  switch (variant) {
#define X(V, KS, TH, TW, CK, POOL)                                                                              \
  case V: {                                                                                                     \
    a.tilesX = KS == 1 ? einx_cdiv(H * W, TH * TW) : einx_cdiv(W, TW);                                          \
    a.tilesY = KS == 1 ? 1 : einx_cdiv(H, TH);                                                                  \
    const dim3 grid((unsigned)(a.tilesX * a.tilesY * B), (unsigned)(a.CoutPad / kCoutTile));                    \
    EINX_PROF(KS == 1 ? "conv_f16_kernel 1x1" : "conv_f16_kernel 3x3", s);                                      \
    hipLaunchKernelGGL((conv_f16_kernel<KS, TH, TW, CK, POOL>), grid, dim3(kThreads), 0, s, a);                 \
    break;                                                                                                      \
  }
    EINX_CONV_F16_VARIANTS(X)
#undef X
  }
  g_last_conv_f16_kernel = conv_f16_name(variant);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
