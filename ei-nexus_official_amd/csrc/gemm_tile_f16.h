// gemm_tile_f16.h -- 128x128x32 f16-MFMA "NT" tile engine beside gemm_tile.h (LightGlue's `mp: True`).
//   C[i][j] = sum_k RN16(A[i][k]) * B16[j][k]     (A: [M,K] fp32 row-major, B16: [N,K] binary16 row-major)
// A stays fp32 in memory and is rounded to binary16 between the global load and the LDS store (v_cvt_f16_f32: round to nearest
// even, overflow to infinity -- what tensor.half() does); B is read as binary16.  The products of two binary16 values are exact in
// fp32 and v_mfma_f32_32x32x16_f16 accumulates them in fp32, so a result differs from the exact sum by the order of K fp32 additions
// only.  Same wave arrangement (4 along M x 2 along N, a wave owns 32 x 64) and the same (wave, lane, register) -> (row, column)
// accumulator map as gemm_tile.h: einx_gemm::Frag, row_of / col_of and every epilogue written for them are reused unchanged.
//
// Operand lane map of v_mfma_f32_32x32x16_f16: lane l supplies row (l & 31) and the 8 consecutive k = 8 (l >> 5) .. + 7 of a 16-deep
// step, for A and B alike: one 16-byte LDS read per fragment.  LDS rows hold the slab's 32 halves at a pitch of 40 halves = 20 words,
// 4 (mod 8): the rows of 8 consecutive lanes start on the banks 0, 20, 8, 28, 16, 4, 24, 12 and cover 32 banks with their 4-word
// reads, so the 16-byte fragment reads are conflict-free (the rule lg_attn_f16_kernel's K rows follow).  20480 bytes per workgroup.
// The slab is 32 deep, not 64: a 64-deep slab keeps 24 VGPRs of loads in flight and every instantiation then spills under the
// 128-register budget of two workgroups per CU (92 to 244 bytes of scratch per lane, measured with tools/kernel_resources.py).
// K must be a multiple of 4 (A rows 16-byte, B16 rows 8-byte aligned); a tail beyond a multiple of 32 and rows past Mvalid / Nvalid
// are zero-filled.  Second A source as in gemm_tile.h: columns k >= Ksplit come from A2[i][k - Ksplit] (Ksplit % 4 == 0).
#pragma once
#include "gemm_tile.h"

namespace einx_gemm16 {

using einx_gemm::BM;
using einx_gemm::BN;
using einx_gemm::Frag;
using einx_gemm::MT;
using einx_gemm::NT;
using einx_gemm::THREADS;
using einx_gemm::WROWS;

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32, PITCH = BK + 8;               // halves
constexpr int LDS_HALVES = (BM + BN) * PITCH;
constexpr int C4 = BK / 4;                           // 4-element groups per operand row per K-slab
constexpr int STAGE = 128 * C4 / THREADS;            // groups per thread per operand per K-slab
static_assert(STAGE * THREADS == 128 * C4 && MT == 1, "eight waves of one 32-row block each");

struct Src {
  const float* A;
  const float* A2;
  const _Float16* B;
  int lda, lda2, ldb, i0, Mvalid, j0, Nvalid;
};

// register image of one K-slab of both operands (global -> registers -> convert -> LDS)
struct Stage {
  f32x4 ra[STAGE];
  h16x4 rb[STAGE];
};

__device__ __forceinline__ void issue_slab(const Src& s, int k0, int K, int Ksplit, Stage& st) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < STAGE; ++i) {
    const int fidx = tid + i * THREADS;
    const int r = fidx / C4, c4 = fidx % C4;
    const int k = k0 + c4 * 4;
    f32x4 va = {0.f, 0.f, 0.f, 0.f};
    h16x4 vb = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    if (s.i0 + r < s.Mvalid && k < K)
      va = (k < Ksplit) ? *reinterpret_cast<const f32x4*>(s.A + (size_t)(s.i0 + r) * s.lda + k)
                        : *reinterpret_cast<const f32x4*>(s.A2 + (size_t)(s.i0 + r) * s.lda2 + (k - Ksplit));
    if (s.j0 + r < s.Nvalid && k < K) vb = *reinterpret_cast<const h16x4*>(s.B + (size_t)(s.j0 + r) * s.ldb + k);
    st.ra[i] = va;
    st.rb[i] = vb;
  }
}

// Same contract as einx_gemm::tile_nt_run: issue_slab(cur, 0, ...) has been called into `st`; the first slab of `next` is requested
// during the last K-slab.  lds: LDS_HALVES halves, 16-byte aligned; no trailing barrier.
__device__ __forceinline__ void tile_nt_run(const Src& cur, int K, int Ksplit, _Float16* lds, Frag& f, Stage& st, const Src& next, bool has_next) {
  _Float16* As = lds;
  _Float16* Bs = lds + BM * PITCH;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) f.acc[0][nt][r] = 0.0f;
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
      const int fidx = tid + i * THREADS;
      const int r = fidx / C4, c4 = fidx % C4;
      const h16x4 a = {(_Float16)st.ra[i][0], (_Float16)st.ra[i][1], (_Float16)st.ra[i][2], (_Float16)st.ra[i][3]};  // v_cvt_f16_f32 (RNE)
      *reinterpret_cast<h16x4*>(As + r * PITCH + c4 * 4) = a;
      *reinterpret_cast<h16x4*>(Bs + r * PITCH + c4 * 4) = st.rb[i];
    }
  };
  const _Float16* afrag = As + (wm * WROWS + l31) * PITCH + 8 * half;
  const _Float16* bfrag = Bs + (wn * 64 + l31) * PITCH + 8 * half;
  // whole tiles of whole slabs reload without predicates: per-thread element offsets that never change from a base that moves with k0
  const bool whole = cur.i0 + BM <= cur.Mvalid && cur.j0 + BN <= cur.Nvalid && K % BK == 0 && (cur.A2 == nullptr || Ksplit % BK == 0);
  // (group i of a thread is row tid / C4 + i * RSTEP: one lane offset per operand, the row step goes into the uniform base)
  constexpr int RSTEP = THREADS / C4;
  const unsigned offa = (unsigned)((tid / C4) * cur.lda + (tid % C4) * 4);
  const unsigned offa2 = (unsigned)((tid / C4) * cur.lda2 + (tid % C4) * 4);
  const unsigned offb = (unsigned)((tid / C4) * cur.ldb + (tid % C4) * 4);
  const float* a_tile = cur.A + (size_t)cur.i0 * cur.lda;
  const float* a2_tile = cur.A2 ? cur.A2 + (size_t)cur.i0 * cur.lda2 : nullptr;
  const _Float16* b_tile = cur.B + (size_t)cur.j0 * cur.ldb;
  auto issue_whole = [&](int k) {
    if (k < Ksplit) {
#pragma unroll
      for (int i = 0; i < STAGE; ++i) st.ra[i] = *reinterpret_cast<const f32x4*>(a_tile + k + (size_t)(i * RSTEP) * cur.lda + offa);
    } else {
#pragma unroll
      for (int i = 0; i < STAGE; ++i) st.ra[i] = *reinterpret_cast<const f32x4*>(a2_tile + (k - Ksplit) + (size_t)(i * RSTEP) * cur.lda2 + offa2);
    }
#pragma unroll
    for (int i = 0; i < STAGE; ++i) st.rb[i] = *reinterpret_cast<const h16x4*>(b_tile + k + (size_t)(i * RSTEP) * cur.ldb + offb);
  };
  for (int k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();  // the previous slab's (or tile's) fragment reads are done
    commit();
    __syncthreads();
    if (k0 + BK < K) {  // in flight under the MFMAs below
      if (whole) issue_whole(k0 + BK);
      else issue_slab(cur, k0 + BK, K, Ksplit, st);
    } else if (has_next) {
      issue_slab(next, 0, K, Ksplit, st);
    }
    // (two 16-deep steps per slab; the fragment reads are not software-pipelined, the other resident waves cover the LDS latency)
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      const h16x8 av = *reinterpret_cast<const h16x8*>(afrag + kk * 16);
      h16x8 bv[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const h16x8*>(bfrag + nt * 32 * PITCH + kk * 16);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) f.acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv[nt], f.acc[0][nt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

}  // namespace einx_gemm16
