// lightglue.hip -- LightGlue inference on gfx950 (fp32 end to end, fp32 matrix cores; with the opt-in `flash: True` the attention
// alone runs in fp16 on the f16 matrix-core instruction: lg_attn_f16_kernel; with the opt-in `mp: True` the layers'
// linears run on it too, lg_gemm_kernel on the f16 tile engine of gemm_tile_f16.h).
//
// Per layer: SelfBlock (Wqkv GEMM -> rotary -> fused softmax(QK^T/8)V -> out_proj GEMM ->
// concat-free FFN GEMM -> LayerNorm+GELU -> FFN GEMM + residual) on both sides, then CrossBlock
// (to_qk / to_v GEMMs, two fused attentions sharing the 1/8 scale, to_out, same FFN).  After the
// last layer MatchAssignment: final_proj/d^(1/4), similarity tiles with double log-softmax +
// matchability (match_tiles.h), mutual filter.  Everything for a batch of pairs is enqueued on one
// stream with device-side keypoint counts; no host synchronisation.
//
// Attention is flash-style per (pair, head, 128 queries): S^T = K Q^T on the matrix cores with the
// query on the MFMA column so that (a) the online-softmax state (running max / sum) is per lane
// and (b) the probability registers are directly the B operand of the PV product O^T = V^T P^T --
// no LDS round trip for P.  K/V blocks of 64 keys are staged through LDS (K with an odd pitch).
//
// Replaces (reference file:line): core/modules/matchers/lightglue.py:137-148 (normalize_keypoints),
// :161-174 (posenc), :151-158 (rotary), :240-272 (SelfBlock), :275-330 (CrossBlock), :365-418
// (assignment + filter_matches), :522-716 (forward).
#include <stdlib.h>

#include "gemm_tile_f16.h"
#include "match_tiles.h"

using namespace einx_gemm;
using namespace einx_match;

namespace {

// The shipped configuration (every EI-Nexus YAML): descriptor_dim 256 = 4 heads x 64.  Its kernels are instantiated with these
// as compile-time constants; any other (heads, head_dim in {32, 64, 128}) configuration of lightglue.py:456-461 runs the same
// kernels with the widths taken from the arguments.
constexpr int D = 256;   // descriptor_dim
constexpr int DH = 64;   // head dim

__device__ __forceinline__ int crow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ------------------------------------------------------------------------------------------
// positional encoding: enc[b][i][0..dh-1] = cos, [dh..2dh-1] = sin of Wr . normalised keypoint (Wr: [dh/2, 2]),
// each frequency repeated twice (repeat_interleave(2)).
// ------------------------------------------------------------------------------------------
__global__ void lg_posenc_kernel(const float* kpts, const int32_t* cnt, int cap, float s0, float s1, const float* Wr, float* enc, int dh) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int nf = dh >> 1;
  const int i = t / nf, f = t - i * nf;
  if (i >= n) return;
  const float sh0 = s0 / 2.0f, sh1 = s1 / 2.0f;
  const float sc = fmaxf(s0, s1) / 2.0f;
  const float* kp = kpts + ((size_t)b * cap + i) * 3;
  const float k0 = (kp[0] - sh0) / sc, k1 = (kp[1] - sh1) / sc;
  float p = fmaf(k0, Wr[f * 2 + 0], 0.0f);
  p = fmaf(k1, Wr[f * 2 + 1], p);
  float sn, cs;
  einx_sincosf(p, &sn, &cs);
  float* e = enc + ((size_t)b * cap + i) * (2 * dh);
  e[2 * f] = cs;
  e[2 * f + 1] = cs;
  e[dh + 2 * f] = sn;
  e[dh + 2 * f + 1] = sn;
}

// ------------------------------------------------------------------------------------------
// batched Linear: Y[b,i,:] = cat(X[b,i,:], X2[b,i,:]) @ W^T + bias  (+ epilogue)
// ------------------------------------------------------------------------------------------
enum { EPI_BIAS = 0, EPI_DIV = 1, EPI_RESID = 2, EPI_ROPE = 3, EPI_ROPE_ANY = 4, EPI_DIV_HEAD = 5 };  // ROPE: d = 256, 64-wide heads; ROPE_ANY: g.d / g.dh
// EPI_DIV_HEAD: EPI_DIV with every entry's W / bias taken from the head its pair stopped at (early stopping)

struct GemmArgs {
  const float* X;
  const float* X2;
  const float* W;
  const float* bias;
  float* Y;
  const int32_t* cnt;  // per-batch row counts, or null: every batch has `cap` rows
  int cap, ldx, ldx2, Ksplit, K, N, ldy, B;
  float div;
  // EPI_ROPE / EPI_ROPE_ANY (the Wqkv projection of SelfBlock, lightglue.py:252-272): W rows are laid out (head, dim, 3);
  // the tile list walks them as three d-column blocks q | k | v (row stride 3 in W), applies the cached
  // rotary encoding to q and k in the epilogue and writes the three [B,cap,d] buffers directly
  const float* enc;  // [B,cap,2 dh]: cos(dh) | sin(dh)
  float *Yq, *Yk, *Yv;
  int d, dh;  // read by EPI_ROPE_ANY only (dh even: rotary pairs are adjacent columns)
  // EPI_DIV_HEAD only: heads[4 h + 0 / 1] = final_proj weight / bias of log_assignment[h] (device table); entry b belongs to pair
  // b mod pairs, whose head is stop - 1 (the last one, nheads - 1, for stop == 0: an empty pair runs as it always did)
  const float* const* heads;
  const int32_t* stop;
  int pairs, nheads;
};

__device__ __forceinline__ int head_of(const int32_t* stop, int pairs, int nheads, int b) {
  const int s = stop[b < pairs ? b : b - pairs];
  return s > 0 ? s - 1 : nheads - 1;
}

// Persistent workgroups: the launch holds as many workgroups as the chip runs at once (a multiple
// of 8) and each walks a list of 128x128 tiles.  Workgroups w and w+8 share an XCD (round-robin
// dispatch), so the tile list of XCD x is built from whole A-row groups: the tilesN tiles that read
// the same 128 rows of X are computed on one XCD at about the same time and X is fetched into that
// L2 once.  The next tile's first K-slab is requested during the current tile's last K-slab, so its
// latency and the epilogue's stores overlap instead of serialising per tile.
//
// Eng: the tile engine.  EngF32 (gemm_tile.h, the default: every fp32 launch) or EngF16 (gemm_tile_f16.h: X rounded to binary16 on
// the way into LDS, W read as binary16 through g.W, fp32 accumulation; LightGlue's `mp: True`).  Both fill the same
// Frag with the same (wave, lane, register) -> (row, column) map, so the tile walk and the epilogues below serve both.
struct EngF32 {
  using WT = float;
  using Src = einx_gemm::Src;
  using Stage = einx_gemm::Stage;
  static constexpr int LDS_FLOATS = einx_gemm::LDS_FLOATS;
  static __device__ __forceinline__ void issue(const Src& s, int k0, int K, int Ksplit, Stage& st) { einx_gemm::issue_slab(s, k0, K, Ksplit, st); }
  static __device__ __forceinline__ void run(const Src& cur, int K, int Ksplit, float* lds, Frag& f, Stage& st, const Src& next, bool has_next) {
    einx_gemm::tile_nt_run(cur, K, Ksplit, lds, f, st, next, has_next);
  }
};
struct EngF16 {
  using WT = _Float16;
  using Src = einx_gemm16::Src;
  using Stage = einx_gemm16::Stage;
  static constexpr int LDS_FLOATS = einx_gemm16::LDS_HALVES / 2;
  static __device__ __forceinline__ void issue(const Src& s, int k0, int K, int Ksplit, Stage& st) { einx_gemm16::issue_slab(s, k0, K, Ksplit, st); }
  static __device__ __forceinline__ void run(const Src& cur, int K, int Ksplit, float* lds, Frag& f, Stage& st, const Src& next, bool has_next) {
    einx_gemm16::tile_nt_run(cur, K, Ksplit, reinterpret_cast<_Float16*>(lds), f, st, next, has_next);
  }
};

template <int EPI, typename Eng = EngF32>
__global__ __launch_bounds__(THREADS, 2 * THREADS / 256) void lg_gemm_kernel(const GemmArgs g) {  // registers for two resident workgroups per CU
  using Src = typename Eng::Src;
  using Stage = typename Eng::Stage;
  using WT = typename Eng::WT;
  __shared__ __attribute__((aligned(16))) float lds[Eng::LDS_FLOATS];
  const WT* const W = reinterpret_cast<const WT*>(g.W);  // (EngF16: the binary16 image of the weight)
  constexpr bool ROPE = EPI == EPI_ROPE || EPI == EPI_ROPE_ANY;
  const int rd = EPI == EPI_ROPE ? D : g.d;              // width of the q | k | v blocks (ROPE only)
  const int rdh = EPI == EPI_ROPE ? DH : g.dh;
  const int tpb = EPI == EPI_ROPE ? D / BN : einx_cdiv(rd, BN);  // tiles per q | k | v block
  const int tilesN = ROPE ? 3 * tpb : einx_cdiv(g.N, BN), tilesM = einx_cdiv(g.cap, BM);
  const int groups = tilesM * g.B;                       // A-row groups
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, slots = gridDim.x >> 3;
  const int local_tiles = einx_cdiv(groups, 8) * tilesN;  // tiles in this XCD's list
  // tile L of this XCD's list -> operands; false when the tile does not exist / has no valid rows
  auto locate = [&](int L, Src& s, int& bb, int& nn) {
    const int grp = (L / tilesN) * 8 + xcd;
    if (grp >= groups) return false;
    const int b = grp / tilesM, ti = grp % tilesM;
    const int n = g.cnt ? min(g.cnt[b], g.cap) : g.cap;
    if (ti * BM >= n) return false;
    s.A = g.X + (size_t)b * g.cap * g.ldx;
    s.A2 = g.X2 ? g.X2 + (size_t)b * g.cap * g.ldx2 : nullptr;
    s.lda = g.ldx;
    s.lda2 = g.ldx2;
    s.i0 = ti * BM;
    s.Mvalid = n;
    if (ROPE) {  // tile tj: block t = tj / tpb of (q, k, v), columns hc0.. of that block = W rows (hc0 + r) * 3 + t
      const int tj = L % tilesN;
      s.B = W + (size_t)(tj / tpb) * g.K;
      s.ldb = 3 * g.K;
      s.j0 = (tj % tpb) * BN;
      s.Nvalid = rd;
    } else {
      s.B = EPI == EPI_DIV_HEAD ? reinterpret_cast<const WT*>(g.heads[4 * head_of(g.stop, g.pairs, g.nheads, b)]) : W;
      s.ldb = g.K;
      s.j0 = (L % tilesN) * BN;
      s.Nvalid = g.N;
    }
    bb = b;
    nn = n;
    return true;
  };
  Src cur, nxt;
  int b = 0, n = 0, nb = 0, nn = 0;
  int L = slot;
  while (L < local_tiles && !locate(L, cur, b, n)) L += slots;
  if (L >= local_tiles) return;
  Stage st;
  Eng::issue(cur, 0, g.K, g.Ksplit, st);
  for (;;) {
    int Ln = L + slots;
    while (Ln < local_tiles && !locate(Ln, nxt, nb, nn)) Ln += slots;
    const bool more = Ln < local_tiles;
    Frag f;
    Eng::run(cur, g.K, g.Ksplit, lds, f, st, nxt, more);
    const int i0 = cur.i0, j0 = cur.j0;
    if (ROPE) {
      const int t = (int)((cur.B - W) / g.K);  // 0: q, 1: k, 2: v
      float* Yt = (t == 0 ? g.Yq : t == 1 ? g.Yk : g.Yv) + (size_t)b * g.cap * rd;
      const float* encb = g.enc + (size_t)b * g.cap * (2 * rdh);
      const bool odd = threadIdx.x & 1;  // column parity == lane parity (col_of(nt) = 64*wn + 32*nt + lane%32)
      float bq[NT];
      int hc[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        hc[nt] = j0 + col_of(nt);
        bq[nt] = (EPI == EPI_ROPE || hc[nt] < rd) ? g.bias[hc[nt] * 3 + t] : 0.0f;
      }
      // rows go in batches of 4: the 16 cos/sin loads of a batch are issued together, ahead of its stores
      // (the compiler cannot move a load above an earlier store through plain float pointers)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 4) {
          float cs[4][NT], sn[4][NT];
          if (t < 2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = i0 + row_of(mt, r0 + r);
              const float* e = encb + (size_t)(i < n ? i : n - 1) * (2 * rdh);
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) {
                const int hd = EPI == EPI_ROPE ? (hc[nt] & (DH - 1)) : hc[nt] % rdh;  // column inside its head (any even head width)
                cs[r][nt] = e[hd];
                sn[r][nt] = e[rdh + hd];
              }
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = i0 + row_of(mt, r0 + r);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              float v = f.acc[mt][nt][r0 + r] + bq[nt];
              const float partner = __shfl_xor(v, 1, 64);  // the other element of the rotary pair (adjacent column)
              if (t < 2) v = (v * cs[r][nt]) + ((odd ? partner : -partner) * sn[r][nt]);  // rotate_half: (x0,x1) -> (-x1,x0), lightglue.py:151-158
              if (i < n && (EPI == EPI_ROPE || hc[nt] < rd)) Yt[(size_t)i * rd + hc[nt]] = v;
            }
          }
        }
      if (!more) break;
      cur = nxt;
      b = nb;
      n = nn;
      L = Ln;
      continue;
    }
    float* Y = g.Y + (size_t)b * g.cap * g.ldy;
    // epilogue: the bias of a lane's NT columns is loaded once; whole tiles take a guard-free path so
    // that the residual loads / stores of all 16*MT rows are issued back to back instead of one
    // load -> wait -> store round trip per element
    float bj[NT];
    int jj[NT];
    const float* bias = EPI == EPI_DIV_HEAD ? g.heads[4 * head_of(g.stop, g.pairs, g.nheads, b) + 1] : g.bias;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int j = j0 + col_of(nt);
      jj[nt] = j < g.N ? j : -1;
      bj[nt] = j < g.N ? bias[j] : 0.0f;
    }
    auto finish = [&](float acc, float bias, float old) {
      float v = acc + bias;
      if (EPI == EPI_DIV || EPI == EPI_DIV_HEAD) v = v / g.div;
      if (EPI == EPI_RESID) v = old + v;
      return v;
    };
    if (i0 + BM <= n && j0 + BN <= g.N) {
      // uniform row pointer (scalar registers) + one 32-bit lane offset shared by every access
      float* ytile = Y + (size_t)i0 * g.ldy + j0;
      const unsigned lane_off = (unsigned)(row_base() * g.ldy + col_of(0));
      // rows go in batches of 8: eight residual loads in flight, then eight stores
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 8) {
          float old[8][NT];
          if (EPI == EPI_RESID) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
              const float* yrow = ytile + (size_t)row_step(mt, r0 + r) * g.ldy;
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) old[r][nt] = yrow[lane_off + nt * 32];
            }
          }
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            float* yrow = ytile + (size_t)row_step(mt, r0 + r) * g.ldy;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              yrow[lane_off + nt * 32] = finish(f.acc[mt][nt][r0 + r], bj[nt], EPI == EPI_RESID ? old[r][nt] : 0.0f);
          }
        }
    } else {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = i0 + row_of(mt, r);
          if (i >= n) continue;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            if (jj[nt] < 0) continue;
            float* y = Y + (size_t)i * g.ldy + jj[nt];
            *y = finish(f.acc[mt][nt][r], bj[nt], EPI == EPI_RESID ? *y : 0.0f);
          }
        }
    }
    if (!more) break;
    cur = nxt;
    b = nb;
    n = nn;
    L = Ln;
  }
}

// ------------------------------------------------------------------------------------------
// The same linears for SMALL grids (single pairs: fewer 128x128 tiles than CUs).  A launch that cannot fill the chip is
// bound by the latency of ONE tile's K loop (8 waves x 32 MFMAs + staging per 32-deep slab, 10-20 us per tile however few
// tiles there are): 64x64 tiles on 4 waves of one 32x32 accumulator each halve the matrix work per slab and give 4x the
// workgroups.  Same K order per output (one k-ordered chain from +0), so results are bit-identical to lg_gemm_kernel;
// same four epilogues.  K % 32 == 0 and N % 64 == 0 (every LightGlue shape); one tile per workgroup, no persistence.
// ------------------------------------------------------------------------------------------
constexpr int SBM = 64, SBN = 64, SBK = 32, SP = SBK + 1;
template <int EPI>
__global__ __launch_bounds__(256) void lg_gemm_small_kernel(const GemmArgs g) {
  __shared__ float As[SBM * SP];
  __shared__ float Bs[SBN * SP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  const int b = blockIdx.z;
  const int n = g.cnt ? min(g.cnt[b], g.cap) : g.cap;
  const int i0 = (int)blockIdx.y * SBM;
  if (i0 >= n) return;
  const int tj = (int)blockIdx.x;
  int j0, t = 0;
  const float* Wb;
  int ldb;
  constexpr bool ROPE = EPI == EPI_ROPE || EPI == EPI_ROPE_ANY;
  const int rd = EPI == EPI_ROPE ? D : g.d, rdh = EPI == EPI_ROPE ? DH : g.dh;
  if (ROPE) {  // d / 64 tiles of 64 columns per (q | k | v) block; W rows (hc + r) * 3 + t (see lg_gemm_kernel)
    const int tpb = rd / SBN;
    t = tj / tpb;
    j0 = (tj - t * tpb) * SBN;
    Wb = g.W + (size_t)t * g.K;
    ldb = 3 * g.K;
  } else {
    j0 = tj * SBN;
    Wb = EPI == EPI_DIV_HEAD ? g.heads[4 * head_of(g.stop, g.pairs, g.nheads, b)] : g.W;
    ldb = g.K;
  }
  const float* A1 = g.X + (size_t)b * g.cap * g.ldx;
  const float* A2 = g.X2 ? g.X2 + (size_t)b * g.cap * g.ldx2 : nullptr;
  // staging: 64 rows x 8 float4 per operand and slab = 2 float4 per thread; rows past n read row n - 1 (never stored)
  int ra[2], c4a[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int f = tid + i * 256;
    ra[i] = f >> 3;
    c4a[i] = f & 7;
  }
  f32x4 va[2], vb[2];
  auto issue = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = min(i0 + ra[i], n - 1);
      const int k = k0 + c4a[i] * 4;
      va[i] = (k < g.Ksplit) ? *reinterpret_cast<const f32x4*>(A1 + (size_t)row * g.ldx + k)
                             : *reinterpret_cast<const f32x4*>(A2 + (size_t)row * g.ldx2 + (k - g.Ksplit));
      vb[i] = *reinterpret_cast<const f32x4*>(Wb + (size_t)(j0 + ra[i]) * ldb + k);
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  issue(0);
  const int aoff = (wm * 32 + l31) * SP + half, boff = (wn * 32 + l31) * SP + half;
  for (int k0 = 0; k0 < g.K; k0 += SBK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        As[ra[i] * SP + c4a[i] * 4 + e] = va[i][e];
        Bs[ra[i] * SP + c4a[i] * 4 + e] = vb[i][e];
      }
    __syncthreads();
    if (k0 + SBK < g.K) issue(k0 + SBK);
    float av[2], bv[2];
    av[0] = As[aoff];
    bv[0] = Bs[boff];
#pragma unroll
    for (int kk = 0; kk < SBK / 2; ++kk) {
      if (kk + 1 < SBK / 2) {
        av[(kk + 1) & 1] = As[aoff + (kk + 1) * 2];
        bv[(kk + 1) & 1] = Bs[boff + (kk + 1) * 2];
      }
      __builtin_amdgcn_sched_barrier(0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk & 1], bv[kk & 1], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // ---- epilogue: C row (r & 3) + 8 (r >> 2) + 4 half of the wave's 32x32 tile, column l31
  const int col = j0 + wn * 32 + l31;  // < N (N % 64 == 0); for EPI_ROPE the column inside the 256-wide q / k / v block
  int rows[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) rows[r] = i0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
  if (ROPE) {
    float* Yt = (t == 0 ? g.Yq : t == 1 ? g.Yk : g.Yv) + (size_t)b * g.cap * rd;
    const float* encb = g.enc + (size_t)b * g.cap * (2 * rdh);
    const float bq = g.bias[col * 3 + t];
    const bool odd = lane & 1;
    float cs[16], sn[16];
    if (t < 2) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* e = encb + (size_t)min(rows[r], n - 1) * (2 * rdh);
        const int hd = EPI == EPI_ROPE ? (col & (DH - 1)) : col % rdh;
        cs[r] = e[hd];
        sn[r] = e[rdh + hd];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[r] + bq;
      const float partner = __shfl_xor(v, 1, 64);
      if (t < 2) v = (v * cs[r]) + ((odd ? partner : -partner) * sn[r]);
      if (rows[r] < n) Yt[(size_t)rows[r] * rd + col] = v;
    }
    return;
  }
  float* Y = g.Y + (size_t)b * g.cap * g.ldy;
  const float bj = (EPI == EPI_DIV_HEAD ? g.heads[4 * head_of(g.stop, g.pairs, g.nheads, b) + 1] : g.bias)[col];
  float old[16];
  if (EPI == EPI_RESID) {
#pragma unroll
    for (int r = 0; r < 16; ++r) old[r] = Y[(size_t)min(rows[r], n - 1) * g.ldy + col];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r] + bj;
    if (EPI == EPI_DIV || EPI == EPI_DIV_HEAD) v = v / g.div;
    if (EPI == EPI_RESID) v = old[r] + v;
    if (rows[r] < n) Y[(size_t)rows[r] * g.ldy + col] = v;
  }
}


// ------------------------------------------------------------------------------------------
// fused attention: out[b,q,h*HD:(h+1)*HD] = softmax_j(scale * Q_h[q] . K_h[j]) V_h[j]
// HD: head dim (32 / 64 / 128); DD: row width d of Q / K / V / O as a compile-time constant (256: the shipped instantiation) or 0 = a.d;
// LD: row stride of Q / K / V when they are column blocks of a wider buffer (the merged to_qk | to_v projection: 512), 0 = the width
// ------------------------------------------------------------------------------------------
struct AttnArgs {
  const float* Q;
  const float* K;
  const float* V;
  float* O;
  const int32_t* nq;
  const int32_t* nk;
  int capq, capk;
  float scale;
  int kv_shift, Btot;  // keys / values of batch entry b come from entry (b + kv_shift) % Btot (cross attention over the two sides stacked in one buffer)
  int d;               // row width (heads * head dim); read when the kernel's DD is 0
  int dh;              // head width when the kernel's DD is 0: <= HD, a multiple of 4; dims dh .. HD - 1 are zero padding
};

constexpr int AKB = 32;   // keys staged per round (32: 124 VGPRs -> three workgroups per CU; 64: 151 -> two)
template <int HD, int DD, int LD = 0>
__global__ __launch_bounds__(256) void lg_attn_kernel(const AttnArgs a) {
  constexpr int KPITCH = HD + 4;  // K rows padded by 4 floats (64-wide heads: 68): 16-byte aligned for ds_read_b128, and the 32 rows a
                                  // half-wave reads start on 16 distinct 4-bank groups (conflict-free)
  constexpr int DH = HD;          // (shadows the file-level constant)
  __shared__ __attribute__((aligned(16))) float Ks[AKB * KPITCH];
  __shared__ __attribute__((aligned(16))) float Vs[AKB * DH];
  const int D = DD ? DD : a.d;
  const int DL = LD ? LD : D;  // row stride of Q / K / V
  // the query blocks of one (pair, head) read the same K / V: keep them on one XCD (see xcd_contiguous)
  const int gx = (int)gridDim.x, gy = (int)gridDim.y;
  int item = xcd_contiguous((int)(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z)), gx * gy * (int)gridDim.z);
  const int qb = item % gx;
  item /= gx;
  const int h = item % gy, b = item / gy;
  const int bk = a.kv_shift ? (b + a.kv_shift) % a.Btot : b;
  const int nq = min(a.nq[b], a.capq), nk = min(a.nk[bk], a.capk);
  const int q0 = qb * 128;
  if (q0 >= nq || nk <= 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q = q0 + wave * 32 + l31;
  const bool qv = q < nq;
  // MFMA K-step t pairs head dims (t, t + DH/2): lane half h supplies dim t + (DH/2) h, so a lane's K fragments
  // for four consecutive steps are one 16-byte LDS read
  // Head widths that are not 32 / 64 / 128 (lightglue.py:456-461 takes any descriptor_dim // num_heads) run the next larger
  // instantiation on zero-padded heads (DD == 0 only): dims dhr .. HD - 1 of Q, K and V read as 0 -- exact zeros add nothing
  // to a dot product -- and are not stored.  The head's columns start at h * dhr.
  const int dhr = DD ? DH : a.dh;
  const float* Qrow = a.Q + ((size_t)b * a.capq + (qv ? q : nq - 1)) * DL + h * dhr + (DH / 2) * half;
  float qreg[DH / 2];
#pragma unroll
  for (int t = 0; t < DH / 2; t += 4) {
    const f32x4 v = (DD || (DH / 2) * half + t < dhr) ? *reinterpret_cast<const f32x4*>(Qrow + t) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    qreg[t] = v[0];
    qreg[t + 1] = v[1];
    qreg[t + 2] = v[2];
    qreg[t + 3] = v[3];
  }
  const float* Kb = a.K + (size_t)bk * a.capk * DL + h * dhr;
  const float* Vb = a.V + (size_t)bk * a.capk * DL + h * dhr;
  constexpr int OT = DH / 32;  // 32-wide blocks of the output row
  f32x16 o[OT];
#pragma unroll
  for (int mt = 0; mt < OT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[mt][r] = 0.0f;
  const float NEG = -einx_u2f(0x7f800000u);
  const float sl2 = a.scale * 1.44269504088896341f;  // softmax in base 2: exp(x) = 2^(x log2 e)
  float m_run = NEG, l_run = 0.0f;

  // K/V block staging through registers: block kb0+64 is in flight while block kb0 is consumed
  constexpr int R4 = DH / 4;               // float4 per K / V row
  constexpr int ASTG = AKB * R4 / 256;     // float4 per thread per operand per round
  static_assert(ASTG >= 1 && DH % 32 == 0, "head dim 32, 64 or 128");
  f32x4 rk[ASTG], rv[ASTG];
  auto issue = [&](int kb0) {
#pragma unroll
    for (int i = 0; i < ASTG; ++i) {
      const int fidx = tid + i * 256;
      const int row = fidx / R4, c4 = fidx % R4;
      const int key = min(kb0 + row, nk - 1);  // clamped: rows past nk are masked after the QK product
      if (DD || c4 * 4 < dhr) {
        rk[i] = *reinterpret_cast<const f32x4*>(Kb + (size_t)key * DL + c4 * 4);
        rv[i] = *reinterpret_cast<const f32x4*>(Vb + (size_t)key * DL + c4 * 4);
      } else {
        rk[i] = rv[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < ASTG; ++i) {
      const int fidx = tid + i * 256;
      const int row = fidx / R4, c4 = fidx % R4;
      *reinterpret_cast<f32x4*>(Ks + row * KPITCH + c4 * 4) = rk[i];
      *reinterpret_cast<f32x4*>(Vs + row * DH + c4 * 4) = rv[i];
    }
  };
  issue(0);
  for (int kb0 = 0; kb0 < nk; kb0 += AKB) {
    __syncthreads();
    commit();
    __syncthreads();
    if (kb0 + AKB < nk) issue(kb0 + AKB);
#pragma unroll
    for (int sub = 0; sub < AKB / 32; ++sub) {
      const int kbase = kb0 + sub * 32;
      if (kbase >= nk) break;
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.0f;
      const float* krow = Ks + (sub * 32 + l31) * KPITCH + (DH / 2) * half;
      f32x4 kf[2];
      kf[0] = *reinterpret_cast<const f32x4*>(krow);
#pragma unroll
      for (int u = 0; u < DH / 8; ++u) {
        if (u + 1 < DH / 8) kf[(u + 1) & 1] = *reinterpret_cast<const f32x4*>(krow + 4 * (u + 1));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 4; ++t) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u & 1][t], qreg[4 * u + t], s, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      float mx = NEG;
      if (kbase + 32 <= nk) {  // whole block (uniform): no key mask
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[r] = s[r] * sl2;
          mx = fmaxf(mx, s[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kbase + crow(r, half);
          s[r] = key < nk ? s[r] * sl2 : NEG;
          mx = fmaxf(mx, s[r]);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      // v_exp_f32 (2^x, ~1 ulp): LightGlue is compared at 1e-4, so the exact-order einx_expf is not
      // needed here; 2^(-inf) = 0 handles masked keys and the first block
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      float psum = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = __builtin_amdgcn_exp2f(s[r] - m_new);
        psum += s[r];
      }
      l_run = l_run * alpha + psum;
      m_run = m_new;
      // once the running maxima have settled alpha is exactly 1 in every lane: skip the 32 multiplications by one
      // (wave-uniform branch; bit-identical, x * 1.0f == x)
      if (__any(alpha != 1.0f)) {
#pragma unroll
        for (int mt = 0; mt < OT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[mt][r] *= alpha;
      }
      const float* vbase = Vs + (size_t)(sub * 32 + 4 * half) * DH + l31;
      float vf[2][OT];
#pragma unroll
      for (int mt = 0; mt < OT; ++mt) vf[0][mt] = vbase[crow(0, 0) * DH + 32 * mt];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (r + 1 < 16) {
#pragma unroll
          for (int mt = 0; mt < OT; ++mt) vf[(r + 1) & 1][mt] = vbase[crow(r + 1, 0) * DH + 32 * mt];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mt = 0; mt < OT; ++mt) o[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[r & 1][mt], s[r], o[mt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  const float l = l_run + __shfl_xor(l_run, 32, 64);
  if (qv) {
    float* orow = a.O + ((size_t)b * a.capq + q) * D + h * dhr;
#pragma unroll
    for (int mt = 0; mt < OT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (DD || mt * 32 + crow(r, half) < dhr) orow[mt * 32 + crow(r, half)] = o[mt][r] / l;
  }
}

// ------------------------------------------------------------------------------------------
// The same attention for SMALL grids (single pairs: 64 workgroups of lg_attn_kernel on 256 CUs, each wave walking all keys of
// its 32 queries alone: 32 key blocks x ~2.4 us).  Here ONE workgroup of four waves owns 32 queries and the waves share the
// matrix work of every key block, on the 16x16x4 instruction (which accumulates its four K products as a sequential fma chain
// like 32x32x2 its two: tools/mfma16_order.hip), so that every output is the SAME chain of operations as in lg_attn_kernel:
//   A  S^T quadrant (16 keys x 16 queries) per wave: K-step g feeds dims (2g, 32+2g, 2g+1, 33+2g) = steps 2g, 2g+1 of the wide kernel
//   B  every wave redoes the block's online softmax for all 32 queries in the wide kernel's lane layout (query = lane % 32, the
//      16 keys crow(r, lane / 32)): same scale, mask, maxima, exponentials, per-half sums -- redundantly, no exchange of state
//   C  O^T tiles (16 dims x 16 queries), two per wave: K-step g feeds keys (crow(2g,0), crow(2g,1), crow(2g+1,0), crow(2g+1,1))
//      = steps 2g, 2g+1 of the wide kernel; the running rescale by alpha is a separate multiplication there and here.
// Bit-identical to lg_attn_kernel<64, 256> (tests/test_lightglue_gpu.py::test_lightglue_small_grid_kernels_equal_the_large_grid_kernels).
// ------------------------------------------------------------------------------------------
constexpr int A16_KP = 68;  // K rows: [slot k = 0..3][g = 0..15] + 4 floats of padding
constexpr int A16_VP = 68;  // V rows: 64 dims + 4
constexpr int A16_SP = 33;  // S / P rows: 32 queries + 1

// Eight waves, two teams: waves 4-7 compute the S^T quadrants of block i + 1 (a chain of 16 dependent matrix steps) while waves
// 0-3 run the softmax and the O^T tiles of block i -- two waves per SIMD whose stalls cover each other; K, V and S are
// double-buffered and a block costs one workgroup barrier.  (Measured on the way, per launch at one pair: all phases in four
// waves with three barriers per block 44 us; the same with phase A moved one block ahead in the SAME waves 47 us; 16 queries per
// workgroup, two workgroups per CU 44 us; lg_attn_kernel 76 us -- profiles/r05_notes.md 5.)
template <int LD>  // row stride of Q / K / V: 256, or 512 when they are column blocks of the merged to_qk | to_v projection
__global__ __launch_bounds__(512) void lg_attn16_kernel(const AttnArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[2][32 * A16_KP];
  __shared__ __attribute__((aligned(16))) float Vs[2][32 * A16_VP];
  __shared__ float Ss[2][32 * A16_SP];
  __shared__ float Ps[4][32 * A16_SP];
  const int qb = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int bk = a.kv_shift ? (b + a.kv_shift) % a.Btot : b;
  const int nq = min(a.nq[b], a.capq), nk = min(a.nk[bk], a.capk);
  const int q0 = qb * 32;
  if (q0 >= nq || nk <= 0) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool team_a = wave >= 4;
  const int w4 = wave & 3;
  const int half = lane >> 5, l31 = lane & 31;  // phase B layout
  const int k4 = lane >> 4, c = lane & 15;      // MFMA 16x16x4 layout: K slot, row / column
  const int kq = w4 >> 1, qq = w4 & 1;          // phase A quadrant: keys 16 kq.., queries 16 qq..
  // Q fragment of phase A: query q0 + 16 qq + c, dims of slot k4 in step order: (k4 & 1) * 32 + 2 g + (k4 >> 1)
  float qf[16];
  {
    const int q = min(q0 + 16 * qq + c, nq - 1);
    const float* Qrow = a.Q + ((size_t)b * a.capq + q) * LD + h * DH + (k4 & 1) * 32 + (k4 >> 1);
#pragma unroll
    for (int g = 0; g < 16; ++g) qf[g] = team_a ? Qrow[2 * g] : 0.0f;
  }
  const float* Kb = a.K + (size_t)bk * a.capk * LD + h * DH;
  const float* Vb = a.V + (size_t)bk * a.capk * LD + h * DH;
  f32x4 o[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) o[t][i] = 0.0f;
  const float NEG = -einx_u2f(0x7f800000u);
  const float sl2 = a.scale * 1.44269504088896341f;
  float m_run = NEG, l_run = 0.0f;
  // staging: 32 keys x 16 float4 per operand = one float4 per thread and operand; rows past nk repeat row nk - 1 (masked in B)
  const int srow = tid >> 4, sc4 = tid & 15;
  auto load_row = [&](const float* base, int kb0) {
    return *reinterpret_cast<const f32x4*>(base + (size_t)min(kb0 + srow, nk - 1) * LD + sc4 * 4);
  };
  auto commit_k = [&](float* dst, const f32x4& r) {  // dims d0 .. d0+3 (d0 = 4 sc4): slot (d >= 32) + 2 (d & 1), position (d & 31) >> 1
    const int hi = sc4 >> 3, g0 = (sc4 & 7) * 2;
    float* kr = dst + srow * A16_KP;
    kr[hi * 16 + g0] = r[0];
    kr[hi * 16 + g0 + 1] = r[2];
    kr[(hi + 2) * 16 + g0] = r[1];
    kr[(hi + 2) * 16 + g0 + 1] = r[3];
  };
  auto commit_v = [&](float* dst, const f32x4& r) { *reinterpret_cast<f32x4*>(dst + srow * A16_VP + sc4 * 4) = r; };
  // phase A of one block: this wave's S^T quadrant from ks into ss
  auto phase_a = [&](const float* ks, float* ss) {
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* kr = ks + (16 * kq + c) * A16_KP + k4 * 16;
    f32x4 kf[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) kf[u] = *reinterpret_cast<const f32x4*>(kr + 4 * u);
#pragma unroll
    for (int g = 0; g < 16; ++g) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[g >> 2][g & 3], qf[g], acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) ss[(16 * kq + 4 * k4 + i) * A16_SP + 16 * qq + c] = acc[i];
  };
  const int nblk = (nk + 31) >> 5;
  // K / V rows travel global -> registers -> LDS with TWO blocks of flight time (a block is ~1 us, an L2 round trip under this
  // access pattern about as long: with one block of distance the loop waited ~9 us per launch for its loads)
  f32x4 rk, rv, rk_new, rv_new;
  {  // prologue: K(0), V(0), K(1) staged, K(2) and V(1) requested; S(0) computed
    const f32x4 r0 = load_row(Kb, 0);
    rv = load_row(Vb, 0);
    rk = load_row(Kb, 32);
    commit_k(Ks[0], r0);
    commit_v(Vs[0], rv);
    commit_k(Ks[1], rk);
    rk = load_row(Kb, 64);
    rv = load_row(Vb, 32);
    __syncthreads();
    if (team_a) phase_a(Ks[0], Ss[0]);
    __syncthreads();
  }
  float* Pw = Ps[w4];
  for (int blk = 0; blk < nblk; ++blk) {
    const int cur = blk & 1, nxt = cur ^ 1;
    const int kbase = blk * 32;
    // requested one block ago, committed at the end of this one: K(blk + 2) -> Ks[cur], V(blk + 1) -> Vs[nxt]; requested now for
    // the next iteration's commit: K(blk + 3), V(blk + 2)
    const bool more1 = blk + 1 < nblk, more2 = blk + 2 < nblk;
    rk_new = load_row(Kb, kbase + 96);
    rv_new = load_row(Vb, kbase + 64);
    if (team_a) {
      // ---- A of the NEXT block
      if (more1) phase_a(Ks[nxt], Ss[nxt]);
    } else {
      // ---- B: the block's online softmax, as in lg_attn_kernel (lane = query l31, keys crow(r, half)); every wave of the team
      // redoes it for all 32 queries (no exchange of state)
      const float* ss = Ss[cur];
      float s[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = ss[crow(r, half) * A16_SP + l31];
      // phase C's V operands do not depend on the softmax: requested with the S values (one LDS round trip for both)
      const float* vs = Vs[cur];
      float vfr[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) vfr[g] = vs[crow(2 * g + (k4 >> 1), k4 & 1) * A16_VP + 16 * w4 + c];
      __builtin_amdgcn_sched_barrier(0);
      float mx = NEG;
      if (kbase + 32 <= nk) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[r] = s[r] * sl2;
          mx = fmaxf(mx, s[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kbase + crow(r, half);
          s[r] = key < nk ? s[r] * sl2 : NEG;
          mx = fmaxf(mx, s[r]);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      float psum = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = __builtin_amdgcn_exp2f(s[r] - m_new);
        psum += s[r];
      }
      l_run = l_run * alpha + psum;
      m_run = m_new;
#pragma unroll
      for (int r = 0; r < 16; ++r) Pw[crow(r, half) * A16_SP + l31] = s[r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the wave's own LDS writes -> its own reads (in-order LDS)
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // ---- C: O^T tiles (dims 16 w4 .., queries 16 t ..)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float al = __shfl(alpha, 16 * t + c, 64);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[t][i] *= al;
      }
      float pr[8][2];  // all P operands in one batch (the chain of matrix steps then runs without LDS waits)
#pragma unroll
      for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t) pr[g][t] = Pw[crow(2 * g + (k4 >> 1), k4 & 1) * A16_SP + 16 * t + c];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(vfr[g], pr[g][t], o[t], 0, 0, 0);
    }
    // Ks[cur] was last read by phase A of THIS block (previous iteration, before its barrier); Vs[nxt] by phase C of the previous block
    if (more2) commit_k(Ks[cur], rk);
    if (more1) commit_v(Vs[nxt], rv);
    rk = rk_new;
    rv = rv_new;
    __syncthreads();
  }
  if (team_a) return;
  const float l = l_run + __shfl_xor(l_run, 32, 64);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float lq = __shfl(l, 16 * t + c, 64);
    const int q = q0 + 16 * t + c;
    if (q < nq) {
      float* orow = a.O + ((size_t)b * a.capq + q) * D + h * DH + 16 * w4 + 4 * k4;
      *reinterpret_cast<f32x4*>(orow) = f32x4{o[t][0] / lq, o[t][1] / lq, o[t][2] / lq, o[t][3] / lq};
    }
  }
}

// ------------------------------------------------------------------------------------------
// `flash: True` (reference lightglue.py:206-230, :293-314): the same fused attention with q, k, v rounded to binary16
// (round to nearest even, v_cvt_f16_f32: what tensor.half() does, overflow -> inf), both products on v_mfma_f32_32x32x16_f16 with
// fp32 accumulation, the context rounded to binary16 and widened again.  Same work split, tails and orientation as lg_attn_kernel
// (one workgroup = 128 queries of one (pair, head), a wave = 32 queries, S^T = K Q^T with the query on the MFMA column, online
// softmax in base 2 per lane); what differs:
//   * Q / K / V are fp32 in memory and converted on the way in: Q into 8-element fp16 fragments in registers (k-step t of the first
//     product = head dims 16 t + 8 (lane >> 5) + j), K / V into LDS as fp16, 64 keys per round (the bytes of 32 fp32 keys).
//   * K rows [key][dim] with a pitch of HD + 8 halves: a lane's fragment is one 16-byte read, the pitch in words is 4 (mod 8), so
//     the rows of 16 consecutive lanes start on 16 distinct 4-bank groups: conflict-free.
//   * The 16 accumulator registers of S^T hold the keys (r & 3) + 8 (r >> 2) + 4 (lane >> 5); registers 8 s .. 8 s + 7, rounded to
//     fp16, are the B fragment of k-step s of O^T = V^T P^T, whose element j then stands for key 16 s + 8 (j >> 2) + 4 (lane >> 5)
//     + (j & 3) of the 32-key block.  CHOSEN: V is staged TRANSPOSED, Vt[dim][key], with the keys of a block stored in that order
//     (position = key with bits 2 and 3 exchanged), so that V^T's A fragment is one 16-byte read as well -- no transposing read, no
//     exchange of P between lanes.  Reads: pitch AKF + 8 halves = 36 words, 4 (mod 8): conflict-free like K.  Writes: a thread
//     packs (key, key + 1) of one dim into a word, four words per float4 pair; a wave's 64 words of one store go to 16 dim rows x 4
//     key pairs whose rows are 144 words apart (16 mod 64): 16 distinct banks, a 4-way conflict on 32 stores per round and
//     workgroup (estimated at about 1 % of a round, not measured; the K store is 2-way on four banks).
//   * The probabilities are summed in fp32 before they are rounded for the second product; o / l in fp32 (correctly rounded
//     division), then binary16, then stored as fp32.
// <64, 256>: 137 VGPRs, 18432 bytes of LDS, three workgroups per CU, no scratch in any instantiation (DESIGN.md 8k has the table).
// Measured at 128 stacked entries of 1024 x 1024 keys: 252 us per launch against lg_attn_kernel's 1068 us (profiles/lg_flash_bench.txt).
// ------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

struct AttnF16Args : AttnArgs {
  int ld;  // row stride of Q / K / V when the kernel's DD and LD are 0 (>= d, a multiple of 4)
};

constexpr int AKF = 64;  // keys staged per round
template <int HD, int DD, int LD = 0>
__global__ __launch_bounds__(256) void lg_attn_f16_kernel(const AttnF16Args a) {
  constexpr int KP = HD + 8;   // halves per K row
  constexpr int VP = AKF + 8;  // halves per Vt row
  constexpr int DH = HD;       // (shadows the file-level constant)
  __shared__ __attribute__((aligned(16))) _Float16 Ks[AKF * KP];
  __shared__ __attribute__((aligned(16))) _Float16 Vt[DH * VP];
  const int D = DD ? DD : a.d;
  const int DL = LD ? LD : (DD ? DD : a.ld);  // row stride of Q / K / V
  const int gx = (int)gridDim.x, gy = (int)gridDim.y;
  int item = xcd_contiguous((int)(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z)), gx * gy * (int)gridDim.z);
  const int qb = item % gx;
  item /= gx;
  const int h = item % gy, b = item / gy;
  const int bk = a.kv_shift ? (b + a.kv_shift) % a.Btot : b;
  const int nq = min(a.nq[b], a.capq), nk = min(a.nk[bk], a.capk);
  const int q0 = qb * 128;
  if (q0 >= nq || nk <= 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q = q0 + wave * 32 + l31;
  const bool qv = q < nq;
  const int dhr = DD ? DH : a.dh;  // the head's real width; dims dhr .. HD - 1 read as zero and are not stored
  constexpr int KS = DH / 16;      // k-steps of the first product
  f16x8 qf[KS];
  {
    const float* Qrow = a.Q + ((size_t)b * a.capq + (qv ? q : nq - 1)) * DL + h * dhr + 8 * half;
#pragma unroll
    for (int t = 0; t < KS; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int dim = 16 * t + 8 * half + 4 * u;
        const f32x4 v = (DD || dim < dhr) ? *reinterpret_cast<const f32x4*>(Qrow + 16 * t + 4 * u) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int e = 0; e < 4; ++e) qf[t][4 * u + e] = (_Float16)v[e];
      }
  }
  const float* Kb = a.K + (size_t)bk * a.capk * DL + h * dhr;
  const float* Vb = a.V + (size_t)bk * a.capk * DL + h * dhr;
  constexpr int OT = DH / 32;  // 32-wide blocks of the output row
  f32x16 o[OT];
#pragma unroll
  for (int mt = 0; mt < OT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[mt][r] = 0.0f;
  const float NEG = -einx_u2f(0x7f800000u);
  const float sl2 = a.scale * 1.44269504088896341f;  // the 1/sqrt(dh) of SDPA on the fp32 product; softmax in base 2
  float m_run = NEG, l_run = 0.0f;

  // staging through registers, one round ahead.  K: float4 = 4 dims of one key.  V: the same float4 of keys 2 p and 2 p + 1
  constexpr int R4 = DH / 4;             // float4 per K / V row
  constexpr int KST = AKF * R4 / 256;    // K float4 per thread and round
  constexpr int VST = KST / 2;           // V key pairs per thread and round
  static_assert(VST >= 1 && DH % 32 == 0, "head dim 32, 64, 128 or 256");
  f32x4 rk[KST], rv[VST][2];
  auto issue = [&](int kb0) {
#pragma unroll
    for (int i = 0; i < KST; ++i) {
      const int fidx = tid + i * 256;
      const int row = fidx / R4, c4 = fidx % R4;
      const int key = min(kb0 + row, nk - 1);  // clamped: rows past nk are masked after the first product
      rk[i] = (DD || c4 * 4 < dhr) ? *reinterpret_cast<const f32x4*>(Kb + (size_t)key * DL + c4 * 4) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int i = 0; i < VST; ++i) {
      const int fidx = tid + i * 256;
      const int kp = fidx / R4, c4 = fidx % R4;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int key = min(kb0 + 2 * kp + e, nk - 1);
        rv[i][e] = (DD || c4 * 4 < dhr) ? *reinterpret_cast<const f32x4*>(Vb + (size_t)key * DL + c4 * 4) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < KST; ++i) {
      const int fidx = tid + i * 256;
      const int row = fidx / R4, c4 = fidx % R4;
      const f16x4 v = {(_Float16)rk[i][0], (_Float16)rk[i][1], (_Float16)rk[i][2], (_Float16)rk[i][3]};
      *reinterpret_cast<f16x4*>(Ks + row * KP + c4 * 4) = v;
    }
#pragma unroll
    for (int i = 0; i < VST; ++i) {
      const int fidx = tid + i * 256;
      const int kp = fidx / R4, c4 = fidx % R4;
      const int key = 2 * kp;  // position of a key in its Vt row: bits 2 and 3 exchanged (see above); key + 1 sits next to it
      const int pos = (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f16x2 v = {(_Float16)rv[i][0][e], (_Float16)rv[i][1][e]};
        *reinterpret_cast<f16x2*>(Vt + (c4 * 4 + e) * VP + pos) = v;
      }
    }
  };
  issue(0);
  for (int kb0 = 0; kb0 < nk; kb0 += AKF) {
    __syncthreads();
    commit();
    __syncthreads();
    if (kb0 + AKF < nk) issue(kb0 + AKF);
#pragma unroll
    for (int sub = 0; sub < AKF / 32; ++sub) {
      const int kbase = kb0 + sub * 32;
      if (kbase >= nk) break;
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.0f;
      const _Float16* krow = Ks + (sub * 32 + l31) * KP + 8 * half;
#pragma unroll
      for (int t = 0; t < KS; ++t) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(krow + 16 * t), qf[t], s, 0, 0, 0);
      float mx = NEG;
      if (kbase + 32 <= nk) {  // whole block (uniform): no key mask
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[r] = s[r] * sl2;
          mx = fmaxf(mx, s[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kbase + crow(r, half);
          s[r] = key < nk ? s[r] * sl2 : NEG;
          mx = fmaxf(mx, s[r]);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // 2^(-inf) = 0: masked keys and the first block
      float psum = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = __builtin_amdgcn_exp2f(s[r] - m_new);
        psum += s[r];
      }
      l_run = l_run * alpha + psum;
      m_run = m_new;
      if (__any(alpha != 1.0f)) {  // (wave-uniform; x * 1.0f == x)
#pragma unroll
        for (int mt = 0; mt < OT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[mt][r] *= alpha;
      }
      const _Float16* vrow = Vt + l31 * VP + sub * 32 + 8 * half;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        f16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = (_Float16)s[8 * st + j];
#pragma unroll
        for (int mt = 0; mt < OT; ++mt)
          o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(vrow + 32 * mt * VP + 16 * st), pf, o[mt], 0, 0, 0);
      }
    }
  }
  const float l = l_run + __shfl_xor(l_run, 32, 64);
  if (qv) {
    float* orow = a.O + ((size_t)b * a.capq + q) * D + h * dhr;
#pragma unroll
    for (int mt = 0; mt < OT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (DD || mt * 32 + crow(r, half) < dhr) orow[mt * 32 + crow(r, half)] = (float)(_Float16)(o[mt][r] / l);
  }
}

// LayerNorm(512, eps 1e-5, biased variance) + exact GELU, in place; one wave per token
__global__ __launch_bounds__(256) void lg_ln_gelu_kernel(float* hbuf, const int32_t* cnt, int cap, const float* g, const float* be) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  float* row = hbuf + ((size_t)b * cap + i) * 512;
  float v[8], gv[8], bv[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) v[t] = row[lane + 64 * t];
  // gamma / beta are requested with the row: read next to the stores below they are one L2 round trip per element
  // (the compiler cannot move a load above a store through plain float pointers)
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    gv[t] = g[lane + 64 * t];
    bv[t] = be[lane + 64 * t];
  }
  float s = 0.0f;
#pragma unroll
  for (int t = 0; t < 8; ++t) s += v[t];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  const float mean = s / 512.0f;
  float q = 0.0f;
#pragma unroll
  for (int t = 0; t < 8; ++t) q = fmaf(v[t] - mean, v[t] - mean, q);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
  const float rstd = 1.0f / sqrtf(q / 512.0f + 1e-5f);
#pragma unroll
  for (int t = 0; t < 8; ++t) row[lane + 64 * t] = einx_geluf(fmaf((v[t] - mean) * rstd, gv[t], bv[t]));
}

// the same for any row width that is a multiple of 64 (configurations other than d = 256): lane partial sums over
// columns lane, lane + 64, ... ascending, then the same butterfly
__global__ __launch_bounds__(256) void lg_ln_gelu_any_kernel(float* hbuf, const int32_t* cnt, int cap, int width, const float* g, const float* be) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  float* row = hbuf + ((size_t)b * cap + i) * width;
  float s = 0.0f;
  for (int c = lane; c < width; c += 64) s += row[c];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  const float mean = s / (float)width;
  float q = 0.0f;
  for (int c = lane; c < width; c += 64) q = fmaf(row[c] - mean, row[c] - mean, q);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
  const float rstd = 1.0f / sqrtf(q / (float)width + 1e-5f);
  for (int c = lane; c < width; c += 64) row[c] = einx_geluf(fmaf((row[c] - mean) * rstd, g[c], be[c]));
}

// row . w by one wave: lane l adds the columns l, l + 64, ... in ascending order, then the xor butterfly; every lane gets the sum
__device__ __forceinline__ float wave_row_dot(const float* row, const float* w, int d, int lane) {
  float s = 0.0f;
  for (int c = lane; c < d; c += 64) s = fmaf(row[c], w[c], s);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// where a matchability head's weight and bias come from: the model's one head (w, b), or the head entry b's pair stopped at
// (heads[4 h + 2 / 3], see GemmArgs)
struct MatchHead {
  const float *w, *b;
};
__device__ __forceinline__ MatchHead match_head(int, const float* w, const float* bm) { return {w, bm}; }
__device__ __forceinline__ MatchHead match_head(int b, const float* const* heads, const int32_t* stop, int pairs, int nheads) {
  const int h = head_of(stop, pairs, nheads, b);
  return {heads[4 * h + 2], heads[4 * h + 3]};
}

// matchability logit z = x . w + b per token, plus logsigmoid(z) and logsigmoid(-z); Src...: the arguments of a match_head()
template <typename... Src>
__global__ __launch_bounds__(256) void lg_matchability_kernel(const float* x, const int32_t* cnt, int cap, int d, Src... src, float* cert, float* dust) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const MatchHead h = match_head(b, src...);
  const float s = wave_row_dot(x + ((size_t)b * cap + i) * d, h.w, d, lane);
  if (lane == 0) {
    const float z = s + h.b[0];
    cert[(size_t)b * cap + i] = einx_logsigmoidf(z);
    dust[(size_t)b * cap + i] = einx_logsigmoidf(-z);
  }
}

// ------------------------------------------------------------------------------------------
// Early stopping: the layers run on PRIVATE active counts; a pair that stops gets both of them zeroed, and every
// kernel above skips its rows from then on.
// ------------------------------------------------------------------------------------------
constexpr int LG_MAX_HEADS = 32;
struct HeadTable {
  const float* p[4 * LG_MAX_HEADS];  // per layer: final_proj w, b, matchability w, b
};

// the heads' pointers into device memory (the kernels pick an entry by stop[b]), the private counts, stop and the decision's counters
__global__ void lg_es_init_kernel(const HeadTable t, int nheads, const float** heads, const int32_t* n, const int32_t* m, int B, int cap0, int cap1,
                                  int32_t* cnt2, int32_t* act, int32_t* stop, int32_t* below, int32_t* done) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4 * nheads) heads[i] = t.p[i];
  if (i < 2 * B) {
    const int32_t v = i < B ? n[i] : m[i - B];
    cnt2[i] = v;
    act[i] = v;
  }
  if (i < B) {
    stop[i] = (min(n[i], cap0) > 0 && min(m[i], cap1) > 0) ? nheads : 0;
    below[i] = 0;
    done[i] = 0;
  }
}

// The launches behind a non-final layer (the stop decision, the pruning step) run over 2B entries: entry e < B is side 0 of pair
// e, entry e >= B side 1 of pair e - B.
struct Entry {
  bool side;
  int p, cap;
};
__device__ __forceinline__ Entry entry_of(int e, int B, int cap0, int cap1) {
  const bool side = e >= B;
  return {side, side ? e - B : e, side ? cap1 : cap0};
}

// ... and what their argument blocks share
struct TailArgs {
  float *x0, *x1;  // [B,cap0,d], [B,cap1,d] after the layer
  int32_t* act;    // [2B]: the layers' active counts
  int32_t* stop;
  int cap0, cap1, d, B, layer;
  const float *tw, *tb;  // token_confidence[layer].token[0], or null: no stop decision
  float thr;             // the layer's confidence threshold
};

struct StopArgs {
  TailArgs t;
  float depth;
  int32_t *below, *done;       // [B], zero between launches
  const int32_t *tot0, *tot1;  // null, or the caller's counts: the ratio's denominator when rows have been pruned
};

// One launch per non-final layer: a workgroup takes STOP_ROWS rows of an entry (a wave one row at a time: c = sigmoid(x . w + b),
// compared with the layer's threshold in float32).  The workgroups of a
// pair add their integer counts into below[pair] and take a ticket; the one that takes the last ticket has every count, applies
// r = 1 - below / (n + m) > depth_confidence, writes stop and zeroes the pair's active counts, and leaves the counters at zero.
// Integer sums only: the order in which the workgroups arrive does not matter.  Every workgroup with rows has read the counts
// before it takes its ticket, so none can meet the zeroed counts of its own launch; those without rows return either way.
constexpr int STOP_ROWS = 32;
__global__ __launch_bounds__(256) void lg_stop_kernel(const StopArgs a) {
  __shared__ int part[4];
  const TailArgs& t = a.t;
  const Entry en = entry_of(blockIdx.y, t.B, t.cap0, t.cap1);
  const int p = en.p;
  const int n = min(t.act[p], t.cap0), m = min(t.act[t.B + p], t.cap1);
  if (n <= 0 || m <= 0) return;  // stopped earlier, or an empty pair (stop = 0)
  const int rows = en.side ? m : n;
  const int r0 = (int)blockIdx.x * STOP_ROWS;
  if (r0 >= rows) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* x = (en.side ? t.x1 : t.x0) + (size_t)p * en.cap * t.d;
  const float b0 = t.tb[0];
  int below = 0;
  for (int k = 0; k < STOP_ROWS / 4; ++k) {
    const int i = r0 + wave * (STOP_ROWS / 4) + k;
    if (i >= rows) break;
    const float s = wave_row_dot(x + (size_t)i * t.d, t.tw, t.d, lane);
    below += einx_sigmoidf(s + b0) < t.thr ? 1 : 0;
  }
  if (lane == 0) part[wave] = below;
  __syncthreads();
  if (threadIdx.x != 0) return;
  atomicAdd(&a.below[p], part[0] + part[1] + part[2] + part[3]);
  __threadfence();
  const int expected = einx_cdiv(n, STOP_ROWS) + einx_cdiv(m, STOP_ROWS);
  if (atomicAdd(&a.done[p], 1) != expected - 1) return;
  __threadfence();
  const int total = atomicExch(&a.below[p], 0);
  atomicExch(&a.done[p], 0);
  const int den = a.tot0 ? min(a.tot0[p], t.cap0) + min(a.tot1[p], t.cap1) : n + m;  // the reference divides by the ORIGINAL m + n (:635)
  const float r = 1.0f - (float)total / (float)den;
  if (r > a.depth) {
    t.stop[p] = t.layer + 1;
    t.act[p] = 0;
    t.act[t.B + p] = 0;
  }
}

// ------------------------------------------------------------------------------------------
// Point pruning: per pair and side, rows whose matchability head calls them unmatchable leave the network.  The
// survivors are compacted to the front in their order, and the side's active count shrinks: every kernel above skips the rest.
// Per non-final layer, after the stop decision: lg_keep_kernel (the flags), lg_prune_scan_kernel (one workgroup per pair: new
// positions, ind, prune, the counts), lg_prune_gather_kernel (x and the rotary encoding into buffers that are free between
// layers) and lg_prune_copyback_kernel.  Launch boundaries are the only synchronisation; no float atomics, no atomics at all.
// ------------------------------------------------------------------------------------------
struct PruneArgs {
  TailArgs t;          // tw / tb null: no early stopping, no token term
  float *enc0, *enc1;  // [B,cap,2 dh]
  float *tx0, *tx1;    // where the gather puts x: the sides' ctx
  float *te0, *te1;    // ... and the encoding: the sides' h, rows packed at 2 dh floats from each entry's base
  int32_t *live, *prev;    // [2B] each: the surviving rows, the surviving rows before this layer's step
  int32_t *dst0, *dst1;    // [B,cap0], [B,cap1]: the keep flag, then the row's new position or -1
  int64_t *kept0, *kept1;  // ind: position -> original index; -1 past the live count
  float *prune0, *prune1;
  const int32_t *n, *m;  // the caller's counts
  int dh2, min_kpts, set_stop;
  const float *mw, *mb;  // log_assignment[layer].matchability
  float thr_w;
};

// ind = identity, prune = 1 for every original point (0 in the padding), live = prev = the clamped counts
__global__ void lg_prune_init_kernel(const PruneArgs a) {
  const int e = blockIdx.y;
  const Entry en = entry_of(e, a.t.B, a.t.cap0, a.t.cap1);
  const int p = en.p, cap = en.cap;
  const int cnt = max(0, min(en.side ? a.m[p] : a.n[p], cap));
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) {
    a.live[e] = cnt;
    a.prev[e] = cnt;
  }
  if (t >= cap) return;
  (en.side ? a.kept1 : a.kept0)[(size_t)p * cap + t] = t < cnt ? t : -1;
  (en.side ? a.prune1 : a.prune0)[(size_t)p * cap + t] = t < cnt ? 1.0f : 0.0f;
}

// keep = sigmoid(matchability(x)) > thr_w, or (early stopping on) sigmoid(token(x)) <= thr: the dot products in the order of
// lg_matchability_kernel, one wave per row; grid and entries as lg_stop_kernel.  Pairs that have stopped, and sides that do not
// pass the gate (rows > min_kpts), are left alone.
__global__ __launch_bounds__(256) void lg_keep_kernel(const PruneArgs a) {
  const TailArgs& t = a.t;
  const Entry en = entry_of(blockIdx.y, t.B, t.cap0, t.cap1);
  const int p = en.p, cap = en.cap;
  const int n = min(t.act[p], t.cap0), m = min(t.act[t.B + p], t.cap1);
  if (n <= 0 || m <= 0) return;
  const int rows = en.side ? m : n;
  if (rows <= a.min_kpts) return;
  const int r0 = (int)blockIdx.x * STOP_ROWS;
  if (r0 >= rows) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* x = (en.side ? t.x1 : t.x0) + (size_t)p * cap * t.d;
  int32_t* dst = (en.side ? a.dst1 : a.dst0) + (size_t)p * cap;
  for (int k = 0; k < STOP_ROWS / 4; ++k) {
    const int i = r0 + wave * (STOP_ROWS / 4) + k;
    if (i >= rows) break;
    const float* row = x + (size_t)i * t.d;
    bool keep = einx_sigmoidf(wave_row_dot(row, a.mw, t.d, lane) + a.mb[0]) > a.thr_w;
    if (t.tw) {  // low-confidence points are never pruned (lightglue.py:728-729)
      const float c = wave_row_dot(row, t.tw, t.d, lane);
      keep = keep || einx_sigmoidf(c + t.tb[0]) <= t.thr;
    }
    if (lane == 0) dst[i] = keep ? 1 : 0;
  }
}

// One workgroup per pair, its two sides one after the other: an exclusive scan of the flags in chunks of 256 rows gives every kept
// row its new position (stable).  ind is compacted in place -- a chunk is read by every thread before any of it is written, and
// a row only moves forward, into places the earlier chunks have left -- and prune[ind] grows by one for the rows that stay.  Then
// the counts: live = act = the rows kept; a side with no rows left finishes the pair (both active counts zero, stop = layer + 1
// when early stopping is on).  prev keeps what live was, so that the two launches behind this one know which sides moved.
__global__ __launch_bounds__(256) void lg_prune_scan_kernel(const PruneArgs a) {
  __shared__ int wsum[4];
  const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = min(a.t.act[p], a.t.cap0), m = min(a.t.act[a.t.B + p], a.t.cap1);
  if (tid == 0) {
    a.prev[p] = a.live[p];
    a.prev[a.t.B + p] = a.live[a.t.B + p];
  }
  if (n <= 0 || m <= 0) return;  // stopped, finished or empty (uniform over the workgroup)
  int newc[2] = {n, m};
  for (int side = 0; side < 2; ++side) {
    const int rows = side ? m : n, cap = side ? a.t.cap1 : a.t.cap0;
    if (rows <= a.min_kpts) continue;  // the gate: untouched at this layer, prune not incremented
    int32_t* dst = (side ? a.dst1 : a.dst0) + (size_t)p * cap;
    int64_t* kept = (side ? a.kept1 : a.kept0) + (size_t)p * cap;
    float* prune = (side ? a.prune1 : a.prune0) + (size_t)p * cap;
    int run = 0;
    for (int base = 0; base < rows; base += 256) {
      const int i = base + tid;
      const int flag = i < rows ? dst[i] : 0;
      const int64_t src = i < rows ? kept[i] : -1;
      const unsigned long long bal = __ballot(flag != 0);
      const int within = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wsum[wave] = __popcll(bal);
      __syncthreads();
      int off = run, total = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w < wave) off += wsum[w];
        total += wsum[w];
      }
      __syncthreads();
      if (i < rows) {
        dst[i] = flag ? off + within : -1;
        if (flag) {
          kept[off + within] = src;
          prune[src] += 1.0f;
        }
      }
      run += total;
    }
    __syncthreads();
    for (int i = run + tid; i < rows; i += 256) kept[i] = -1;
    newc[side] = run;
  }
  if (tid != 0) return;
  a.live[p] = newc[0];
  a.live[a.t.B + p] = newc[1];
  const bool finished = newc[0] == 0 || newc[1] == 0;
  a.t.act[p] = finished ? 0 : newc[0];
  a.t.act[a.t.B + p] = finished ? 0 : newc[1];
  if (finished && a.set_stop) a.t.stop[p] = a.t.layer + 1;
}

// the rows that stay, of the sides that lost rows at this layer: x -> tx, enc -> te at the new position; one wave per row
__global__ __launch_bounds__(256) void lg_prune_gather_kernel(const PruneArgs a) {
  const int e = blockIdx.y;
  const int old = a.prev[e];
  if (a.live[e] == old) return;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= old) return;
  const Entry en = entry_of(e, a.t.B, a.t.cap0, a.t.cap1);
  const bool side = en.side;
  const int p = en.p, cap = en.cap;
  const int j = (side ? a.dst1 : a.dst0)[(size_t)p * cap + i];
  if (j < 0) return;
  const int lane = threadIdx.x & 63;
  const size_t xb = (size_t)p * cap * a.t.d, eb = (size_t)p * cap * a.dh2;
  const float* xs = (side ? a.t.x1 : a.t.x0) + xb + (size_t)i * a.t.d;
  float* xd = (side ? a.tx1 : a.tx0) + xb + (size_t)j * a.t.d;
  for (int c = lane * 4; c < a.t.d; c += 256) *reinterpret_cast<f32x4*>(xd + c) = *reinterpret_cast<const f32x4*>(xs + c);
  const float* es = (side ? a.enc1 : a.enc0) + eb + (size_t)i * a.dh2;
  float* ed = (side ? a.te1 : a.te0) + (size_t)p * cap * 2 * a.t.d + (size_t)j * a.dh2;
  for (int c = lane * 4; c < a.dh2; c += 256) *reinterpret_cast<f32x4*>(ed + c) = *reinterpret_cast<const f32x4*>(es + c);
}

// ... and back: the first live rows of x and enc (16 bytes per thread; the x part, then the enc part of an entry)
__global__ __launch_bounds__(256) void lg_prune_copyback_kernel(const PruneArgs a) {
  const int e = blockIdx.y;
  const int nw = a.live[e];
  if (nw == a.prev[e]) return;
  const Entry en = entry_of(e, a.t.B, a.t.cap0, a.t.cap1);
  const bool side = en.side;
  const int p = en.p, cap = en.cap;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t xq = (size_t)cap * (a.t.d / 4), eq = (size_t)cap * (a.dh2 / 4);
  if (t < xq) {
    if (t >= (size_t)nw * (a.t.d / 4)) return;
    const size_t o = (size_t)p * cap * a.t.d + t * 4;
    *reinterpret_cast<f32x4*>((side ? a.t.x1 : a.t.x0) + o) = *reinterpret_cast<const f32x4*>((side ? a.tx1 : a.tx0) + o);
  } else if (t - xq < eq) {
    const size_t u = t - xq;
    if (u >= (size_t)nw * (a.dh2 / 4)) return;
    *reinterpret_cast<f32x4*>((side ? a.enc1 : a.enc0) + (size_t)p * cap * a.dh2 + u * 4) =
        *reinterpret_cast<const f32x4*>((side ? a.te1 : a.te0) + (size_t)p * cap * 2 * a.t.d + u * 4);
  }
}

// a packed arg-max key (pack_key, match_tiles.h) back into its index and its value
__device__ __forceinline__ int key_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)); }
__device__ __forceinline__ float key_value(unsigned long long k) { return einx_ordered_unkey((unsigned)(k >> 32)); }

// filter_matches (lightglue.py:402-418) from the packed arg-max keys of the assignment scores
__global__ void lg_finalize_kernel(const unsigned long long* rowkey, const unsigned long long* colkey, const int32_t* nn, const int32_t* mm,
                                   int cap0, int cap1, float th, int64_t* m0, int64_t* m1, float* s0, float* s1) {
  const int b = blockIdx.y;
  const int n = min(nn[b], cap0), m = min(mm[b], cap1);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long* rk = rowkey + (size_t)b * cap0;
  const unsigned long long* ck = colkey + (size_t)b * cap1;
  if (t < cap0) {
    int64_t r = -1;
    float sc = 0.0f;
    if (t < n && m > 0) {
      const int j = key_index(rk[t]);
      const bool mutual = key_index(ck[j]) == t;
      sc = mutual ? einx_expf(key_value(rk[t])) : 0.0f;
      if (mutual && sc > th) r = j;
    }
    m0[(size_t)b * cap0 + t] = r;
    s0[(size_t)b * cap0 + t] = sc;
  }
  if (t < cap1) {
    int64_t r = -1;
    float sc = 0.0f;
    if (t < m && n > 0) {
      const int i = key_index(ck[t]);
      const int back = key_index(rk[i]);
      const bool mutual1 = back == t;
      // mscores1 = mscores0[m1] where mutual1; mscores0[i] is non-zero only if i is mutual too,
      // which is the same condition (back == t  <=>  i's best is t and t's best is i)
      const float ms0 = mutual1 ? einx_expf(key_value(rk[i])) : 0.0f;
      sc = ms0;
      if (mutual1 && ms0 > th) r = i;
    }
    m1[(size_t)b * cap1 + t] = r;
    s1[(size_t)b * cap1 + t] = sc;
  }
}

// The same after point pruning: the keys are those of the LIVE rows, and the results go back to original indexing
// through ind (lightglue.py:659-667).  One workgroup per pair: every row gets -1 / 0 first, then the live rows scatter.
__global__ __launch_bounds__(256) void lg_finalize_scatter_kernel(const unsigned long long* rowkey, const unsigned long long* colkey, const int32_t* live,
                                                                  int B, const int64_t* kept0, const int64_t* kept1, int cap0, int cap1, float th,
                                                                  int64_t* m0, int64_t* m1, float* s0, float* s1) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(live[b], cap0), m = min(live[B + b], cap1);
  m0 += (size_t)b * cap0;
  s0 += (size_t)b * cap0;
  m1 += (size_t)b * cap1;
  s1 += (size_t)b * cap1;
  for (int t = tid; t < cap0; t += 256) {
    m0[t] = -1;
    s0[t] = 0.0f;
  }
  for (int t = tid; t < cap1; t += 256) {
    m1[t] = -1;
    s1[t] = 0.0f;
  }
  __syncthreads();
  if (n <= 0 || m <= 0) return;
  const unsigned long long* rk = rowkey + (size_t)b * cap0;
  const unsigned long long* ck = colkey + (size_t)b * cap1;
  const int64_t* i0 = kept0 + (size_t)b * cap0;
  const int64_t* i1 = kept1 + (size_t)b * cap1;
  for (int t = tid; t < n; t += 256) {
    const int j = key_index(rk[t]);
    const bool mutual = key_index(ck[j]) == t;
    const float sc = mutual ? einx_expf(key_value(rk[t])) : 0.0f;
    m0[i0[t]] = (mutual && sc > th) ? i1[j] : -1;
    s0[i0[t]] = sc;
  }
  for (int t = tid; t < m; t += 256) {
    const int i = key_index(ck[t]);
    const bool mutual1 = key_index(rk[i]) == t;
    const float ms0 = mutual1 ? einx_expf(key_value(rk[i])) : 0.0f;
    m1[i1[t]] = (mutual1 && ms0 > th) ? i0[i] : -1;
    s1[i1[t]] = ms0;
  }
}

// dst_bstride: elements between consecutive batches of dst (cap*width for a plain [B,cap,width] copy)
__global__ void lg_copy_rows_kernel(const float* src, float* dst, const int32_t* cnt, int cap, int width, size_t dst_bstride) {
  const int b = blockIdx.y;
  const int n = min(cnt[b], cap);
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * width) return;
  dst[(size_t)b * dst_bstride + t] = src[(size_t)b * cap * width + t];
}

// normalize_keypoints (lightglue.py:137-148): (kpt - size/2) / (max(size)/2), first two columns
__global__ void lg_normalize_kpts_kernel(const float* kpts, int cols, size_t total, float s0, float s1, float* out, int out_cols) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const float sc = fmaxf(s0, s1) / 2.0f;
  out[t * out_cols + 0] = (kpts[t * cols + 0] - s0 / 2.0f) / sc;
  out[t * out_cols + 1] = (kpts[t * cols + 1] - s1 / 2.0f) / sc;
  for (int c = 2; c < out_cols; ++c) out[t * out_cols + c] = 0.0f;
}

struct Side {
  const float* kpts;
  const float* desc;
  const int32_t* cnt;
  int cap;
  float *x, *enc, *q, *k, *v, *ctx, *msg, *h, *cert, *dust;
};

// The three entries share one driver (lg_run): einx_lightglue, einx_lightglue_early_stop and
// einx_lightglue_adaptive (8j: point pruning, with or without the stop decision).  Each mode's workspace is the one before it
// plus a block of its own.
enum LgMode { LG_PLAIN = 0, LG_EARLY_STOP = 1, LG_ADAPTIVE = 2 };

struct LgShape {
  int B, cap0, cap1, d, dh, n_layers;  // d: descriptor_dim, dh: head dim
  // equal capacities (every shipped configuration): the two sides are stacked and every layer runs ONCE over 2B entries --
  // half the launches, and at small batch twice the workgroups per launch (a single pair: 8.0 -> see profiles/r03_notes.md)
  bool stacked() const { return cap0 == cap1; }
};

struct LgWs {
  Side s[2];
  int32_t* cnt2;  // the caller's counts of both sides as [2B] (written when stacked, or by the early-stop init)
  MnnArgs mnn;
  // early stopping
  const float** heads;          // [4 n_layers] device table
  int32_t *act, *below, *done;  // private active counts [2B]; the decision's counters [B] each
  // point pruning
  int32_t *dst0, *dst1;  // [B,cap0], [B,cap1]
  int32_t *prev, *stop;  // [2B]; [B], used when the caller passes no stop
};

// The workspace of all three entries (their size queries walk it from a null base).  Per side the buffers [tokens, d] (x, q, k,
// v, ctx, msg), [tokens, 2 dh] (enc), [tokens, 2 d] (h), [tokens] (cert, dust); then the stacked counts, the assignment stage's
// MNN workspace (match_tiles.h) and 1024 bytes of slack; then the early-stop block, then the pruning block, 256 bytes of slack
// each.  Stacked (equal capacities): every buffer is ONE array [2B, cap, width], side 0 = entries 0..B-1, side 1 = entries
// B..2B-1.  LightGlue applies the same weights to both sides, so every per-side launch becomes one launch over 2B entries (cross
// attention reaches the partner entry B entries on); s[0] / s[1] stay views of the halves.  The array lies in the two regions
// that its halves would take apart, side 1 directly behind side 0's last element: rounding each half up never gives less than the
// whole needs, so the size does not depend on `stacked`.
void carve(WsCarver& c, LgWs& w, LgMode mode, const LgShape& sh) {
  const size_t B = (size_t)sh.B, d = (size_t)sh.d;
  const struct {
    float* Side::*buf;
    size_t width;  // floats per token
  } bufs[] = {{&Side::x, d},   {&Side::enc, (size_t)2 * sh.dh}, {&Side::q, d},     {&Side::k, d},     {&Side::v, d},
              {&Side::ctx, d}, {&Side::msg, d},                 {&Side::h, 2 * d}, {&Side::cert, 1}, {&Side::dust, 1}};
  if (sh.stacked()) {
    for (const auto& b : bufs) {
      const size_t n = B * sh.cap0 * b.width;
      float* both = c.take<float>(n);
      c.take<float>(n);
      w.s[0].*b.buf = both;
      w.s[1].*b.buf = both ? both + n : nullptr;
    }
  } else {
    for (const auto& b : bufs) w.s[0].*b.buf = c.take<float>(B * sh.cap0 * b.width);
    for (const auto& b : bufs) w.s[1].*b.buf = c.take<float>(B * sh.cap1 * b.width);
  }
  w.cnt2 = c.take<int32_t>(2 * B);
  einx_match::carve(c, w.mnn, sh.B, sh.cap0, sh.cap1);
  c.slack(1024);
  if (mode == LG_PLAIN) return;
  w.heads = c.take<const float*>((size_t)4 * sh.n_layers);
  w.act = c.take<int32_t>(2 * B);
  w.below = c.take<int32_t>(B);
  w.done = c.take<int32_t>(B);
  c.slack(256);
  if (mode == LG_EARLY_STOP) return;
  w.dst0 = c.take<int32_t>(B * sh.cap0);
  w.dst1 = c.take<int32_t>(B * sh.cap1);
  w.prev = c.take<int32_t>(2 * B);
  w.stop = c.take<int32_t>(B);
  c.slack(256);
}

__global__ void lg_stack_counts_kernel(const int32_t* n, const int32_t* m, int B, int32_t* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 2 * B) out[t] = t < B ? n[t] : m[t - B];
}

// persistent launch size: resident workgroups of the tile kernels on this device (a multiple of
// 8 so that every XCD gets the same number of slots), never more than the tiles there are
template <typename Eng = EngF32>
unsigned gemm_grid(int tiles) {
  static int resident = 0;  // (one per engine)
  if (resident == 0) {
    int dev = 0, cus = 256, per_cu = 2;
    if (hipGetDevice(&dev) == hipSuccess) {
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lg_gemm_kernel<EPI_BIAS, Eng>, THREADS, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    }
    resident = (cus * per_cu) & ~7;
    if (resident < 8) resident = 8;
  }
  const int want = (tiles + 7) & ~7;
  return (unsigned)(want < resident ? want : resident);
}

// fewer 128x128 tiles than CUs (and shapes the small kernel takes): 64x64 tiles, one per workgroup
bool small_grid(int N, int cap, int B, int K, int Ksplit) {
  const long max_tiles = 256;
  const long tiles = (long)einx_cdiv(N, BN) * einx_cdiv(cap, BM) * B;
  return tiles < max_tiles && K % SBK == 0 && N % SBN == 0 && (Ksplit >= K || Ksplit % SBK == 0);
}

// W16: null, or the binary16 image of W: the launch then runs the f16 tile engine (`mp: True`; EPI_BIAS / EPI_RESID
// only, one kernel for every grid size -- no f16 twin of lg_gemm_small_kernel)
int gemm(hipStream_t st, int epi, const Side& s, int B, const float* X, int ldx, const float* X2, int ldx2, int Ksplit, int K, const float* W,
         const float* bias, int N, float* Y, int ldy, float div = 1.0f, const float* const* heads = nullptr, const int32_t* stop = nullptr,
         int pairs = 0, int nheads = 0, const uint16_t* W16 = nullptr) {
  GemmArgs g;
  g.heads = heads;
  g.stop = stop;
  g.pairs = pairs;
  g.nheads = nheads;
  g.X = X;
  g.X2 = X2;
  g.W = W;
  g.bias = bias;
  g.Y = Y;
  g.cnt = s.cnt;
  g.cap = s.cap;
  g.ldx = ldx;
  g.ldx2 = ldx2;
  g.Ksplit = Ksplit;
  g.K = K;
  g.N = N;
  g.ldy = ldy;
  g.div = div;
  g.B = B;
  if (W16) {
    if (epi != EPI_BIAS && epi != EPI_RESID) return -1;
    g.W = reinterpret_cast<const float*>(W16);
    const dim3 grid(gemm_grid<EngF16>(einx_cdiv(N, BN) * einx_cdiv(s.cap, BM) * B));
    EINX_PROF("lg_gemm_kernel (f16)", st);
    if (epi == EPI_BIAS) hipLaunchKernelGGL((lg_gemm_kernel<EPI_BIAS, EngF16>), grid, dim3(THREADS), 0, st, g);
    else hipLaunchKernelGGL((lg_gemm_kernel<EPI_RESID, EngF16>), grid, dim3(THREADS), 0, st, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  if (small_grid(N, s.cap, B, K, Ksplit)) {
    const dim3 sg((unsigned)(N / SBN), (unsigned)einx_cdiv(s.cap, SBM), (unsigned)B);
    EINX_PROF("lg_gemm_small_kernel", st);
    if (epi == EPI_BIAS) hipLaunchKernelGGL(lg_gemm_small_kernel<EPI_BIAS>, sg, dim3(256), 0, st, g);
    else if (epi == EPI_DIV) hipLaunchKernelGGL(lg_gemm_small_kernel<EPI_DIV>, sg, dim3(256), 0, st, g);
    else if (epi == EPI_DIV_HEAD) hipLaunchKernelGGL(lg_gemm_small_kernel<EPI_DIV_HEAD>, sg, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(lg_gemm_small_kernel<EPI_RESID>, sg, dim3(256), 0, st, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  const dim3 grid(gemm_grid<>(einx_cdiv(N, BN) * einx_cdiv(s.cap, BM) * B));
  EINX_PROF("lg_gemm_kernel", st);
  if (epi == EPI_BIAS) hipLaunchKernelGGL(lg_gemm_kernel<EPI_BIAS>, grid, dim3(THREADS), 0, st, g);
  else if (epi == EPI_DIV) hipLaunchKernelGGL(lg_gemm_kernel<EPI_DIV>, grid, dim3(THREADS), 0, st, g);
  else if (epi == EPI_DIV_HEAD) hipLaunchKernelGGL(lg_gemm_kernel<EPI_DIV_HEAD>, grid, dim3(THREADS), 0, st, g);
  else hipLaunchKernelGGL(lg_gemm_kernel<EPI_RESID>, grid, dim3(THREADS), 0, st, g);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the mode bits of einx_lightglue_mp (einx.h: EINX_LG_ATTN_F16, EINX_LG_LIN_F16)
enum { LG_ATTN_F16 = 1, LG_LIN_F16 = 2 };

// the model's widths and precision modes, as the launchers need them
struct Dims {
  int d, heads, dh;
  bool flash = false;  // LG_ATTN_F16: attention in fp16 on the matrix cores (conf.flash)
  bool lin16 = false;  // LG_LIN_F16: the layers' linears on the f16 tile engine (conf.mp)
  bool shipped() const { return d == D && dh == DH; }
};

// fused Wqkv projection + rotary split: X [B,cap,d] -> q, k (rotary applied), v, each [B,cap,d]
int gemm_qkv_rope(hipStream_t st, const Side& s, int B, const Dims& dm, const float* X, const float* Wqkv, const uint16_t* Wqkv16, const float* bqkv,
                  float* q, float* k, float* v) {
  const int d = dm.d;
  GemmArgs g{};
  g.X = X;
  g.X2 = nullptr;
  g.W = Wqkv;
  g.bias = bqkv;
  g.Y = nullptr;
  g.cnt = s.cnt;
  g.cap = s.cap;
  g.ldx = d;
  g.ldx2 = 0;
  g.Ksplit = 0x7fffffff;
  g.K = d;
  g.N = 3 * d;
  g.ldy = d;
  g.div = 1.0f;
  g.B = B;
  g.enc = s.enc;
  g.Yq = q;
  g.Yk = k;
  g.Yv = v;
  g.d = dm.d;
  g.dh = dm.dh;
  const int tiles = 3 * einx_cdiv(d, BN) * einx_cdiv(s.cap, BM) * B;  // three blocks (q | k | v) of whole tiles each
  if (dm.lin16) {
    if (!Wqkv16) return -1;
    g.W = reinterpret_cast<const float*>(Wqkv16);
    const dim3 grid(gemm_grid<EngF16>(tiles));
    EINX_PROF("lg_gemm_kernel (f16)", st);
    if (dm.shipped()) hipLaunchKernelGGL((lg_gemm_kernel<EPI_ROPE, EngF16>), grid, dim3(THREADS), 0, st, g);
    else hipLaunchKernelGGL((lg_gemm_kernel<EPI_ROPE_ANY, EngF16>), grid, dim3(THREADS), 0, st, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  if (tiles < 256 && d % SBN == 0 && d % SBK == 0) {  // as small_grid()
    const dim3 sg((unsigned)(3 * d / SBN), (unsigned)einx_cdiv(s.cap, SBM), (unsigned)B);
    EINX_PROF("lg_gemm_small_kernel", st);
    if (dm.shipped()) hipLaunchKernelGGL(lg_gemm_small_kernel<EPI_ROPE>, sg, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(lg_gemm_small_kernel<EPI_ROPE_ANY>, sg, dim3(256), 0, st, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  const dim3 grid(gemm_grid<>(tiles));
  EINX_PROF("lg_gemm_kernel", st);
  if (dm.shipped()) hipLaunchKernelGGL(lg_gemm_kernel<EPI_ROPE>, grid, dim3(THREADS), 0, st, g);
  else hipLaunchKernelGGL(lg_gemm_kernel<EPI_ROPE_ANY>, grid, dim3(THREADS), 0, st, g);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// conf.flash: one kernel for every grid size (no fp16 twin of lg_attn16_kernel); ld: row stride of Q / K / V
int attn_f16(hipStream_t st, dim3 grid, const Dims& dm, const AttnArgs& base, int ld) {
  AttnF16Args a;
  static_cast<AttnArgs&>(a) = base;
  a.ld = ld;
  EINX_PROF("lg_attn_f16_kernel", st);
  if (dm.shipped() && ld == 2 * D) hipLaunchKernelGGL((lg_attn_f16_kernel<64, D, 2 * D>), grid, dim3(256), 0, st, a);
  else if (dm.shipped() && ld == D) hipLaunchKernelGGL((lg_attn_f16_kernel<64, D>), grid, dim3(256), 0, st, a);
  else if (dm.dh <= 32) hipLaunchKernelGGL((lg_attn_f16_kernel<32, 0>), grid, dim3(256), 0, st, a);  // (narrower heads: zero padded)
  else if (dm.dh <= 64) hipLaunchKernelGGL((lg_attn_f16_kernel<64, 0>), grid, dim3(256), 0, st, a);
  else if (dm.dh <= 128) hipLaunchKernelGGL((lg_attn_f16_kernel<128, 0>), grid, dim3(256), 0, st, a);
  else if (dm.dh <= 256) hipLaunchKernelGGL((lg_attn_f16_kernel<256, 0>), grid, dim3(256), 0, st, a);
  else return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// merged: Q, K, V are column blocks of a [.., 2 d] buffer (row stride 512; shipped widths only)
int attn(hipStream_t st, int B, const Dims& dm, const float* Q, const int32_t* nq, int capq, const float* K, const float* V, const int32_t* nk,
         int capk, float* O, int kv_shift = 0, bool merged = false) {
  AttnArgs a;
  a.kv_shift = kv_shift;
  a.Btot = B;
  a.Q = Q;
  a.K = K;
  a.V = V;
  a.O = O;
  a.nq = nq;
  a.nk = nk;
  a.capq = capq;
  a.capk = capk;
  a.d = dm.d;
  a.dh = dm.dh;
  a.scale = 1.0f / sqrtf((float)dm.dh);  // SDPA scale (self) = (dh^-1/4)^2 (cross, lightglue.py:316); 64-wide heads: exactly 0.125
  const dim3 grid((unsigned)einx_cdiv(capq, 128), (unsigned)dm.heads, (unsigned)B);
  if (dm.flash) return attn_f16(st, grid, dm, a, merged ? 2 * dm.d : dm.d);
  EINX_PROF("lg_attn_kernel", st);
  // the latency form (same bits) while ITS grid fits the chip twice: fewer wide workgroups than CUs alone is not enough -- three
  // pairs of 1024 keypoints (768 latency-form workgroups of eight waves, 1.5 rounds) ran 3.67 instead of 3.26 ms; one pair
  // 1.82 instead of 2.39 ms, two pairs 2.51 instead of 2.68 (tools/lg_bench.py --batch 1 / 2 / 3 --skip-linear)
  if (dm.shipped() && (long)grid.x * grid.y * grid.z < 256 && (long)einx_cdiv(capq, 32) * dm.heads * B <= 512) {
    const dim3 g16((unsigned)einx_cdiv(capq, 32), (unsigned)dm.heads, (unsigned)B);
    if (merged) hipLaunchKernelGGL(lg_attn16_kernel<2 * D>, g16, dim3(512), 0, st, a);
    else hipLaunchKernelGGL(lg_attn16_kernel<D>, g16, dim3(512), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  if (merged && !dm.shipped()) return -1;
  if (merged) hipLaunchKernelGGL((lg_attn_kernel<64, D, 2 * D>), grid, dim3(256), 0, st, a);
  else if (dm.shipped()) hipLaunchKernelGGL((lg_attn_kernel<64, D>), grid, dim3(256), 0, st, a);
  else if (dm.dh <= 32) hipLaunchKernelGGL((lg_attn_kernel<32, 0>), grid, dim3(256), 0, st, a);  // (narrower heads: zero padded)
  else if (dm.dh <= 64) hipLaunchKernelGGL((lg_attn_kernel<64, 0>), grid, dim3(256), 0, st, a);
  else if (dm.dh <= 128) hipLaunchKernelGGL((lg_attn_kernel<128, 0>), grid, dim3(256), 0, st, a);
  else if (dm.dh <= 256) hipLaunchKernelGGL((lg_attn_kernel<256, 0>), grid, dim3(256), 0, st, a);
  else return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// a layer's Linear: gemm() on the engine the mode asks for (the fp16 image is passed on only under LG_LIN_F16)
int linear(hipStream_t st, int epi, const Side& s, int B, const Dims& dm, const float* X, int ldx, const float* X2, int ldx2, int Ksplit, int K,
           const float* W, const uint16_t* W16, const float* bias, int N, float* Y, int ldy) {
  if (dm.lin16 && !W16) return -1;
  return gemm(st, epi, s, B, X, ldx, X2, ldx2, Ksplit, K, W, bias, N, Y, ldy, 1.0f, nullptr, nullptr, 0, 0, dm.lin16 ? W16 : nullptr);
}

// ffn(cat[x,msg]) + residual, in place on s.x
int ffn(hipStream_t st, const Side& s, int B, const Dims& dm, const float* msg, const float* w0, const uint16_t* w0h, const float* b0, const float* g,
        const float* be, const float* w3, const uint16_t* w3h, const float* b3) {
  const int d = dm.d;
  // (one fused launch for ffn.0 + LayerNorm + GELU was measured in round 3 and is slower: tools/experiments/lg_ffn0_ln_gelu_kernel.hip.txt)
  if (linear(st, EPI_BIAS, s, B, dm, s.x, d, msg, d, d, 2 * d, w0, w0h, b0, 2 * d, s.h, 2 * d)) return -1;
  {
    EINX_PROF("lg_ln_gelu_kernel", st);
    const dim3 lg((unsigned)einx_cdiv(s.cap, 4), (unsigned)B);
    if (2 * d == 512) hipLaunchKernelGGL(lg_ln_gelu_kernel, lg, dim3(256), 0, st, s.h, s.cnt, s.cap, g, be);
    else hipLaunchKernelGGL(lg_ln_gelu_any_kernel, lg, dim3(256), 0, st, s.h, s.cnt, s.cap, 2 * d, g, be);
  }
  if (hipGetLastError() != hipSuccess) return -1;
  return linear(st, EPI_RESID, s, B, dm, s.h, 2 * d, nullptr, 0, 0x7fffffff, 2 * d, w3, w3h, b3, d, s.x, d);
}

}  // namespace

EINX_EXPORT int einx_linear(const float* x, int M, int K, const float* w, const float* bias, int N, float* y, int accumulate, void* stream) {
  EINX_CHECK_ARG(x && w && bias && y, "null pointer");
  EINX_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 4 == 0, "bad shape (K must be a multiple of 4)");
  GemmArgs g;
  g.X = x;
  g.X2 = nullptr;
  g.W = w;
  g.bias = bias;
  g.Y = y;
  g.cnt = nullptr;
  g.cap = M;
  g.ldx = K;
  g.ldx2 = 0;
  g.Ksplit = 0x7fffffff;
  g.K = K;
  g.N = N;
  g.ldy = N;
  g.div = 1.0f;
  g.B = 1;
  const dim3 grid(gemm_grid<>(einx_cdiv(N, BN) * einx_cdiv(M, BM)));
  if (accumulate) hipLaunchKernelGGL(lg_gemm_kernel<EPI_RESID>, grid, dim3(THREADS), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL(lg_gemm_kernel<EPI_BIAS>, grid, dim3(THREADS), 0, (hipStream_t)stream, g);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_normalize_keypoints(const float* kpts, int rows, int cols, float h, float w, float* out, int out_cols,
                                         void* stream) {
  EINX_CHECK_ARG(kpts && out, "null pointer");
  EINX_CHECK_ARG(rows > 0 && cols >= 2 && out_cols >= 2, "bad shape");
  hipLaunchKernelGGL(lg_normalize_kpts_kernel, dim3((unsigned)einx_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, kpts, cols,
                     (size_t)rows, h, w, out, out_cols);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

namespace {
// lightglue.py:456-461: head_dim = descriptor_dim // num_heads.  The attention kernel is instantiated for 32-, 64- and 128-wide
// heads; other widths run the next larger one on zero-padded heads (round 6).  Multiples of 4 (16-byte rows of a head; the
// rotary encoding needs an even width anyway) up to 256 (<256, 0>: 256 + 100 registers, one workgroup per SIMD -- rare widths, not tuned).
bool dims_of(int d, int heads, Dims& dm) {
  if (d <= 0 || heads <= 0 || d % heads != 0) return false;
  dm.d = d;
  dm.heads = heads;
  dm.dh = d / heads;
  return dm.dh % 4 == 0 && dm.dh <= 256;
}
}  // namespace

namespace {
// the one launch check of this file; `entry`: the exported function the error is reported under
#define LG_CHECK(entry, expr)                                         \
  do {                                                                \
    if ((expr) != 0 || hipGetLastError() != hipSuccess) {             \
      einx_set_error("%s: kernel launch failed at %s", entry, #expr); \
      return EINX_ERR_LAUNCH;                                         \
    }                                                                 \
  } while (0)
constexpr const char* LG = "einx_lightglue";  // all three modes report under it

size_t lg_ws_bytes(LgMode mode, int B, int cap0, int cap1, int d, int heads, int n_layers) {
  Dims dm;
  if (B <= 0 || cap0 <= 0 || cap1 <= 0 || !dims_of(d, heads, dm)) return 0;
  if (mode != LG_PLAIN && (n_layers < 1 || n_layers > LG_MAX_HEADS)) return 0;
  LgWs w;
  WsCarver c{nullptr};
  carve(c, w, mode, {B, cap0, cap1, d, dm.dh, n_layers});
  return c.bytes;
}
}  // namespace

// (input_dim: part of the ABI; the descriptors are projected in place, so no region depends on it)
EINX_EXPORT size_t einx_lg_ws_bytes_heads(int B, int cap0, int cap1, int d, int heads, int) { return lg_ws_bytes(LG_PLAIN, B, cap0, cap1, d, heads, 0); }

EINX_EXPORT size_t einx_lg_ws_bytes(int B, int cap0, int cap1, int d, int input_dim) {  // 64-wide heads (the LightGlue default)
  return d > 0 && d % 64 == 0 ? einx_lg_ws_bytes_heads(B, cap0, cap1, d, d / 64, input_dim) : 0;
}

EINX_EXPORT size_t einx_lightglue_early_stop_ws_bytes(int B, int cap0, int cap1, int d, int heads, int, int n_layers) {
  return lg_ws_bytes(LG_EARLY_STOP, B, cap0, cap1, d, heads, n_layers);
}

EINX_EXPORT size_t einx_lightglue_adaptive_ws_bytes(int B, int cap0, int cap1, int d, int heads, int, int n_layers) {
  return lg_ws_bytes(LG_ADAPTIVE, B, cap0, cap1, d, heads, n_layers);
}

namespace {
// what einx_lightglue_early_stop hands to the shared body (null: einx_lightglue)
struct Adaptive {  // point pruning
  float thr_w;  // float32(1.0 - double(width_confidence))
  int min_kpts;
  float *prune0, *prune1;
  int64_t *kept0, *kept1;
  int32_t* live;
};
struct EarlyStop {
  const einx_lg_head* heads;
  float depth_confidence;  // with `ad`: <= 0 means no stop decision
  int32_t* stop;           // with `ad`: may be null (carved in the workspace; route (a) reads it either way)
  const Adaptive* ad;      // null: einx_lightglue_early_stop
};

// A set of keypoint counts: side 0 [B], side 1 [B], and the two as one [2B] array (what a launch over stacked sides reads)
struct Counts {
  const int32_t *c0, *c1, *both;
};

// the sides as a shared-weight stage iterates over them: one view of 2B entries (stacked), or two of B
struct Views {
  Side s[2];
  int n, entries;
};

struct LgCtx {
  hipStream_t st;
  const einx_lg_weights* w;
  Dims dm;
  LgShape sh;
  LgMode mode;
  const EarlyStop* es;  // null: LG_PLAIN
  const Adaptive* ad;   // null unless LG_ADAPTIVE
  bool decide;          // the stop decision runs (LG_ADAPTIVE: only with depth_confidence > 0)
  int32_t* stop;        // the caller's, or the workspace's; null: LG_PLAIN
  LgWs ws;
  Counts caller, layers, heads;  // see lg_run
  float size[2][2];              // the images' (h, w)
  int64_t* matches[2];
  float *scores[2], *la, *ref[2];
  bool all_layers;  // ref holds every layer's descriptors (training-mode output)
};

Views views(const LgCtx& c, const Counts& cnt, bool stacked) {
  Views v{{c.ws.s[0], c.ws.s[1]}, stacked ? 1 : 2, stacked ? 2 * c.sh.B : c.sh.B};
  v.s[0].cnt = stacked ? cnt.both : cnt.c0;
  v.s[1].cnt = cnt.c1;
  return v;
}

// confidence_threshold of a layer (lightglue.py:718-722): in double, rounded to float32 once
float confidence_threshold(int li, int n_layers) {
  const double thr = 0.8 + 0.1 * exp(-4.0 * li / n_layers);
  return (float)(thr < 0.0 ? 0.0 : thr > 1.0 ? 1.0 : thr);
}

// li < 0: the init launch, which reads no field of a layer
TailArgs tail_args(const LgCtx& c, int li) {
  TailArgs t{};
  t.x0 = c.ws.s[0].x, t.x1 = c.ws.s[1].x;
  t.act = c.ws.act;
  t.stop = c.stop;
  t.cap0 = c.sh.cap0, t.cap1 = c.sh.cap1, t.d = c.sh.d, t.B = c.sh.B;
  if (li < 0) return t;
  t.layer = li;
  if (c.decide) t.tw = c.es->heads[li].token_w, t.tb = c.es->heads[li].token_b;
  t.thr = confidence_threshold(li, c.w->n_layers);
  return t;
}

PruneArgs prune_args(const LgCtx& c, int li) {
  const Side* s = c.ws.s;
  PruneArgs a{};
  a.t = tail_args(c, li);
  a.enc0 = s[0].enc, a.enc1 = s[1].enc;
  a.tx0 = s[0].ctx, a.tx1 = s[1].ctx, a.te0 = s[0].h, a.te1 = s[1].h;
  a.live = c.ad->live, a.prev = c.ws.prev;
  a.dst0 = c.ws.dst0, a.dst1 = c.ws.dst1;
  a.kept0 = c.ad->kept0, a.kept1 = c.ad->kept1, a.prune0 = c.ad->prune0, a.prune1 = c.ad->prune1;
  a.n = c.caller.c0, a.m = c.caller.c1;
  a.dh2 = 2 * c.sh.dh;
  a.min_kpts = c.ad->min_kpts;
  a.set_stop = c.decide ? 1 : 0;
  a.thr_w = c.ad->thr_w;
  if (li >= 0) a.mw = c.es->heads[li].match_w, a.mb = c.es->heads[li].match_b;
  return a;
}

// the grid of a launch over 2B entries that gives every workgroup `rows` rows of the longer side
dim3 tail_grid(const LgShape& sh, int rows) { return dim3((unsigned)einx_cdiv(sh.cap0 > sh.cap1 ? sh.cap0 : sh.cap1, rows), (unsigned)(2 * sh.B)); }

template <typename... Src>  // the arguments of a match_head()
void launch_matchability(hipStream_t st, const Side& s, const float* x, int entries, int d, Src... src) {
  hipLaunchKernelGGL(lg_matchability_kernel<Src...>, dim3((unsigned)einx_cdiv(s.cap, 4), (unsigned)entries), dim3(256), 0, st, x, s.cnt, s.cap, d, src...,
                     s.cert, s.dust);
}

// ---- what has to be on the device before the first layer.  Early stopping: the heads' table, the [2B] counts, the private
// counts, stop and the counters in one launch; point pruning: its outputs' start values.  Otherwise the [2B] counts when the
// stacked layers will read them; plain and unstacked: no launch.
int lg_setup(const LgCtx& c) {
  const LgShape& sh = c.sh;
  if (c.es) {
    HeadTable t;
    for (int i = 0; i < sh.n_layers; ++i) {
      t.p[4 * i + 0] = c.es->heads[i].proj_w;
      t.p[4 * i + 1] = c.es->heads[i].proj_b;
      t.p[4 * i + 2] = c.es->heads[i].match_w;
      t.p[4 * i + 3] = c.es->heads[i].match_b;
    }
    const int items = 4 * sh.n_layers > 2 * sh.B ? 4 * sh.n_layers : 2 * sh.B;
    hipLaunchKernelGGL(lg_es_init_kernel, dim3((unsigned)einx_cdiv(items, 256)), dim3(256), 0, c.st, t, sh.n_layers, c.ws.heads, c.caller.c0, c.caller.c1,
                       sh.B, sh.cap0, sh.cap1, c.ws.cnt2, c.ws.act, c.stop, c.ws.below, c.ws.done);
    if (c.ad) hipLaunchKernelGGL(lg_prune_init_kernel, tail_grid(sh, 256), dim3(256), 0, c.st, prune_args(c, -1));
  } else if (sh.stacked()) {
    hipLaunchKernelGGL(lg_stack_counts_kernel, dim3((unsigned)einx_cdiv(2 * sh.B, 256)), dim3(256), 0, c.st, c.caller.c0, c.caller.c1, sh.B, c.ws.cnt2);
  }
  LG_CHECK(LG, 0);
  return EINX_OK;
}

// ---- input projection (or copy) + positional encodings (per side: own inputs, own image size)
int lg_input(const LgCtx& c) {
  const einx_lg_weights* w = c.w;
  const int B = c.sh.B, d = c.sh.d, dh = c.sh.dh;
  const Views v = views(c, c.caller, false);
  for (int sd = 0; sd < 2; ++sd) {
    const Side& s = v.s[sd];
    if (w->in_w) {
      LG_CHECK(LG, gemm(c.st, EPI_BIAS, s, B, s.desc, w->input_dim, nullptr, 0, 0x7fffffff, w->input_dim, w->in_w, w->in_b, d, s.x, d));
    } else {
      const size_t per = (size_t)s.cap * d;
      hipLaunchKernelGGL(lg_copy_rows_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)B), dim3(256), 0, c.st, s.desc, s.x, s.cnt, s.cap, d, per);
      LG_CHECK(LG, 0);
    }
    hipLaunchKernelGGL(lg_posenc_kernel, dim3((unsigned)einx_cdiv(s.cap * (dh / 2), 256), (unsigned)B), dim3(256), 0, c.st, s.kpts, s.cnt, s.cap,
                       c.size[sd][0], c.size[sd][1], w->Wr, s.enc, dh);
    LG_CHECK(LG, 0);
  }
  return EINX_OK;
}

// ---- one transformer layer: SelfBlock, then CrossBlock
int lg_layer(const LgCtx& c, int li) {
  const einx_lg_layer& L = c.w->layers[li];
  const Dims& dm = c.dm;
  hipStream_t st = c.st;
  const int B = c.sh.B, d = c.sh.d;
  const Views v = views(c, c.layers, c.sh.stacked());
  const int E = v.entries;
  for (int sd = 0; sd < v.n; ++sd) {
    const Side& s = v.s[sd];
    LG_CHECK(LG, gemm_qkv_rope(st, s, E, dm, s.x, L.Wqkv, L.Wqkv_h, L.bqkv, s.q, s.k, s.v));
    LG_CHECK(LG, attn(st, E, dm, s.q, s.cnt, s.cap, s.k, s.v, s.cnt, s.cap, s.ctx));
    if (L.Wo) {
      LG_CHECK(LG, linear(st, EPI_BIAS, s, E, dm, s.ctx, d, nullptr, 0, 0x7fffffff, d, L.Wo, L.Wo_h, L.bo, d, s.msg, d));
      LG_CHECK(LG, ffn(st, s, E, dm, s.msg, L.sf0_w, L.sf0_h, L.sf0_b, L.sln_g, L.sln_b, L.sf3_w, L.sf3_h, L.sf3_b));
    } else {  // out_proj folded into the FFN's first Linear at load time: message = context
      LG_CHECK(LG, ffn(st, s, E, dm, s.ctx, L.sf0_w, L.sf0_h, L.sf0_b, L.sln_g, L.sln_b, L.sf3_w, L.sf3_h, L.sf3_b));
    }
  }
  // to_qk and to_v read the same rows: with the merged weight image [Wqk; Wv] (shipped widths) they are ONE launch writing
  // qk | v side by side into the FFN's hidden buffer (free until ffn.0 runs), and the attention reads them at row stride 2 d --
  // the same k-ordered chain and bias per output, one launch less per layer
  const bool merged = L.Wqk_v && L.bqk_v && dm.shipped() && (!dm.lin16 || L.Wqk_v_h);
  for (int sd = 0; sd < v.n; ++sd) {
    const Side& s = v.s[sd];
    if (merged) {
      LG_CHECK(LG, linear(st, EPI_BIAS, s, E, dm, s.x, d, nullptr, 0, 0x7fffffff, d, L.Wqk_v, L.Wqk_v_h, L.bqk_v, 2 * d, s.h, 2 * d));
    } else {
      LG_CHECK(LG, linear(st, EPI_BIAS, s, E, dm, s.x, d, nullptr, 0, 0x7fffffff, d, L.Wqk, L.Wqk_h, L.bqk, d, s.q, d));
      LG_CHECK(LG, linear(st, EPI_BIAS, s, E, dm, s.x, d, nullptr, 0, 0x7fffffff, d, L.Wv, L.Wv_h, L.bv, d, s.v, d));
    }
  }
  const Side &r0 = v.s[0], &r1 = v.s[1];
  if (v.n == 1) {  // stacked: entry b attends to the keys / values of its partner entry (b + B) mod 2B
    if (merged) LG_CHECK(LG, attn(st, E, dm, r0.h, r0.cnt, r0.cap, r0.h, r0.h + d, r0.cnt, r0.cap, r0.ctx, B, true));
    else LG_CHECK(LG, attn(st, E, dm, r0.q, r0.cnt, r0.cap, r0.q, r0.v, r0.cnt, r0.cap, r0.ctx, B));
  } else if (merged) {
    LG_CHECK(LG, attn(st, B, dm, r0.h, r0.cnt, r0.cap, r1.h, r1.h + d, r1.cnt, r1.cap, r0.ctx, 0, true));
    LG_CHECK(LG, attn(st, B, dm, r1.h, r1.cnt, r1.cap, r0.h, r0.h + d, r0.cnt, r0.cap, r1.ctx, 0, true));
  } else {
    LG_CHECK(LG, attn(st, B, dm, r0.q, r0.cnt, r0.cap, r1.q, r1.v, r1.cnt, r1.cap, r0.ctx));
    LG_CHECK(LG, attn(st, B, dm, r1.q, r1.cnt, r1.cap, r0.q, r0.v, r0.cnt, r0.cap, r1.ctx));
  }
  for (int sd = 0; sd < v.n; ++sd) {
    const Side& s = v.s[sd];
    if (L.Wco) {
      LG_CHECK(LG, linear(st, EPI_BIAS, s, E, dm, s.ctx, d, nullptr, 0, 0x7fffffff, d, L.Wco, L.Wco_h, L.bco, d, s.msg, d));
      LG_CHECK(LG, ffn(st, s, E, dm, s.msg, L.cf0_w, L.cf0_h, L.cf0_b, L.cln_g, L.cln_b, L.cf3_w, L.cf3_h, L.cf3_b));
    } else {
      LG_CHECK(LG, ffn(st, s, E, dm, s.ctx, L.cf0_w, L.cf0_h, L.cf0_b, L.cln_g, L.cln_b, L.cf3_w, L.cf3_h, L.cf3_b));
    }
  }
  return EINX_OK;
}

// ---- ref_descriptors: x of both sides, rows below `cnt`, into slot `slot` of `slots` per pair (lightglue.py:626-629)
int lg_ref_copy(const LgCtx& c, const Counts& cnt, int slot, int slots) {
  const Views v = views(c, cnt, false);
  for (int sd = 0; sd < 2; ++sd) {
    const Side& s = v.s[sd];
    if (!c.ref[sd]) continue;
    const size_t per = (size_t)s.cap * c.sh.d;
    hipLaunchKernelGGL(lg_copy_rows_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)c.sh.B), dim3(256), 0, c.st, s.x, c.ref[sd] + (size_t)slot * per,
                       s.cnt, s.cap, c.sh.d, per * (size_t)slots);
    LG_CHECK(LG, 0);
  }
  return EINX_OK;
}

// ---- the pairs still running decide whether layer li was their last
int lg_stop(const LgCtx& c, int li) {
  StopArgs a{};
  a.t = tail_args(c, li);
  a.depth = c.es->depth_confidence;
  a.below = c.ws.below;
  a.done = c.ws.done;
  if (c.ad) a.tot0 = c.caller.c0, a.tot1 = c.caller.c1;
  EINX_PROF("lg_stop_kernel", c.st);
  hipLaunchKernelGGL(lg_stop_kernel, tail_grid(c.sh, STOP_ROWS), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  return EINX_OK;
}

// ---- point pruning behind layer li, after the stop decision (lightglue.py:632-652): a pair that has just stopped is not pruned
int lg_prune(const LgCtx& c, int li) {
  const LgShape& sh = c.sh;
  const PruneArgs a = prune_args(c, li);
  EINX_PROF("lg_prune (keep + scan + gather + copy back)", c.st);
  hipLaunchKernelGGL(lg_keep_kernel, tail_grid(sh, STOP_ROWS), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  hipLaunchKernelGGL(lg_prune_scan_kernel, dim3((unsigned)sh.B), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  hipLaunchKernelGGL(lg_prune_gather_kernel, tail_grid(sh, 4), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  const size_t quads = (size_t)(sh.cap0 > sh.cap1 ? sh.cap0 : sh.cap1) * ((sh.d + 2 * sh.dh) / 4);
  hipLaunchKernelGGL(lg_prune_copyback_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)(2 * sh.B)), dim3(256), 0, c.st, a);
  LG_CHECK(LG, 0);
  return EINX_OK;
}

// ---- MatchAssignment's inputs (lightglue.py:365-377): final_proj / d^(1/4) and the matchability terms.  Early stopping, route
// (a): one stage over every pair's own rows, each pair with the head it stopped at (x frozen since then)
int lg_assign_heads(const LgCtx& c) {
  const einx_lg_weights* w = c.w;
  const int d = c.sh.d;
  const float div = sqrtf(sqrtf((float)d));
  const Views v = views(c, c.heads, c.sh.stacked());
  for (int sd = 0; sd < v.n; ++sd) {
    const Side& s = v.s[sd];
    if (c.es) {
      LG_CHECK(LG, gemm(c.st, EPI_DIV_HEAD, s, v.entries, s.x, d, nullptr, 0, 0x7fffffff, d, nullptr, nullptr, d, s.q, d, div, c.ws.heads, c.stop,
                        c.sh.B, c.sh.n_layers));
      launch_matchability(c.st, s, s.x, v.entries, d, c.ws.heads, c.stop, c.sh.B, c.sh.n_layers);
    } else {
      LG_CHECK(LG, gemm(c.st, EPI_DIV, s, v.entries, s.x, d, nullptr, 0, 0x7fffffff, d, w->proj_w, w->proj_b, d, s.q, d, div));
      launch_matchability(c.st, s, s.x, v.entries, d, w->match_w, w->match_b);
    }
    LG_CHECK(LG, 0);
  }
  return EINX_OK;
}

dim3 assign_grid(const MnnArgs& a, int B) { return dim3((unsigned)einx_cdiv(a.cap1, BN), (unsigned)einx_cdiv(a.cap0, BM), (unsigned)B); }

// The first half of every assignment: the MNN argument block from the two sides (q, cert, dust) and a pair of counts, then the
// softmax statistics (first tile pass) and their reduction.  The caller opens the profile scope and runs its own second pass.
int assign_prologue(const char* entry, hipStream_t st, MnnArgs& a, const Side& s0, const Side& s1, const int32_t* n, const int32_t* m, int B, int d,
                    float* la) {
  a.d0 = s0.q;
  a.d1 = s1.q;
  a.n = n;
  a.m = m;
  a.cap0 = s0.cap;
  a.cap1 = s1.cap;
  a.D = d;
  a.la = la;
  a.cert0 = s0.cert;
  a.cert1 = s1.cert;
  a.dust0 = s0.dust;
  a.dust1 = s1.dust;
  const int mx = a.cap0 > a.cap1 ? a.cap0 : a.cap1;
  hipLaunchKernelGGL((mnn_tile_kernel<1, false>), assign_grid(a, B), dim3(THREADS), 0, st, a);
  LG_CHECK(entry, 0);
  hipLaunchKernelGGL(mnn_lse_kernel, dim3((unsigned)einx_cdiv(mx + 1, 256), (unsigned)B), dim3(256), 0, st, a);
  LG_CHECK(entry, 0);
  return EINX_OK;
}

// ---- assignment scores, their arg-max keys, filter_matches
int lg_assign(const LgCtx& c) {
  const LgShape& sh = c.sh;
  hipStream_t st = c.st;
  MnnArgs a = c.ws.mnn;
  if (hipMemsetAsync(a.rowkey, 0, (char*)a.rowstat - (char*)a.rowkey, st) != hipSuccess) {  // rowkey | colkey
    einx_set_error("einx_lightglue: memset failed");
    return EINX_ERR_LAUNCH;
  }
  EINX_PROF("lg_assignment (3 tile passes + lse + finalize)", st);
  if (const int rc = assign_prologue(LG, st, a, c.ws.s[0], c.ws.s[1], c.heads.c0, c.heads.c1, sh.B, sh.d, c.la)) return rc;
  if (c.la) hipLaunchKernelGGL((mnn_tile_kernel<6, true>), assign_grid(a, sh.B), dim3(THREADS), 0, st, a);  // arg-max + log_assignment write in one visit
  else hipLaunchKernelGGL((mnn_tile_kernel<0, true>), assign_grid(a, sh.B), dim3(THREADS), 0, st, a);
  LG_CHECK(LG, 0);
  if (c.ad) {  // the keys are those of the live rows: back to original indexing
    hipLaunchKernelGGL(lg_finalize_scatter_kernel, dim3((unsigned)sh.B), dim3(256), 0, st, a.rowkey, a.colkey, c.heads.both, sh.B, c.ad->kept0,
                       c.ad->kept1, sh.cap0, sh.cap1, c.w->filter_threshold, c.matches[0], c.matches[1], c.scores[0], c.scores[1]);
  } else {
    const int mx = sh.cap0 > sh.cap1 ? sh.cap0 : sh.cap1;
    hipLaunchKernelGGL(lg_finalize_kernel, dim3((unsigned)einx_cdiv(mx, 256), (unsigned)sh.B), dim3(256), 0, st, a.rowkey, a.colkey, c.heads.c0, c.heads.c1,
                       sh.cap0, sh.cap1, c.w->filter_threshold, c.matches[0], c.matches[1], c.scores[0], c.scores[1]);
  }
  LG_CHECK(LG, 0);
  return EINX_OK;
}

int lg_run(const einx_lg_weights* w, const EarlyStop* es, unsigned mode, const float* kpts0, const float* desc0, const int32_t* n, int cap0, const float* kpts1,
           const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1, float w1, void* ws, int64_t* matches0,
           int64_t* matches1, float* scores0, float* scores1, float* la, float* ref0, float* ref1, int ref_layers, void* stream) {
  EINX_CHECK_ARG(w && kpts0 && desc0 && n && kpts1 && desc1 && m && ws && matches0 && matches1 && scores0 && scores1, "null pointer");
  Dims dm;
  EINX_CHECK_ARG(dims_of(w->d, w->heads, dm), "descriptor_dim must be num_heads x head_dim with head_dim a multiple of 4, at most 256");
  EINX_CHECK_ARG(w->struct_size == sizeof(einx_lg_weights) && w->layer_size == sizeof(einx_lg_layer),
                 "einx_lg_weights::struct_size / layer_size do not match this library (header / library ABI mismatch)");
  EINX_CHECK_ARG(w->n_layers >= 1 && w->layers, "no layers");
  EINX_CHECK_ARG(B > 0 && cap0 > 0 && cap1 > 0, "bad shape");
  EINX_CHECK_ARG(w->input_dim % 4 == 0 && w->input_dim > 0, "input_dim must be a multiple of 4");
  EINX_CHECK_ARG((w->input_dim == dm.d) == (w->in_w == nullptr), "input_proj must be given exactly when input_dim != d");
  EINX_CHECK_ARG(ref_layers == 0 || ref_layers == 1 || ref_layers == w->n_layers, "ref_layers must be 0/1 (last layer) or n_layers");
  LgCtx c{};
  c.st = (hipStream_t)stream;
  c.w = w;
  c.dm = dm;
  c.dm.flash = (mode & LG_ATTN_F16) != 0;
  c.dm.lin16 = (mode & LG_LIN_F16) != 0;
  c.sh = {B, cap0, cap1, dm.d, dm.dh, w->n_layers};
  c.es = es;
  if (es) c.ad = es->ad;
  c.mode = LG_PLAIN;
  if (es) c.mode = c.ad ? LG_ADAPTIVE : LG_EARLY_STOP;
  WsCarver wc{(char*)ws};
  carve(wc, c.ws, c.mode, c.sh);
  c.ws.s[0].kpts = kpts0, c.ws.s[0].desc = desc0, c.ws.s[0].cap = cap0;
  c.ws.s[1].kpts = kpts1, c.ws.s[1].desc = desc1, c.ws.s[1].cap = cap1;
  // caller: the input stage and the all-layers ref copy; with pruning also the stop ratio's denominator
  // layers: the transformer layers; the stop decision zeroes a pair's, the pruning step shrinks them with the rows kept
  // heads:  the assignment heads, the last-layer ref copy, the assignment and filter_matches: what survived, also of a stopped pair
  c.caller = {n, m, c.ws.cnt2};
  c.layers = c.heads = c.caller;
  if (es) c.layers = {c.ws.act, c.ws.act + B, c.ws.act};
  if (c.ad) c.heads = {c.ad->live, c.ad->live + B, c.ad->live};
  if (es) c.stop = es->stop ? es->stop : c.ws.stop;
  c.decide = es && (!c.ad || es->depth_confidence > 0.0f);
  c.size[0][0] = h0, c.size[0][1] = w0, c.size[1][0] = h1, c.size[1][1] = w1;
  c.matches[0] = matches0, c.matches[1] = matches1, c.scores[0] = scores0, c.scores[1] = scores1;
  c.la = la, c.ref[0] = ref0, c.ref[1] = ref1;
  c.all_layers = ref_layers > 1;

  int rc = lg_setup(c);
  if (!rc) rc = lg_input(c);
  for (int li = 0; li < w->n_layers && !rc; ++li) {
    const bool last = li == w->n_layers - 1;
    rc = lg_layer(c, li);
    if (!rc && c.all_layers) rc = lg_ref_copy(c, c.caller, li, w->n_layers);
    if (!rc && c.decide && !last) rc = lg_stop(c, li);
    if (!rc && c.ad && !last) rc = lg_prune(c, li);
  }
  if (!rc) rc = lg_assign_heads(c);
  if (!rc && !c.all_layers) rc = lg_ref_copy(c, c.heads, 0, 1);
  if (!rc) rc = lg_assign(c);
  return rc;
}

// What is wrong with the heads of an early-stop or adaptive call, or null; in the order the entries have always checked: the
// struct's size, the layer count, the entry's complaint about its own scalars (`own`, or null), every layer's heads.  token_msg:
// the complaint about a missing token_confidence head, or null when none is needed.
const char* heads_error(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, const char* layers_msg, const char* own,
                        const char* token_msg) {
  if (head_size != sizeof(einx_lg_head)) return "head_size does not match this library's einx_lg_head (header / library ABI mismatch)";
  if (w->n_layers < 1 || w->n_layers > LG_MAX_HEADS) return layers_msg;
  if (own) return own;
  for (int i = 0; i < w->n_layers; ++i) {
    const einx_lg_head& h = heads[i];
    if (!(h.proj_w && h.proj_b && h.match_w && h.match_b)) return "every layer needs its log_assignment head";
    if (token_msg && i < w->n_layers - 1 && !(h.token_w && h.token_b)) return token_msg;
  }
  return nullptr;
}
}  // namespace

EINX_EXPORT int einx_lightglue(const einx_lg_weights* w, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                               const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1,
                               float w1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la,
                               float* ref0, float* ref1, int ref_layers, void* stream) {
  return lg_run(w, nullptr, 0, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0, w0, h1, w1, ws, matches0, matches1, scores0, scores1, la, ref0,
                ref1, ref_layers, stream);
}

namespace {
// the bodies of the early-stop and adaptive entries; entry: the exported function an argument error is reported under; mode: the
// precision bits (LG_ATTN_F16: the attention of einx_lightglue_flash, LG_LIN_F16: the linears of einx_lightglue_mp)
#define LG_CHECK_ARG(cond, msg)                \
  do {                                         \
    if (!(cond)) {                             \
      einx_set_error("%s: %s", entry, msg);    \
      return EINX_ERR_ARG;                     \
    }                                          \
  } while (0)
int lg_early_stop(const char* entry, unsigned mode, const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                          const float* kpts0, const float* desc0, const int32_t* n, int cap0, const float* kpts1,
                                          const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1, float w1, void* ws,
                                          int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, float* ref0,
                                          float* ref1, int32_t* stop, void* stream) {
  LG_CHECK_ARG(w && heads && stop, "null pointer");
  const char* bad =
      heads_error(w, heads, head_size, "early stopping takes 1..32 layers", nullptr, "every layer but the last needs its token_confidence head");
  LG_CHECK_ARG(!bad, bad);
  const EarlyStop es{heads, depth_confidence, stop, nullptr};
  return lg_run(w, &es, mode, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0, w0, h1, w1, ws, matches0, matches1, scores0, scores1, la, ref0, ref1,
                1, stream);
}

int lg_adaptive(const char* entry, unsigned mode, const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                        double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                                        const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1,
                                        float w1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la,
                                        float* ref0, float* ref1, int32_t* stop, float* prune0, float* prune1, int64_t* kept0, int64_t* kept1,
                                        int32_t* live, void* stream) {
  LG_CHECK_ARG(w && heads && prune0 && prune1 && kept0 && kept1 && live, "null pointer");
  const char* own = nullptr;
  if (la) own = "log_assignment is not produced with point pruning (DESIGN.md 8j): la must be null";
  if (!(width_confidence > 0.0 && width_confidence <= 1.0)) own = "width_confidence must be in (0, 1]";
  const char* token_msg = depth_confidence <= 0.0f ? nullptr : "with depth_confidence > 0 every layer but the last needs its token_confidence head";
  const char* bad = heads_error(w, heads, head_size, "point pruning takes 1..32 layers", own, token_msg);
  LG_CHECK_ARG(!bad, bad);
  const Adaptive ad{(float)(1.0 - width_confidence), min_kpts, prune0, prune1, kept0, kept1, live};
  const EarlyStop es{heads, depth_confidence, stop, &ad};
  return lg_run(w, &es, mode, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0, w0, h1, w1, ws, matches0, matches1, scores0, scores1, nullptr, ref0,
                ref1, 1, stream);
}
}  // namespace

EINX_EXPORT int einx_lightglue_early_stop(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                          const float* kpts0, const float* desc0, const int32_t* n, int cap0, const float* kpts1,
                                          const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1, float w1, void* ws,
                                          int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, float* ref0,
                                          float* ref1, int32_t* stop, void* stream) {
  return lg_early_stop(__func__, 0, w, heads, head_size, depth_confidence, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0, w0, h1, w1, ws, matches0,
                       matches1, scores0, scores1, la, ref0, ref1, stop, stream);
}

EINX_EXPORT int einx_lightglue_adaptive(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                        double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                                        const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1,
                                        float w1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la,
                                        float* ref0, float* ref1, int32_t* stop, float* prune0, float* prune1, int64_t* kept0, int64_t* kept1,
                                        int32_t* live, void* stream) {
  return lg_adaptive(__func__, 0, w, heads, head_size, depth_confidence, width_confidence, min_kpts, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0,
                     w0, h1, w1, ws, matches0, matches1, scores0, scores1, la, ref0, ref1, stop, prune0, prune1, kept0, kept1, live, stream);
}

// conf.flash: the three runs above with every attention in fp16 on the matrix cores.  width_confidence > 0: the
// adaptive run; else depth_confidence > 0: the early-stop run; else the plain run (heads, stop and the pruning outputs unread).
EINX_EXPORT size_t einx_lightglue_flash_ws_bytes(int B, int cap0, int cap1, int d, int heads, int, int n_layers) {
  // the kernel needs no region of its own: the largest carve of the three runs; a layer count only the plain run takes: its carve
  const size_t adaptive = lg_ws_bytes(LG_ADAPTIVE, B, cap0, cap1, d, heads, n_layers);
  return adaptive ? adaptive : lg_ws_bytes(LG_PLAIN, B, cap0, cap1, d, heads, 0);
}

EINX_EXPORT int einx_lightglue_flash(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                     double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                                     const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1,
                                     float w1, void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la,
                                     float* ref0, float* ref1, int ref_layers, int32_t* stop, float* prune0, float* prune1, int64_t* kept0,
                                     int64_t* kept1, int32_t* live, void* stream) {
  if (width_confidence > 0.0) {
    EINX_CHECK_ARG(ref_layers == 0 || ref_layers == 1, "point pruning returns the surviving rows, not every layer's: ref_layers must be 0 or 1");
    return lg_adaptive(__func__, LG_ATTN_F16, w, heads, head_size, depth_confidence, width_confidence, min_kpts, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0,
                       w0, h1, w1, ws, matches0, matches1, scores0, scores1, la, ref0, ref1, stop, prune0, prune1, kept0, kept1, live, stream);
  }
  if (depth_confidence > 0.0f) {
    EINX_CHECK_ARG(ref_layers == 0 || ref_layers == 1, "early stopping returns the rows the stopping head read: ref_layers must be 0 or 1");
    return lg_early_stop(__func__, LG_ATTN_F16, w, heads, head_size, depth_confidence, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0, w0, h1, w1, ws, matches0,
                         matches1, scores0, scores1, la, ref0, ref1, stop, stream);
  }
  return lg_run(w, nullptr, LG_ATTN_F16, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0, w0, h1, w1, ws, matches0, matches1, scores0, scores1, la, ref0,
                ref1, ref_layers, stream);
}

// conf.mp: the same three runs with the precision modes as bits.  EINX_LG_LIN_F16: the nine linears of every layer on
// the f16 tile engine (inputs and weights rounded to binary16, fp32 accumulation, fp32 bias, fp32 result); EINX_LG_ATTN_F16: the
// attention of einx_lightglue_flash.  mode == 0 is einx_lightglue / _early_stop / _adaptive, mode == EINX_LG_ATTN_F16 is _flash.
EINX_EXPORT size_t einx_lightglue_mp_ws_bytes(int B, int cap0, int cap1, int d, int heads, int input_dim, int n_layers) {
  return einx_lightglue_flash_ws_bytes(B, cap0, cap1, d, heads, input_dim, n_layers);  // neither kernel needs a region of its own
}

EINX_EXPORT int einx_lightglue_mp(const einx_lg_weights* w, const einx_lg_head* heads, size_t head_size, float depth_confidence,
                                  double width_confidence, int min_kpts, const float* kpts0, const float* desc0, const int32_t* n, int cap0,
                                  const float* kpts1, const float* desc1, const int32_t* m, int cap1, int B, float h0, float w0, float h1, float w1,
                                  void* ws, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1, float* la, float* ref0,
                                  float* ref1, int ref_layers, int32_t* stop, float* prune0, float* prune1, int64_t* kept0, int64_t* kept1,
                                  int32_t* live, int mode, void* stream) {
  EINX_CHECK_ARG(w, "null pointer");
  EINX_CHECK_ARG((mode & ~(LG_ATTN_F16 | LG_LIN_F16)) == 0, "mode takes EINX_LG_ATTN_F16 | EINX_LG_LIN_F16 only");
  if (mode & LG_LIN_F16) {  // the contract rounds the weights as written: no folded out_proj / to_out, and every linear's fp16 image
    EINX_CHECK_ARG(w->struct_size == sizeof(einx_lg_weights) && w->layer_size == sizeof(einx_lg_layer),
                   "einx_lg_weights::struct_size / layer_size do not match this library (header / library ABI mismatch)");
    EINX_CHECK_ARG(w->n_layers >= 1 && w->layers, "no layers");
    for (int li = 0; li < w->n_layers; ++li) {
      const einx_lg_layer& L = w->layers[li];
      EINX_CHECK_ARG(L.Wo && L.bo && L.Wco && L.bco, "linears in fp16 take unfolded weights: every layer needs Wo / bo / Wco / bco");
      EINX_CHECK_ARG(L.Wqkv_h && L.Wo_h && L.sf0_h && L.sf3_h && L.Wqk_h && L.Wv_h && L.Wco_h && L.cf0_h && L.cf3_h,
                     "linears in fp16 need the binary16 image of every layer's nine weights");
    }
  }
  if (width_confidence > 0.0) {
    EINX_CHECK_ARG(ref_layers == 0 || ref_layers == 1, "point pruning returns the surviving rows, not every layer's: ref_layers must be 0 or 1");
    return lg_adaptive(__func__, (unsigned)mode, w, heads, head_size, depth_confidence, width_confidence, min_kpts, kpts0, desc0, n, cap0, kpts1, desc1, m,
                       cap1, B, h0, w0, h1, w1, ws, matches0, matches1, scores0, scores1, la, ref0, ref1, stop, prune0, prune1, kept0, kept1, live, stream);
  }
  if (depth_confidence > 0.0f) {
    EINX_CHECK_ARG(ref_layers == 0 || ref_layers == 1, "early stopping returns the rows the stopping head read: ref_layers must be 0 or 1");
    return lg_early_stop(__func__, (unsigned)mode, w, heads, head_size, depth_confidence, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0, w0, h1, w1, ws,
                         matches0, matches1, scores0, scores1, la, ref0, ref1, stop, stream);
  }
  return lg_run(w, nullptr, (unsigned)mode, kpts0, desc0, n, cap0, kpts1, desc1, m, cap1, B, h0, w0, h1, w1, ws, matches0, matches1, scores0, scores1, la,
                ref0, ref1, ref_layers, stream);
}

// The linear of conf.mp alone (a test hook): Y[b, i, :] (+)= RN16(cat(X[b, i, :Ksplit], X2[b, i, :K - Ksplit])) @ W16^T + bias for the
// first min(cnt[b], cap) rows of entry b (cnt null: cap rows); rows past the count are not written.
EINX_EXPORT int einx_lg_linear_f16(const float* X, const float* X2, int Ksplit, int K, const uint16_t* W16, const float* bias, int N, float* Y, int ldy,
                                   const float* resid, const int32_t* cnt, int cap, int B, int epi, void* stream) {
  EINX_CHECK_ARG(X && W16 && bias && Y, "null pointer");
  EINX_CHECK_ARG(B > 0 && cap > 0 && N > 0 && K > 0 && K % 4 == 0, "bad shape (K must be a multiple of 4)");
  EINX_CHECK_ARG(ldy >= N, "ldy must be at least N");
  EINX_CHECK_ARG(!X2 || (Ksplit > 0 && Ksplit < K && Ksplit % einx_gemm16::BK == 0), "Ksplit must be a multiple of the 32-deep K slab inside (0, K)");
  EINX_CHECK_ARG(epi == 0 || epi == 1, "epi must be 0 (bias) or 1 (bias + residual)");
  EINX_CHECK_ARG(epi == 1 || resid == nullptr, "resid is read by epi 1 only: with epi 0 it must be null");
  EINX_CHECK_ARG(epi == 0 || resid == nullptr || resid == Y, "the residual is accumulated in place: resid must be Y (or null)");
  Side s{};
  s.cnt = cnt;
  s.cap = cap;
  const int k1 = X2 ? Ksplit : K;
  if (gemm((hipStream_t)stream, epi ? EPI_RESID : EPI_BIAS, s, B, X, k1, X2, K - k1, X2 ? Ksplit : 0x7fffffff, K, nullptr, bias, N, Y, ldy, 1.0f, nullptr,
           nullptr, 0, 0, W16) != 0) {
    einx_set_error("einx_lg_linear_f16: kernel launch failed");
    return EINX_ERR_LAUNCH;
  }
  return EINX_OK;
}

// The attention of conf.flash alone (a test hook): O[b, q, h dh ..] = RN16(softmax_j(RN16(Q_h[q]) . RN16(K_h[j]) / sqrt(dh)) RN16(V_h[j]))
// for the first nq[b] rows of entry b over the first nk[bk] keys of entry bk = (b + kv_shift) mod B.  Q / K / V: fp32 [B, cap, ld]
// (the heads' columns start at 0; ld >= heads * dh, a multiple of 4), O: fp32 [B, capq, heads * dh]; rows past nq are not written.
EINX_EXPORT int einx_lg_attention_f16(const float* Q, const float* K, const float* V, float* O, const int32_t* nq, const int32_t* nk, int capq,
                                      int capk, int B, int heads, int dh, int ld, int kv_shift, void* stream) {
  EINX_CHECK_ARG(Q && K && V && O && nq && nk, "null pointer");
  EINX_CHECK_ARG(B > 0 && capq > 0 && capk > 0, "bad shape");
  Dims dm;
  EINX_CHECK_ARG(heads > 0 && dh > 0 && dims_of(heads * dh, heads, dm), "head_dim must be a multiple of 4, at most 256");
  EINX_CHECK_ARG(ld >= dm.d && ld % 4 == 0, "ld must be a multiple of 4, at least heads x head_dim");
  EINX_CHECK_ARG(kv_shift >= 0 && kv_shift < B, "kv_shift must be in [0, B)");
  AttnArgs a;
  a.Q = Q, a.K = K, a.V = V, a.O = O, a.nq = nq, a.nk = nk;
  a.capq = capq, a.capk = capk;
  a.scale = 1.0f / sqrtf((float)dm.dh);
  a.kv_shift = kv_shift, a.Btot = B, a.d = dm.d, a.dh = dm.dh;
  const dim3 grid((unsigned)einx_cdiv(capq, 128), (unsigned)dm.heads, (unsigned)B);
  if (attn_f16((hipStream_t)stream, grid, dm, a, ld) != 0) {
    einx_set_error("einx_lg_attention_f16: kernel launch failed");
    return EINX_ERR_LAUNCH;
  }
  return EINX_OK;
}

// ------------------------------------------------------------------------------------------
// Assignment NLL of one MatchAssignment head (lightglue.py:66-133, :751-769): the sums behind NLLLoss and
// row_norm without a log_assignment matrix.
// ------------------------------------------------------------------------------------------
namespace {

struct NllWs {
  Side s0, s1;  // q (projected descriptors), cert, dust
};

// einx_lg_assign_nll's workspace (einx_lg_assign_nll_ws_bytes walks it from a null base): per side the projected descriptors
// [B,cap,d] and cert / dust [B,cap]; the matcher's workspace (match_tiles.h); the per-chunk partial sums [B,cap0,nc64,3]; slack.
void carve_nll(WsCarver& c, NllWs& w, MnnArgs& a, int B, int cap0, int cap1, int d) {
  w.s0.q = c.take<float>((size_t)B * cap0 * d);
  w.s1.q = c.take<float>((size_t)B * cap1 * d);
  w.s0.cert = c.take<float>((size_t)B * cap0);
  w.s0.dust = c.take<float>((size_t)B * cap0);
  w.s1.cert = c.take<float>((size_t)B * cap1);
  w.s1.dust = c.take<float>((size_t)B * cap1);
  einx_match::carve(c, a, B, cap0, cap1);
  a.nllstat = c.take<float>((size_t)B * cap0 * a.nc64 * 3);
  c.slack(256);
}

constexpr int NLL_OUT = 8;  // S_pos, num_pos, S_neg0, num_neg0, S_neg1, num_neg1, sum of the row sums of exp, n

// One workgroup per pair.  A thread adds its rows (i = tid, tid + 256, ...) in ascending order, each row's chunk partials in
// ascending chunk order, then its columns; the threads' sums meet as in loss.hip: lane l of wave 0 adds the LDS entries l,
// l + 64, ... in order, then the xor butterfly.  float64 throughout, one fixed order: two calls give the same bits.
__global__ __launch_bounds__(256) void lg_nll_finish_kernel(const MnnArgs a, const int64_t* gt0, const int64_t* gt1, double* out) {
  __shared__ double red[7 * 256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = max(0, min(a.n[b], a.cap0)), m = max(0, min(a.m[b], a.cap1));
  double* o = out + (size_t)b * NLL_OUT;
  if (n == 0 || m == 0) {  // no assignment to speak of: zeros (uniform over the workgroup)
    if (tid < NLL_OUT) o[tid] = 0.0;
    return;
  }
  const int chunks = (m + 63) / 64;
  double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += 256) {
    const float* st = a.nllstat + ((size_t)b * a.cap0 + i) * a.nc64 * 3;
    double e = 0.0, sw = 0.0, cw = 0.0;
    for (int c = 0; c < chunks; ++c) {
      e += (double)st[3 * c];
      sw += (double)st[3 * c + 1];
      cw += (double)st[3 * c + 2];
    }
    const float d0 = a.dust0[(size_t)b * a.cap0 + i];
    v[0] += sw;
    v[1] += cw;
    v[6] += e + exp((double)d0);  // the dustbin column belongs to row_norm (:769)
    if (gt0[(size_t)b * a.cap0 + i] == -1) {
      v[2] += (double)d0;
      v[3] += 1.0;
    }
  }
  for (int j = tid; j < m; j += 256)
    if (gt1[(size_t)b * a.cap1 + j] == -1) {
      v[4] += (double)a.dust1[(size_t)b * a.cap1 + j];
      v[5] += 1.0;
    }
#pragma unroll
  for (int k = 0; k < 7; ++k) red[k * 256 + tid] = v[k];
  __syncthreads();
  if (tid < 64) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      double s = 0.0;
      for (int i = tid; i < 256; i += 64) s += red[k * 256 + i];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
      if (tid == 0) o[k] = s;
    }
    if (tid == 0) o[7] = (double)n;
  }
}

}  // namespace

EINX_EXPORT size_t einx_lg_assign_nll_ws_bytes(int B, int cap0, int cap1, int d) {
  if (B <= 0 || cap0 <= 0 || cap1 <= 0 || d <= 0 || d % 4 != 0) return 0;
  NllWs w;
  MnnArgs a;
  WsCarver c{nullptr};
  carve_nll(c, w, a, B, cap0, cap1, d);
  return c.bytes;
}

EINX_EXPORT int einx_lg_assign_nll(const float* proj_w, const float* proj_b, const float* match_w, const float* match_b, int d, const float* x0,
                                   const int32_t* n, int cap0, const float* x1, const int32_t* m, int cap1, int B, const int64_t* gt_matches0,
                                   const int64_t* gt_matches1, const int32_t* pos0, const unsigned char* assignment, int64_t as_b, int64_t as_i,
                                   int64_t as_j, void* ws, double* out, void* stream) {
  EINX_CHECK_ARG(proj_w && proj_b && match_w && match_b && x0 && n && x1 && m && gt_matches0 && gt_matches1 && ws && out, "null pointer");
  EINX_CHECK_ARG((pos0 != nullptr) != (assignment != nullptr), "give the positives as pos0 or as a dense assignment, not both");
  EINX_CHECK_ARG(B > 0 && cap0 > 0 && cap1 > 0 && d > 0 && d % 4 == 0, "bad shape (d must be a multiple of 4)");
  hipStream_t st = (hipStream_t)stream;
  const char* const entry = __func__;
  NllWs w{};
  MnnArgs a{};
  WsCarver c{(char*)ws};
  carve_nll(c, w, a, B, cap0, cap1, d);
  w.s0.cnt = n;
  w.s0.cap = cap0;
  w.s1.cnt = m;
  w.s1.cap = cap1;
  const float* x[2] = {x0, x1};
  const Side* sides[2] = {&w.s0, &w.s1};
  LG_CHECK(entry, 0);
  for (int sd = 0; sd < 2; ++sd) {  // MatchAssignment (lightglue.py:365-377): final_proj / d^(1/4) and the matchability terms
    const Side& s = *sides[sd];
    LG_CHECK(entry, gemm(st, EPI_DIV, s, B, x[sd], d, nullptr, 0, 0x7fffffff, d, proj_w, proj_b, d, s.q, d, sqrtf(sqrtf((float)d))));
    launch_matchability(st, s, x[sd], B, d, match_w, match_b);
    LG_CHECK(entry, 0);
  }
  a.pos0 = pos0;
  a.assign = assignment;
  a.as_b = as_b;
  a.as_i = as_i;
  a.as_j = as_j;
  EINX_PROF("lg_assign_nll (2 tile passes + lse + finish)", st);
  if (const int rc = assign_prologue(entry, st, a, w.s0, w.s1, n, m, B, d, nullptr)) return rc;
  hipLaunchKernelGGL((mnn_tile_kernel<7, true>), assign_grid(a, B), dim3(THREADS), 0, st, a);
  LG_CHECK(entry, 0);
  hipLaunchKernelGGL(lg_nll_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, a, gt_matches0, gt_matches1, out);
  LG_CHECK(entry, 0);
  return EINX_OK;
}
