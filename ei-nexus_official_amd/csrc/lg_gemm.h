// lg_gemm.h -- LightGlue's batched Linear: args, the two tile engines, the persistent 128x128 kernel, the 64x64 small-grid kernel,
// the call record and its launcher.  Part of lightglue.hip's translation unit, included only there (after D / DH / Side).
#pragma once

namespace {

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

// ---- the epilogues' per-element arithmetic, shared by both kernels (the load batching around it is each kernel's own tuning)
// W (which = 0) or bias (1) of entry b: the model's one (`plain`), or under EPI_DIV_HEAD that of the head b's pair stopped at
template <int EPI>
__device__ __forceinline__ const float* head_param(const GemmArgs& g, int b, int which, const float* plain) {
  return EPI == EPI_DIV_HEAD ? g.heads[4 * head_of(g.stop, g.pairs, g.nheads, b) + which] : plain;
}
template <int EPI>
__device__ __forceinline__ float gemm_finish(float acc, float bias, float old, float div) {
  float v = acc + bias;
  if (EPI == EPI_DIV || EPI == EPI_DIV_HEAD) v = v / div;
  if (EPI == EPI_RESID) v = old + v;
  return v;
}
// a column's index inside its head (any even head width)
template <int EPI>
__device__ __forceinline__ int col_in_head(int col, int rdh) {
  return EPI == EPI_ROPE ? (col & (DH - 1)) : col % rdh;
}
// rotate_half: (x0, x1) -> (-x1, x0), lightglue.py:151-158; partner: the other element of the rotary pair, the adjacent column =
// the neighbouring lane's value (the kernels fetch it with their own __shfl_xor: DESIGN.md 8o)
__device__ __forceinline__ float rope_rotate(float v, float partner, bool odd, float cs, float sn) {
  return (v * cs) + ((odd ? partner : -partner) * sn);
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
      s.B = reinterpret_cast<const WT*>(head_param<EPI>(g, b, 0, g.W));
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
  for (int Ln;; cur = nxt, b = nb, n = nn, L = Ln) {  // (the next tile, located below, becomes the current one)
    Ln = L + slots;
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
                const int hd = col_in_head<EPI>(hc[nt], rdh);
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
              const float partner = __shfl_xor(v, 1, 64);
              if (t < 2) v = rope_rotate(v, partner, odd, cs[r][nt], sn[r][nt]);
              if (i < n && (EPI == EPI_ROPE || hc[nt] < rd)) Yt[(size_t)i * rd + hc[nt]] = v;
            }
          }
        }
      if (!more) break;
      continue;
    }
    float* Y = g.Y + (size_t)b * g.cap * g.ldy;
    // epilogue: the bias of a lane's NT columns is loaded once; whole tiles take a guard-free path so
    // that the residual loads / stores of all 16*MT rows are issued back to back instead of one
    // load -> wait -> store round trip per element
    float bj[NT];
    int jj[NT];
    const float* bias = head_param<EPI>(g, b, 1, g.bias);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int j = j0 + col_of(nt);
      jj[nt] = j < g.N ? j : -1;
      bj[nt] = j < g.N ? bias[j] : 0.0f;
    }
    auto finish = [&](float acc, float bias, float old) { return gemm_finish<EPI>(acc, bias, old, g.div); };
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
    Wb = head_param<EPI>(g, b, 0, g.W);
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
        const int hd = col_in_head<EPI>(col, rdh);
        cs[r] = e[hd];
        sn[r] = e[rdh + hd];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[r] + bq;
      const float partner = __shfl_xor(v, 1, 64);
      if (t < 2) v = rope_rotate(v, partner, odd, cs[r], sn[r]);
      if (rows[r] < n) Yt[(size_t)rows[r] * rd + col] = v;
    }
    return;
  }
  float* Y = g.Y + (size_t)b * g.cap * g.ldy;
  const float bj = head_param<EPI>(g, b, 1, g.bias)[col];
  float old[16];
  if (EPI == EPI_RESID) {
#pragma unroll
    for (int r = 0; r < 16; ++r) old[r] = Y[(size_t)min(rows[r], n - 1) * g.ldy + col];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float v = gemm_finish<EPI>(acc[r], bj, EPI == EPI_RESID ? old[r] : 0.0f, g.div);
    if (rows[r] < n) Y[(size_t)rows[r] * g.ldy + col] = v;
  }
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

// One GEMM call: what the kernel reads (the GemmArgs it is) and what picks the kernel.  Value-initialised by gemm_call(), which
// fills the common case; a call site then names whatever else its call needs.
struct GemmCall : GemmArgs {
  int epi;
  const uint16_t* W16;  // non-null: the f16 tile engine on this binary16 image of W (`mp: True`)
  int rope_tiles;       // EPI_ROPE / EPI_ROPE_ANY: the launch's 128x128 tiles, three blocks (q | k | v) of whole tiles each
  bool bare;            // einx_linear: the wide f32 kernel whatever the grid, no profile scope, the launch status left to the caller
};

// Y[b, i, :N] = X[b, i, :K] @ W^T + bias (dense rows: ldx = K, ldy = N) for the first min(cnt[b], cap) rows of each of B entries
// (cnt null: cap rows)
GemmCall gemm_call(int epi, const int32_t* cnt, int cap, int B, const float* X, int K, const float* W, const float* bias, int N, float* Y) {
  GemmCall c{};
  c.epi = epi;
  c.cnt = cnt, c.cap = cap, c.B = B;
  c.X = X, c.ldx = K, c.K = K, c.Ksplit = 0x7fffffff;
  c.W = W, c.bias = bias, c.N = N;
  c.Y = Y, c.ldy = N;
  c.div = 1.0f;
  return c;
}
GemmCall gemm_call(int epi, const Side& s, int B, const float* X, int K, const float* W, const float* bias, int N, float* Y) {
  return gemm_call(epi, s.cnt, s.cap, B, X, K, W, bias, N, Y);
}

// (engine f32 | f16, form wide | small, EPI) -> instantiation.  The f16 engine (second column) has the wide kernel only, for
// EPI_BIAS / EPI_RESID / EPI_ROPE / EPI_ROPE_ANY -- no f16 twin of lg_gemm_small_kernel; anything else returns -1.
#define LG_GEMM_EPIS(X) X(EPI_BIAS, true) X(EPI_DIV, false) X(EPI_RESID, true) X(EPI_ROPE, true) X(EPI_ROPE_ANY, true) X(EPI_DIV_HEAD, false)
template <typename Eng, bool SMALL>
int launch_gemm_kernel(hipStream_t st, dim3 grid, int epi, const GemmArgs& g) {
  constexpr bool F16 = std::is_same<Eng, EngF16>::value;
  switch (epi) {
#define X(EPI, ON_F16)                                                                                   \
  case EPI:                                                                                              \
    if constexpr (SMALL) hipLaunchKernelGGL(lg_gemm_small_kernel<EPI>, grid, dim3(256), 0, st, g);       \
    else if constexpr (!F16 || ON_F16) hipLaunchKernelGGL((lg_gemm_kernel<EPI, Eng>), grid, dim3(THREADS), 0, st, g); \
    else return -1;                                                                                      \
    return 0;
    LG_GEMM_EPIS(X)
#undef X
  }
  return -1;
}

// The one GEMM launcher: the call record -> GemmArgs, the engine, the form, the grid, the profile scope, the launch.
//   f16 engine: always the wide kernel.
//   f32: the small kernel when small_grid() says so; the rope launch by its own rule on the tile count the caller passes in (three
//   whole-tile blocks: 3 cdiv(d, BN), not cdiv(3 d, BN)).
int launch_gemm(hipStream_t st, const GemmCall& c) {
  GemmArgs g = c;
  const bool rope = c.epi == EPI_ROPE || c.epi == EPI_ROPE_ANY;
  const int tiles = rope ? c.rope_tiles : einx_cdiv(c.N, BN) * einx_cdiv(c.cap, BM) * c.B;
  const bool small = !c.W16 && !c.bare && (rope ? tiles < 256 && c.d % SBN == 0 && c.d % SBK == 0 : small_grid(c.N, c.cap, c.B, c.K, c.Ksplit));
  if (c.W16 && (c.epi == EPI_DIV || c.epi == EPI_DIV_HEAD)) return -1;  // (refused before the scope opens; LG_GEMM_EPIS)
  std::optional<EinxProfScope> prof;
  if (!c.bare) prof.emplace(c.W16 ? "lg_gemm_kernel (f16)" : small ? "lg_gemm_small_kernel" : "lg_gemm_kernel", st);
  int rc;
  if (c.W16) {
    g.W = reinterpret_cast<const float*>(c.W16);
    rc = launch_gemm_kernel<EngF16, false>(st, dim3(gemm_grid<EngF16>(tiles)), c.epi, g);
  } else if (small) {
    rc = launch_gemm_kernel<EngF32, true>(st, dim3((unsigned)(c.N / SBN), (unsigned)einx_cdiv(c.cap, SBM), (unsigned)c.B), c.epi, g);
  } else {
    rc = launch_gemm_kernel<EngF32, false>(st, dim3(gemm_grid<>(tiles)), c.epi, g);
  }
  if (rc || c.bare) return rc;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace
