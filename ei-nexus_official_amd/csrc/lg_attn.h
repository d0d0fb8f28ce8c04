// lg_attn.h -- LightGlue's fused attention: args, the wide fp32 kernel, its small-grid latency form, the fp16 kernel of `flash: True`,
// the call record and its launcher.  Part of lightglue.hip's translation unit, included only there (after D / DH / crow / Dims).
#pragma once

namespace {

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

// The work item of a wide attention workgroup (lg_attn_kernel, lg_attn_f16_kernel): query block qb of head h of entry b, whose keys
// and values are entry bk's, and the two counts.  The query blocks of one (pair, head) read the same K / V: they are kept on one
// XCD (see xcd_contiguous).  (The Q / K / V bases stay in the kernels: DESIGN.md 8o.)
struct AttnItem { int qb, h, b, bk, nq, nk; };
__device__ __forceinline__ AttnItem attn_item(const AttnArgs& a) {
  AttnItem w;
  const int gx = (int)gridDim.x, gy = (int)gridDim.y;
  int item = xcd_contiguous((int)(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z)), gx * gy * (int)gridDim.z);
  w.qb = item % gx;
  item /= gx;
  w.h = item % gy, w.b = item / gy;
  w.bk = a.kv_shift ? (w.b + a.kv_shift) % a.Btot : w.b;
  w.nq = min(a.nq[w.b], a.capq), w.nk = min(a.nk[w.bk], a.capk);
  return w;
}

// One 32-key block of the online softmax (base 2) in the kernels' lane layout (lane = query lane % 32, its 16 values the keys
// kbase + crow(r, half)).  s: the raw products in, the probabilities 2^(s sl2 - m_new) out: scale and key mask (a whole block,
// uniform, takes none), the maximum across the two lane halves, the running maximum and per-half sum.  Returns alpha =
// 2^(m_run - m_new), the caller's rescale.  v_exp_f32 (2^x, ~1 ulp): LightGlue is compared at 1e-4, so the exact-order einx_expf
// is not needed here; 2^(-inf) = 0 handles masked keys and the first block
template <typename S>
__device__ __forceinline__ float softmax_step(S& s, int kbase, int nk, int half, float sl2, float& m_run, float& l_run) {
  const float NEG = -einx_u2f(0x7f800000u);
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
  return alpha;
}

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
  // Head widths that are not 32 / 64 / 128 (lightglue.py:456-461 takes any descriptor_dim // num_heads) run the next larger
  // instantiation on zero-padded heads (DD == 0 only): dims dhr .. HD - 1 of Q, K and V read as 0 -- exact zeros add nothing
  // to a dot product -- and are not stored.  The head's columns start at h * dhr.
  const int dhr = DD ? DH : a.dh;
  const AttnItem w = attn_item(a);
  const int h = w.h, b = w.b, bk = w.bk, nq = w.nq, nk = w.nk;
  const int q0 = w.qb * 128;
  if (q0 >= nq || nk <= 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q = q0 + wave * 32 + l31;
  const bool qv = q < nq;
  // MFMA K-step t pairs head dims (t, t + DH/2): lane half h supplies dim t + (DH/2) h, so a lane's K fragments
  // for four consecutive steps are one 16-byte LDS read
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
      const float alpha = softmax_step(s, kbase, nk, half, sl2, m_run, l_run);
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
      // (its own copy of softmax_step: through the helper the compiler unpacks the rescale of o)
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
  const int dhr = DD ? DH : a.dh;              // the head's real width; dims dhr .. HD - 1 read as zero and are not stored
  const AttnItem w = attn_item(a);
  const int h = w.h, b = w.b, bk = w.bk, nq = w.nq, nk = w.nk;
  const int q0 = w.qb * 128;
  if (q0 >= nq || nk <= 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int q = q0 + wave * 32 + l31;
  const bool qv = q < nq;
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
      const float alpha = softmax_step(s, kbase, nk, half, sl2, m_run, l_run);
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

// One attention call: what the kernels read (the AttnF16Args it is; ld, the row stride of Q / K / V, picks the instantiation on
// both paths: d, or 2 d when they are column blocks of the merged to_qk | to_v buffer) and the grid's other two factors.
struct AttnCall : AttnF16Args {
  int heads;
  bool f16;  // lg_attn_f16_kernel (conf.flash): one kernel for every grid size, no fp16 twin of lg_attn16_kernel
};

// the first min(nq[b], capq) queries of each of B entries against the keys / values of entry (b + kv_shift) mod B, rows of width d
AttnCall attn_call(const Dims& dm, int B, const float* Q, const int32_t* nq, int capq, const float* K, const float* V, const int32_t* nk, int capk,
                   float* O) {
  AttnCall c{};
  c.Q = Q, c.K = K, c.V = V, c.O = O;
  c.nq = nq, c.nk = nk, c.capq = capq, c.capk = capk;
  c.Btot = B;
  c.d = dm.d, c.dh = dm.dh, c.ld = dm.d, c.heads = dm.heads;
  c.scale = 1.0f / sqrtf((float)dm.dh);  // SDPA scale (self) = (dh^-1/4)^2 (cross, lightglue.py:316); 64-wide heads: exactly 0.125
  c.f16 = dm.flash;
  return c;
}

// the head-width ladder over a kernel family: the shipped widths at their two row strides as compile-time constants, any other
// configuration on the next wider instantiation (narrower heads: zero padded)
template <bool F16, int HD, int DD, int LD = 0>
void launch_attn_kernel(hipStream_t st, dim3 grid, const AttnCall& c) {
  if constexpr (F16) hipLaunchKernelGGL((lg_attn_f16_kernel<HD, DD, LD>), grid, dim3(256), 0, st, c);
  else hipLaunchKernelGGL((lg_attn_kernel<HD, DD, LD>), grid, dim3(256), 0, st, c);
}
template <bool F16>
int launch_attn_ladder(hipStream_t st, dim3 grid, const AttnCall& c) {
  const bool shipped = c.d == D && c.dh == DH;
  if (shipped && c.ld == 2 * D) launch_attn_kernel<F16, 64, D, 2 * D>(st, grid, c);
  else if (shipped && c.ld == D) launch_attn_kernel<F16, 64, D>(st, grid, c);
  else if (c.dh <= 32) launch_attn_kernel<F16, 32, 0>(st, grid, c);
  else if (c.dh <= 64) launch_attn_kernel<F16, 64, 0>(st, grid, c);
  else if (c.dh <= 128) launch_attn_kernel<F16, 128, 0>(st, grid, c);
  else if (c.dh <= 256) launch_attn_kernel<F16, 256, 0>(st, grid, c);
  else return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_attn(hipStream_t st, const AttnCall& c) {
  const dim3 grid((unsigned)einx_cdiv(c.capq, 128), (unsigned)c.heads, (unsigned)c.Btot);
  if (c.f16) {
    EINX_PROF("lg_attn_f16_kernel", st);
    return launch_attn_ladder<true>(st, grid, c);
  }
  const bool shipped = c.d == D && c.dh == DH, merged = c.ld == 2 * c.d;  // (fp32: shipped widths only; its <HD, 0> kernels take no stride)
  EINX_PROF("lg_attn_kernel", st);
  // the latency form (same bits) while ITS grid fits the chip twice: fewer wide workgroups than CUs alone is not enough -- three
  // pairs of 1024 keypoints (768 latency-form workgroups of eight waves, 1.5 rounds) ran 3.67 instead of 3.26 ms; one pair
  // 1.82 instead of 2.39 ms, two pairs 2.51 instead of 2.68 (tools/lg_bench.py --batch 1 / 2 / 3 --skip-linear)
  if (shipped && (long)grid.x * grid.y * grid.z < 256 && (long)einx_cdiv(c.capq, 32) * c.heads * c.Btot <= 512) {
    const dim3 g16((unsigned)einx_cdiv(c.capq, 32), (unsigned)c.heads, (unsigned)c.Btot);
    if (merged) hipLaunchKernelGGL(lg_attn16_kernel<2 * D>, g16, dim3(512), 0, st, c);
    else hipLaunchKernelGGL(lg_attn16_kernel<D>, g16, dim3(512), 0, st, c);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  if (merged && !shipped) return -1;
  return launch_attn_ladder<false>(st, grid, c);
}

}  // namespace
