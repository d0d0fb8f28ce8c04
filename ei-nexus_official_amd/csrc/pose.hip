// pose.hip -- relative pose of a batch of matched pairs on the device: RANSAC over Nister's five-point essential-matrix solver,
// then the cheirality vote of recoverPose and the error epilogue of RelativePoseEstimation.update_one.  The contract (generator,
// inlier rule, selection scan, candidate order) is DESIGN.md section 8b; tests/pose_f64.py restates it in float64 numpy.
//
// Replaces (reference file:line): core/metrics/matching_metrics.py:362-518 (cv2.findEssentialMat(RANSAC) + cv2.recoverPose +
// relative_pose_error), which ran on the host after a device-to-host copy.
//
// Launch sequence for B pairs with ragged nmatch, all on the caller's stream, no host synchronisation:
//   pose_norm_kernel     normalised matches (double), the per-pair RANSAC threshold
//   in rounds of iterations (32, 32, 64, 128, ...), each pair skipping the iterations at or past its current scan bound:
//   pose_solve_kernel    one wave per (iteration, pair): five draws, the minimal solver -> up to 10 E per sample
//   pose_score_kernel    one workgroup per (iteration, pair): Sampson inlier counts of the sample's models
//   ransac_select_kernel one lane per pair: OpenCV's sequential scan with its shrinking iteration bound, resumed per round
//   pose_recover_kernel  one workgroup per pair: decomposition, cheirality vote, mask, errors
//
// einx_relative_pose_refine (tests/pose_refine_f64.py) then fits such a pose to its Sampson inliers, opt-in:
//   pose_refine_norm_kernel  the same normalisation into the refinement's own workspace
//   pose_refine_kernel       one workgroup per pair: rounds of inlier selection + Levenberg-Marquardt, keep rule, mask, errors
#include "einx_common.h"
#include "ransac.h"

namespace {

constexpr int MAXS = 10;  // real solutions of one five-point sample

struct PoseWs {
  double4* xn;       // [B,cap] (u1, v1, u2, v2) normalised
  float* thr2;       // [B] (float)(thr * thr)
  double* E;         // [B,iters,MAXS,9]
  int32_t* nsol;     // [B,iters]
  int32_t* cnt;      // [B,iters,MAXS]
  RansacScan* scan;  // [B] best = iteration * 16 + solution
  uint8_t* cur;      // [B,cap] the recoverPose in/out mask
  uint8_t* ok;       // [B,cap] cheirality bits of the four candidates
};

// the workspace's regions; ws == nullptr: only their total size in *bytes
PoseWs carve(const einx_pose_params* p, void* ws, size_t* bytes = nullptr) {
  const size_t B = p->B, cap = p->cap, it = p->max_iters;
  WsCarver c{(char*)ws};
  PoseWs w;
  w.xn = c.take<double4>(B * cap);
  w.thr2 = c.take<float>(B);
  w.E = c.take<double>(B * it * MAXS * 9);
  w.nsol = c.take<int32_t>(B * it);
  w.cnt = c.take<int32_t>(B * it * MAXS);
  w.scan = c.take<RansacScan>(B);
  w.cur = c.take<uint8_t>(B * cap);
  w.ok = c.take<uint8_t>(B * cap);
  if (bytes) *bytes = c.bytes;
  return w;
}

// monomial x^ex y^ey z^ez (total degree 3 or less) -> column of Nister's ordering
// [x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1]
__device__ __forceinline__ int nister_col(int ex, int ey, int ez) {
  switch (ex * 16 + ey * 4 + ez) {
    case 48: return 0;   // x3
    case 12: return 1;   // y3
    case 36: return 2;   // x2y
    case 24: return 3;   // xy2
    case 33: return 4;   // x2z
    case 32: return 5;   // x2
    case 9: return 6;    // y2z
    case 8: return 7;    // y2
    case 21: return 8;   // xyz
    case 20: return 9;   // xy
    case 18: return 10;  // xz2
    case 17: return 11;  // xz
    case 16: return 12;  // x
    case 6: return 13;   // yz2
    case 5: return 14;   // yz
    case 4: return 15;   // y
    case 3: return 16;   // z3
    case 2: return 17;   // z2
    case 1: return 18;   // z
    default: return 19;  // 1
  }
}

// Gauss-Newton on det E = 0 and 2 E E^T E - tr(E E^T) E = 0 from a root of the degree-10 polynomial, evaluated on E(x, y, z) =
// Ec . (x, y, z, 1) itself: the ten cubics expanded over the monomials carry coefficients of |Ec|^3 that cancel, which leaves E
// 1e-8 off the essential variety on ill-conditioned samples (tests/pose_f64.py:_polish does the same from the eigenpairs)
__device__ void polish(const double (*Ec)[4], double* w, double& x, double& y, double& z) {
  double* E = w;         // w: 39 doubles of LDS of this lane's own: E, E E^T, E^T E and the cofactors, read by rolled loops
  double* G = w + 9;     // (all in registers and unrolled, a step takes 254 VGPRs and 316 bytes of scratch, one wave per SIMD)
  double* H = w + 18;
  double* cof = w + 27;
  double* dv = w + 36;   // one residual row of the Jacobian
#pragma unroll 1
  for (int step = 0; step < 12; ++step) {  // quadratic from a good root (three or four steps); a root of a cluster starts farther off
#pragma unroll 1
    for (int e = 0; e < 9; ++e) E[e] = Ec[e][0] * x + Ec[e][1] * y + Ec[e][2] * z + Ec[e][3];
#pragma unroll 1
    for (int i = 0; i < 3; ++i)
#pragma unroll 1
      for (int j = 0; j < 3; ++j) {
        G[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];  // E E^T
        H[3 * i + j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];                          // E^T E
      }
    const double tr = G[0] + G[4] + G[8];
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {
      const int a = r == 2 ? 0 : r + 1, b = r == 0 ? 2 : r - 1;
      cof[3 * r + 0] = E[3 * a + 1] * E[3 * b + 2] - E[3 * a + 2] * E[3 * b + 1];
      cof[3 * r + 1] = E[3 * a + 2] * E[3 * b + 0] - E[3 * a + 0] * E[3 * b + 2];
      cof[3 * r + 2] = E[3 * a + 0] * E[3 * b + 1] - E[3 * a + 1] * E[3 * b + 0];
    }
    // J'J and J'r one residual row at a time: the Jacobian is never held
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    auto row = [&](double res, double d0, double d1, double d2) {
      a00 += d0 * d0;
      a01 += d0 * d1;
      a02 += d0 * d2;
      a11 += d1 * d1;
      a12 += d1 * d2;
      a22 += d2 * d2;
      g0 += d0 * res;
      g1 += d1 * res;
      g2 += d2 * res;
    };
    double ed[3] = {0.0, 0.0, 0.0}, dd[3] = {0.0, 0.0, 0.0};  // <E, dE/dv> and the derivative of det E, dE/dv = Ec[.][v]
#pragma unroll 1
    for (int e = 0; e < 9; ++e) {
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        ed[v] += E[e] * Ec[e][v];
        dd[v] += cof[e] * Ec[e][v];
      }
    }
    row(E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2], dd[0], dd[1], dd[2]);
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
#pragma unroll 1
      for (int j = 0; j < 3; ++j) {
        // the (i, j) loops stay rolled and their LDS loads inside them: hoisted, the loop-invariant operands alone take 100 VGPRs
        __asm__ volatile("" ::: "memory");
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          double dh = 0.0, fe = 0.0, gd = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double f = E[3 * i] * Ec[3 * k][v] + E[3 * i + 1] * Ec[3 * k + 1][v] + E[3 * i + 2] * Ec[3 * k + 2][v];  // (E dE^T)[i][k]
            dh += Ec[3 * i + k][v] * H[3 * k + j];
            fe += f * E[3 * k + j];
            gd += G[3 * i + k] * Ec[3 * k + j][v];
          }
          dv[v] = 2.0 * (dh + fe + gd) - 2.0 * ed[v] * E[3 * i + j] - tr * Ec[3 * i + j][v];
        }
        __asm__ volatile("" ::: "memory");
        const double res = 2.0 * (G[3 * i] * E[j] + G[3 * i + 1] * E[3 + j] + G[3 * i + 2] * E[6 + j]) - tr * E[3 * i + j];
        row(res, dv[0], dv[1], dv[2]);
      }
    }
    // (J'J) delta = -J'r by Cramer's rule
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double dx = -(c00 * g0 + c01 * g1 + c02 * g2) / det;
    const double dy = -(c01 * g0 + c11 * g1 + c12 * g2) / det;
    const double dz = -(c02 * g0 + c12 * g1 + c22 * g2) / det;
    if (!(isfinite(dx) && isfinite(dy) && isfinite(dz))) break;
    x += dx;
    y += dy;
    z += dz;
    // quadratic convergence: after a step this small the next one is below the rounding of (x, y, z)
    if (fmax(fabs(dx), fmax(fabs(dy), fabs(dz))) <= 1e-9 * (1.0 + fmax(fabs(x), fmax(fabs(y), fabs(z))))) break;
  }
}

template <int NA, int NB>
__device__ __forceinline__ void pmul(const double* a, const double* b, double* c) {
#pragma unroll
  for (int i = 0; i < NA + NB - 1; ++i) c[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) c[i + j] += a[i] * b[j];
}

__device__ __forceinline__ double horner(const double* c, int n, double x) {
  double v = c[n];
  for (int i = n - 1; i >= 0; --i) v = v * x + c[i];
  return v;
}

struct SolveLds {
  double A[5][9];
  double Ec[9][4];
  double T[10][64];
  double M[10][20];
  double fac[10];
  double D[11][11];   // p and its derivatives, coefficients ascending: D[k] = k-th derivative (degree n - k)
  double crit[12];    // sorted real roots of the level below (critical points of the current level), bracketed by -+bound
  double found[12];
  int has[12];
  int n, ncrit;
  double bound;
  double Bz[6][10];   // rows 4..9 of the reduced system, basis part
  double sol[MAXS][9];
  int valid[MAXS];
  double pw[MAXS][39];  // the polish's working set of each solution's lane
};

// the five-point solver for one sample, one 64-lane workgroup: x[5] = (u1, v1, u2, v2).  Writes the solutions ordered by
// ascending z = E[2,1] / E[2,2] (E[2,2] = 1) to E_out[MAXS][9] and returns their count (lane 0's value is authoritative).
__device__ int solve5(SolveLds& L, const double4* x, double* E_out) {
  const int lane = threadIdx.x;
  if (lane < 45) {
    const int r = lane / 9, c = lane % 9;
    const double4 q = x[r];
    const double a2 = (c / 3 == 0) ? q.z : (c / 3 == 1) ? q.w : 1.0;
    const double a1 = (c % 3 == 0) ? q.x : (c % 3 == 1) ? q.y : 1.0;
    L.A[r][c] = (c / 3 == 2) ? a1 : (c % 3 == 2 ? a2 : a2 * a1);
  }
  __syncthreads();
  // Gauss-Jordan with partial pivoting over the first five columns (tests/pose_f64.py:null_basis)
  double amax = 0.0;
  for (int i = 0; i < 45; ++i) amax = fmax(amax, fabs(L.A[i / 9][i % 9]));
  if (!gauss_jordan<5, 9>(L.A, L.fac, 1e-9 * amax)) return 0;  // uniform across the workgroup
  if (lane < 36) {
    const int e = lane / 4, k = lane % 4;
    L.Ec[e][k] = e < 5 ? -L.A[e][5 + k] : (e - 5 == k ? 1.0 : 0.0);
  }
  __syncthreads();
  // the ten cubics, one lane per product (a, b, c) of three linear forms over (x, y, z, 1)
  {
    const int a = lane >> 4, b = (lane >> 2) & 3, c = lane & 3;
    auto e = [&](int i, int j, int k) { return L.Ec[3 * i + j][k]; };
    double det = e(0, 0, a) * e(1, 1, b) * e(2, 2, c) + e(0, 1, a) * e(1, 2, b) * e(2, 0, c) + e(0, 2, a) * e(1, 0, b) * e(2, 1, c) -
                 e(0, 0, a) * e(1, 2, b) * e(2, 1, c) - e(0, 1, a) * e(1, 0, b) * e(2, 2, c) - e(0, 2, a) * e(1, 1, b) * e(2, 0, c);
    L.T[0][lane] = det;
    double tr = 0.0;
    for (int m = 0; m < 3; ++m)
      for (int l = 0; l < 3; ++l) tr += e(m, l, a) * e(m, l, b);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double t1 = 0.0;
        for (int k = 0; k < 3; ++k)
          for (int l = 0; l < 3; ++l) t1 += e(i, l, a) * e(k, l, b) * e(k, j, c);
        L.T[1 + 3 * i + j][lane] = 2.0 * t1 - tr * e(i, j, c);
      }
  }
  __syncthreads();
  for (int q = lane; q < 200; q += 64) {
    const int r = q / 20, col = q % 20;
    double s = 0.0;
    for (int t = 0; t < 64; ++t) {
      const int a = t >> 4, b = (t >> 2) & 3, c = t & 3;
      const int ex = (a == 0) + (b == 0) + (c == 0), ey = (a == 1) + (b == 1) + (c == 1), ez = (a == 2) + (b == 2) + (c == 2);
      if (nister_col(ex, ey, ez) == col) s += L.T[r][t];
    }
    L.M[r][col] = s;
  }
  __syncthreads();
  double mmax = 0.0;
  for (int i = 0; i < 100; ++i) mmax = fmax(mmax, fabs(L.M[i / 10][i % 10]));
  if (!gauss_jordan<10, 20>(L.M, L.fac, 1e-13 * mmax)) return 0;
  if (lane < 60) L.Bz[lane / 10][lane % 10] = L.M[4 + lane / 10][10 + lane % 10];
  __syncthreads();
  // <k> = <e> - z<f>, <l> = <g> - z<h>, <m> = <i> - z<j>: a 3x3 matrix of polynomials in z acting on (x, y, 1);
  // its determinant is the degree-10 polynomial (coefficients ascending in z)
  if (lane == 0) {
    double px[3][4], py[3][4], p1[3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double* u = L.Bz[2 * r];
      const double* v = L.Bz[2 * r + 1];
      px[r][0] = u[2];
      px[r][1] = u[1] - v[2];
      px[r][2] = u[0] - v[1];
      px[r][3] = -v[0];
      py[r][0] = u[5];
      py[r][1] = u[4] - v[5];
      py[r][2] = u[3] - v[4];
      py[r][3] = -v[3];
      p1[r][0] = u[9];
      p1[r][1] = u[8] - v[9];
      p1[r][2] = u[7] - v[8];
      p1[r][3] = u[6] - v[7];
      p1[r][4] = -v[6];
    }
    double a7[8], b7[8], c6[7], d6[7], t7[8], t6[7], r1[11], r2[11], r3[11];
    pmul<4, 5>(py[1], p1[2], a7);
    pmul<5, 4>(p1[1], py[2], b7);
#pragma unroll
    for (int i = 0; i < 8; ++i) t7[i] = a7[i] - b7[i];
    pmul<4, 8>(px[0], t7, r1);
    pmul<4, 5>(px[1], p1[2], a7);
    pmul<5, 4>(p1[1], px[2], b7);
#pragma unroll
    for (int i = 0; i < 8; ++i) t7[i] = a7[i] - b7[i];
    pmul<4, 8>(py[0], t7, r2);
    pmul<4, 4>(px[1], py[2], c6);
    pmul<4, 4>(py[1], px[2], d6);
#pragma unroll
    for (int i = 0; i < 7; ++i) t6[i] = c6[i] - d6[i];
    pmul<5, 7>(p1[0], t6, r3);
    double pmax = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      L.D[0][i] = r1[i] - r2[i] + r3[i];
      pmax = fmax(pmax, fabs(L.D[0][i]));
    }
    int n = 10;
    // solutions far out in z (|E[2,2]| small against E[2,1]) come with leading coefficients many orders below the largest one,
    // so magnitude alone does not tell such a coefficient from a true zero computed as rounding noise: only one below 1e-30 of
    // the largest lowers the degree.  A noise coefficient that stays adds a root near +-1e16, which the polish on E either
    // turns into a solution or leaves to the det E guard; its bracket of up to +-2e30 is why the bisection below may take 300
    // halvings (2e30 down to a root of 1e-10 at full precision takes about 240)
    while (n > 0 && !(fabs(L.D[0][n]) > 1e-30 * pmax)) --n;
    L.n = (pmax > 0.0) ? n : 0;
    double cb = 0.0;
    for (int k = 1; k <= n; ++k) cb = fmax(cb, pow(fabs(L.D[0][n - k] / L.D[0][n]), 1.0 / k));
    L.bound = 2.0 * cb + 1.0;  // Fujiwara: every root of p (and, by Gauss-Lucas, of its derivatives) lies inside
    for (int k = 1; k <= n; ++k)
      for (int i = 0; i <= n - k; ++i) L.D[k][i] = (i + 1) * L.D[k - 1][i + 1];
    L.ncrit = 0;
  }
  __syncthreads();
  // real roots level by level, from p^(n-1) (linear) up to p: between two consecutive real roots of p^(k+1), p^(k) is monotonic
  // and has a root there iff it changes sign; one lane bisects each such interval.  Distinct real roots, ascending.
  const int n = L.n;
  for (int k = n - 1; k >= 0; --k) {
    const int m = L.ncrit;  // intervals: (-bound, c0], (c0, c1], ..., (c_{m-1}, bound]
    const double* c = L.D[k];
    const int dk = n - k;
    if (lane <= m) {
      double lo = lane == 0 ? -L.bound : L.crit[lane - 1];
      double hi = lane == m ? L.bound : L.crit[lane];
      const double flo = horner(c, dk, lo), fhi = horner(c, dk, hi);
      int got = 0;
      double r = hi;
      if (fhi == 0.0) {
        got = 1;
      } else if (flo != 0.0 && ((flo < 0.0) != (fhi < 0.0)) && lo < hi) {
        const bool neg_lo = flo < 0.0;
        for (int it = 0; it < 300; ++it) {
          const double mid = 0.5 * (lo + hi);
          if (!(mid > lo && mid < hi)) break;
          const double fm = horner(c, dk, mid);
          if (fm == 0.0) {
            lo = hi = mid;
            break;
          }
          if ((fm < 0.0) == neg_lo)
            lo = mid;
          else
            hi = mid;
        }
        r = 0.5 * (lo + hi);
        got = 1;
      }
      L.has[lane] = got;
      L.found[lane] = r;
    }
    __syncthreads();
    if (lane == 0) {
      int q = 0;
      for (int j = 0; j <= m; ++j)
        if (L.has[j] && (q == 0 || L.found[j] > L.crit[q - 1])) L.crit[q++] = L.found[j];
      L.ncrit = q;
    }
    __syncthreads();
  }
  const int nr = min(L.ncrit, MAXS);
  if (lane < nr) {
    double z = L.crit[lane];
  // (x, y, 1) spans the null space of the 3x3 matrix at z: largest cross product of two of its rows
    double Bm[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double* u = L.Bz[2 * r];
      const double* v = L.Bz[2 * r + 1];
      const double z2 = z * z, z3 = z2 * z;
      Bm[r][0] = u[2] + (u[1] - v[2]) * z + (u[0] - v[1]) * z2 - v[0] * z3;
      Bm[r][1] = u[5] + (u[4] - v[5]) * z + (u[3] - v[4]) * z2 - v[3] * z3;
      Bm[r][2] = u[9] + (u[8] - v[9]) * z + (u[7] - v[8]) * z2 + (u[6] - v[7]) * z3 - v[6] * z3 * z;
    }
    double best = -1.0, cx = 0.0, cy = 0.0, cz = 0.0;
#pragma unroll
    for (int pr = 0; pr < 3; ++pr) {
      const int i = pr == 2 ? 1 : 0, j = pr == 0 ? 1 : 2;
      const double x0 = Bm[i][1] * Bm[j][2] - Bm[i][2] * Bm[j][1];
      const double x1 = Bm[i][2] * Bm[j][0] - Bm[i][0] * Bm[j][2];
      const double x2 = Bm[i][0] * Bm[j][1] - Bm[i][1] * Bm[j][0];
      const double nn = x0 * x0 + x1 * x1 + x2 * x2;
      if (nn > best) {
        best = nn;
        cx = x0;
        cy = x1;
        cz = x2;
      }
    }
    double sx = cx / cz, sy = cy / cz;
    polish(L.Ec, L.pw[lane], sx, sy, z);
    bool good = true;
    double ev[9], en = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      ev[e] = L.Ec[e][0] * sx + L.Ec[e][1] * sy + L.Ec[e][2] * z + L.Ec[e][3];
      L.sol[lane][e] = ev[e];
      good &= isfinite(ev[e]);
      en += ev[e] * ev[e];
    }
    // a root lost to cancellation in the degree-10 polynomial gives a matrix off the essential variety: det E must stay below
    // 1e-6 |E|^3 (Frobenius; tests/pose_f64.py:solve5 applies the same test)
    en = sqrt(en);
    const double det = ev[0] * (ev[4] * ev[8] - ev[5] * ev[7]) - ev[1] * (ev[3] * ev[8] - ev[5] * ev[6]) + ev[2] * (ev[3] * ev[7] - ev[4] * ev[6]);
    good &= fabs(det) <= 1e-6 * en * en * en;
    L.valid[lane] = good;
  }
  __syncthreads();
  int ns = 0;
  for (int k = 0; k < nr; ++k) {
    if (!L.valid[k]) continue;
    if (lane < 9) E_out[ns * 9 + lane] = L.sol[k][lane];
    ++ns;
  }
  return ns;
}

struct PoseArgs {
  const float *mk0, *mk1;
  const int32_t* nmatch;
  const void *K0, *K1;
  const void* T;
  double *R_out, *t_out, *rows_out;
  uint8_t* mask_out;
  int32_t* status;
  PoseWs w;
  einx_pose_params p;
};

template <typename KT>
__device__ __forceinline__ void norm_pair(const PoseArgs& a, int b, int t) {
  const KT* K0 = (const KT*)a.K0 + b * 9;
  const KT* K1 = (const KT*)a.K1 + b * 9;
  const int cols = a.p.cols, xi = a.p.kp_yx ? 1 : 0, yi = a.p.kp_yx ? 0 : 1;
  const float* q0 = a.mk0 + ((size_t)b * a.p.cap + t) * cols;
  const float* q1 = a.mk1 + ((size_t)b * a.p.cap + t) * cols;
  // numpy's dtype: float32 keypoints with a float32 K stay float32, a float64 K promotes; widened to double afterwards
  const double u1 = (double)(((KT)q0[xi] - K0[2]) / K0[0]), v1 = (double)(((KT)q0[yi] - K0[5]) / K0[4]);
  const double u2 = (double)(((KT)q1[xi] - K1[2]) / K1[0]), v2 = (double)(((KT)q1[yi] - K1[5]) / K1[4]);
  a.w.xn[(size_t)b * a.p.cap + t] = make_double4(u1, v1, u2, v2);
  if (t == 0) {
    // thresh / np.mean([K0[0,0], K1[1,1], K0[0,0], K1[1,1]]): K's dtype, summed left to right
    const KT f0 = K0[0], f1 = K1[4];
    const KT m = (((f0 + f1) + f0) + f1) / (KT)4;
    const double thr = (double)((KT)a.p.thresh / m);
    a.w.thr2[b] = (float)(thr * thr);
  }
}

__global__ void pose_norm_kernel(const PoseArgs a) {
  const int b = blockIdx.y;
  const int n = min(a.nmatch[b], a.p.cap);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) ransac_scan_init(a.w.scan[b], a.p.max_iters);
  if (t >= n) return;
  if (a.p.k_f64)
    norm_pair<double>(a, b, t);
  else
    norm_pair<float>(a, b, t);
}

// one round of iterations [it0, it0 + gridDim.x)
__global__ __launch_bounds__(64) void pose_solve_kernel(const PoseArgs a, int it0) {
  __shared__ SolveLds L;
  __shared__ double4 xs[5];
  const int it = it0 + blockIdx.x, b = blockIdx.y;
  const int n = min(a.nmatch[b], a.p.cap);
  int32_t* nsol = a.w.nsol + (size_t)b * a.p.max_iters + it;
  double* E = a.w.E + ((size_t)b * a.p.max_iters + it) * MAXS * 9;
  // n == 5: OpenCV solves the one sample and keeps every solution (iteration 0 holds it); n < 5: no pose
  if (n < 5 || (n == 5 && it > 0) || !ransac_live(a.w.scan[b], it)) {
    if (threadIdx.x == 0) *nsol = 0;
    return;
  }
  int idx[5] = {0, 1, 2, 3, 4};
  if (n > 5 && !ransac_draw<5>(a.p.seed, it, 0, n, idx)) {
    if (threadIdx.x == 0) *nsol = 0;
    return;
  }
  int mine = 0;
#pragma unroll
  for (int e = 0; e < 5; ++e)
    if ((int)threadIdx.x == e) mine = idx[e];
  if (threadIdx.x < 5) xs[threadIdx.x] = a.w.xn[(size_t)b * a.p.cap + mine];
  __syncthreads();
  const int ns = solve5(L, xs, E);
  if (threadIdx.x == 0) *nsol = ns;
}

__global__ __launch_bounds__(64) void essential_5pt_kernel(const double* x1, const double* x2, double* E_out, int32_t* n_out) {
  __shared__ SolveLds L;
  __shared__ double4 xs[5];
  const int pb = blockIdx.x;
  if (threadIdx.x < 5) {
    const double* p1 = x1 + ((size_t)pb * 5 + threadIdx.x) * 2;
    const double* p2 = x2 + ((size_t)pb * 5 + threadIdx.x) * 2;
    xs[threadIdx.x] = make_double4(p1[0], p1[1], p2[0], p2[1]);
  }
  __syncthreads();
  const int ns = solve5(L, xs, E_out + (size_t)pb * MAXS * 9);
  if (threadIdx.x == 0) n_out[pb] = ns;
}

// OpenCV EMEstimatorCallback::computeError, rounded to float
__device__ __forceinline__ float sampson(const double* e, const double4 q) {
  const double x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
  const double a = e[0] * x1 + e[1] * y1 + e[2];
  const double b = e[3] * x1 + e[4] * y1 + e[5];
  const double c = e[6] * x1 + e[7] * y1 + e[8];
  const double s2 = e[0] * x2 + e[3] * y2 + e[6];
  const double s1 = e[1] * x2 + e[4] * y2 + e[7];
  const double d1 = x2 * a + y2 * b + c;
  return (float)(d1 * d1 / (a * a + b * b + s2 * s2 + s1 * s1));
}

// inlier counts of one round's models: each thread holds a tile point, the sample's models are read from LDS one at a time
// and every wave adds the popcount of its ballot to its own LDS counter (no per-model register arrays)
__global__ __launch_bounds__(256) void pose_score_kernel(const PoseArgs a, int it0) {
  __shared__ double Es[MAXS * 9];
  __shared__ int red[4][MAXS];
  const int it = it0 + blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = min(a.nmatch[b], a.p.cap);
  if (n <= 5 || !ransac_live(a.w.scan[b], it)) return;
  const size_t h = (size_t)b * a.p.max_iters + it;
  const int ns = a.w.nsol[h];
  if (ns == 0) return;
  if (tid < ns * 9) Es[tid] = a.w.E[h * MAXS * 9 + tid];
  if (tid < 4 * MAXS) red[tid / MAXS][tid % MAXS] = 0;
  __syncthreads();
  const float thr2 = a.w.thr2[b];
  const int wv = tid >> 6, lane = tid & 63;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + tid;
    const bool valid = j < n;
    const double4 q = a.w.xn[(size_t)b * a.p.cap + (valid ? j : 0)];
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
      const bool in = valid && sampson(Es + 9 * s, q) <= thr2;  // a NaN error is never an inlier
      const unsigned long long m = __ballot(in);
      if (lane == 0) red[wv][s] += __popcll(m);
    }
  }
  __syncthreads();
  if (tid < ns) a.w.cnt[h * MAXS + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// the models of one iteration for the selection scan
struct PoseModels {
  const int32_t *nsol, *cnt;
  __device__ int count(size_t h) const { return nsol[h]; }
  __device__ int inliers(size_t h, int s) const { return cnt[h * MAXS + s]; }
};

// DLT triangulation against [I|0] and [R|t] (smallest eigenvector of A^T A, cyclic Jacobi) and recoverPose's depth tests
__device__ bool cheiral(const double* R, const double* t, const double4 q) {
  const double dist = 1e9;
  double A[4][4] = {{-1.0, 0.0, q.x, 0.0},
                    {0.0, -1.0, q.y, 0.0},
                    {q.z * R[6] - R[0], q.z * R[7] - R[1], q.z * R[8] - R[2], q.z * t[2] - t[0]},
                    {q.w * R[6] - R[3], q.w * R[7] - R[4], q.w * R[8] - R[5], q.w * t[2] - t[1]}};
  double S[4][4], V[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) s += A[k][i] * A[k][j];
      S[i][j] = s;
      V[i][j] = i == j ? 1.0 : 0.0;
    }
#pragma unroll
  for (int sweep = 0; sweep < 8; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        const double apq = S[p][r];
        if (apq == 0.0) continue;
        const double theta = (S[r][r] - S[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double skp = S[k][p], skr = S[k][r];
          S[k][p] = c * skp - s * skr;
          S[k][r] = s * skp + c * skr;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double spk = S[p][k], srk = S[r][k];
          S[p][k] = c * spk - s * srk;
          S[r][k] = s * spk + c * srk;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkr = V[k][r];
          V[k][p] = c * vkp - s * vkr;
          V[k][r] = s * vkp + c * vkr;
        }
      }
  }
  double X[4], ev = S[0][0];
#pragma unroll
  for (int k = 0; k < 4; ++k) X[k] = V[k][0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (S[i][i] < ev) {
      ev = S[i][i];
#pragma unroll
      for (int k = 0; k < 4; ++k) X[k] = V[k][i];
    }
  if (!(X[2] * X[3] > 0.0)) return false;
  const double x = X[0] / X[3], y = X[1] / X[3], z = X[2] / X[3];
  const double z2 = R[6] * x + R[7] * y + R[8] * z + t[2];
  return z < dist && z2 > 0.0 && z2 < dist;
}

// (R1, R2, t) of E scaled to Frobenius norm sqrt(2): t = unit left null vector (largest cross product of two columns),
// R1 = cof(E) - [t]x E, R2 = cof(E) + [t]x E (tests/pose_f64.py:decompose)
__device__ void decompose(const double* e0, double* R1, double* R2, double* t) {
  double nn = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) nn += e0[i] * e0[i];
  const double sc = sqrt(2.0) / sqrt(nn);
  double E[9];
  for (int i = 0; i < 9; ++i) E[i] = e0[i] * sc;
  double best = -1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = k == 2 ? 1 : 0, j = k == 0 ? 1 : 2;
    const double c0 = E[3 + i] * E[6 + j] - E[6 + i] * E[3 + j];
    const double c1 = E[6 + i] * E[0 + j] - E[0 + i] * E[6 + j];
    const double c2 = E[0 + i] * E[3 + j] - E[3 + i] * E[0 + j];
    const double n2 = c0 * c0 + c1 * c1 + c2 * c2;
    if (n2 > best) {
      best = n2;
      t[0] = c0;
      t[1] = c1;
      t[2] = c2;
    }
  }
  const double tn = sqrt(best);
  t[0] /= tn;
  t[1] /= tn;
  t[2] /= tn;
  // cofactor rows: r0 x r1 ordering as tests/pose_f64.py:cofactor
  double C[9];
  for (int r = 0; r < 3; ++r) {
    const int a = (r + 1) % 3, b = (r + 2) % 3;
    C[3 * r + 0] = E[3 * a + 1] * E[3 * b + 2] - E[3 * a + 2] * E[3 * b + 1];
    C[3 * r + 1] = E[3 * a + 2] * E[3 * b + 0] - E[3 * a + 0] * E[3 * b + 2];
    C[3 * r + 2] = E[3 * a + 0] * E[3 * b + 1] - E[3 * a + 1] * E[3 * b + 0];
  }
  const double sk[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double s = sk[3 * i] * E[j] + sk[3 * i + 1] * E[3 + j] + sk[3 * i + 2] * E[6 + j];
      R1[3 * i + j] = C[3 * i + j] - s;
      R2[3 * i + j] = C[3 * i + j] + s;
    }
}

// relative_pose_error + update_one (matching_metrics.py:452-518): R_err, t_err, pose_err of (R, t) against T [4,4] into rows[0..2]
__device__ void pose_error_rows(const double* R, const double* t, const double* T, double* rows) {
  const double tg0 = T[3], tg1 = T[7], tg2 = T[11];
  const double ngt = sqrt(tg0 * tg0 + tg1 * tg1 + tg2 * tg2);
  const double nrm = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) * ngt;
  const double rad2deg = 57.29577951308232;
  double c = (t[0] * tg0 + t[1] * tg1 + t[2] * tg2) / nrm;
  if (!isnan(c)) c = fmin(fmax(c, -1.0), 1.0);
  double t_err = acos(c) * rad2deg;
  t_err = isnan(t_err) ? t_err : fmin(t_err, 180.0 - t_err);
  if (!isfinite(ngt)) t_err = 0.0;
  double tr = 0.0;
  for (int i = 0; i < 3; ++i) {
    double d = 0.0;
    for (int k = 0; k < 3; ++k) d += R[3 * k + i] * T[4 * k + i];
    tr += d;
  }
  double cs = (tr - 1.0) / 2.0;
  if (!isnan(cs)) cs = fmin(fmax(cs, -1.0), 1.0);
  const double R_err = fabs(acos(cs)) * rad2deg;
  rows[0] = R_err;
  rows[1] = t_err;
  rows[2] = isfinite(t_err) ? fmax(R_err, t_err) : R_err;
}

__global__ __launch_bounds__(256) void pose_recover_kernel(const PoseArgs a) {
  __shared__ double cand[4][12];  // (R, t) of (R1,t), (R2,t), (R1,-t), (R2,-t)
  __shared__ int red[4][4];
  __shared__ double keepR[12];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(a.nmatch[b], a.p.cap);
  const size_t cap = a.p.cap;
  uint8_t* mout = a.mask_out + b * cap;
  uint8_t* cur = a.w.cur + b * cap;
  uint8_t* okb = a.w.ok + b * cap;
  const double4* xn = a.w.xn + b * cap;
  for (size_t j = tid; j < cap; j += 256) mout[j] = 0;
  int status = n < 5 ? -1 : -2, nmodels = 0;
  const double* models = nullptr;
  if (n == 5) {
    nmodels = a.w.nsol[(size_t)b * a.p.max_iters];
    models = a.w.E + (size_t)b * a.p.max_iters * MAXS * 9;
    for (int j = tid; j < n; j += 256) cur[j] = 1;
  } else if (n > 5 && a.w.scan[b].best >= 0) {
    const int bi = a.w.scan[b].best;
    nmodels = 1;
    models = a.w.E + (((size_t)b * a.p.max_iters + (bi >> 4)) * MAXS + (bi & 15)) * 9;
    const float thr2 = a.w.thr2[b];
    for (int j = tid; j < n; j += 256) cur[j] = sampson(models, xn[j]) <= thr2;
  }
  __syncthreads();
  int best_n = 0;
  for (int s = 0; s < nmodels; ++s) {
    if (tid == 0) {
      double R1[9], R2[9], t[3];
      decompose(models + 9 * s, R1, R2, t);
      for (int k = 0; k < 4; ++k) {
        const double* R = (k & 1) ? R2 : R1;
        const double sg = k < 2 ? 1.0 : -1.0;
        for (int i = 0; i < 9; ++i) cand[k][i] = R[i];
        for (int i = 0; i < 3; ++i) cand[k][9 + i] = sg * t[i];
      }
    }
    __syncthreads();
    int c[4] = {0, 0, 0, 0};
    for (int j = tid; j < n; j += 256) {
      uint8_t bits = 0;
      if (cur[j]) {
        const double4 q = xn[j];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (cheiral(cand[k], cand[k] + 9, q)) {
            bits |= (uint8_t)(1 << k);
            ++c[k];
          }
      }
      okb[j] = bits;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int v = c[k];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    int g[4], kbest = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (g[k] > g[kbest]) kbest = k;  // the first maximum: OpenCV's if / else-if chain of >=
    const int ng = g[kbest];
    // recoverPose writes the chosen candidate's mask into the in/out mask
    for (int j = tid; j < n; j += 256) cur[j] = (okb[j] >> kbest) & 1;
    __syncthreads();
    if (ng > best_n) {
      best_n = ng;
      status = n == 5 ? s : a.w.scan[b].best;
      if (tid < 12) keepR[tid] = cand[kbest][tid];
      for (int j = tid; j < n; j += 256) mout[j] = cur[j];
    }
    __syncthreads();
  }
  if (n >= 5 && best_n == 0 && nmodels > 0) status = -3;
  if (tid != 0) return;
  a.status[b] = status;
  double* Ro = a.R_out + (size_t)b * 9;
  double* to = a.t_out + (size_t)b * 3;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double* rows = a.rows_out ? a.rows_out + (size_t)b * 4 : nullptr;
  if (status < 0) {
    for (int i = 0; i < 9; ++i) Ro[i] = 0.0;
    for (int i = 0; i < 3; ++i) to[i] = 0.0;
    if (rows) {
      rows[0] = rows[1] = rows[2] = inf;
      rows[3] = 0.0;
    }
    return;
  }
  for (int i = 0; i < 9; ++i) Ro[i] = keepR[i];
  for (int i = 0; i < 3; ++i) to[i] = keepR[9 + i];
  if (!rows) return;
  rows[3] = (double)best_n / (double)n;  // mask.mean()
  if (!a.T) {
    rows[0] = rows[1] = rows[2] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  pose_error_rows(keepR, keepR + 9, (const double*)a.T + (size_t)b * 16, rows);
}

// ---------------------------------------------------------------------------------------------- refinement on the inliers (8w)
// Levenberg-Marquardt on the signed Sampson distances of the current Sampson inliers over the five parameters of E = [t]x R
// (R <- exp([w]x) R, t moved in its tangent plane and renormalised), in rounds that re-select the inliers; the refined pose is
// kept when a step was accepted and its inlier count is not below the input pose's.  tests/pose_refine_f64.py restates it.
constexpr double FLT_EPS = 1.1920928955078125e-07;
constexpr int RF_MIN_SET = 6;  // a round needs this many Sampson inliers: five parameters and one to spare
constexpr int RF_SUMS = 21;    // J^T J (packed upper 5x5: 15), J^T r (5), |r|^2

struct RefineWs {
  double4* xn;   // [B,cap] (u1, v1, u2, v2) normalised
  float* thr2;   // [B] (float)(thr * thr)
  uint8_t* inl;  // [B,cap] the current round's set; in the end the Sampson inliers of the refined pose
};

// the workspace's regions; ws == nullptr: only their total size in *bytes
RefineWs carve(const einx_pose_refine_params* p, void* ws, size_t* bytes = nullptr) {
  const size_t B = p->B, cap = p->cap;
  WsCarver c{(char*)ws};
  RefineWs w;
  w.xn = c.take<double4>(B * cap);
  w.thr2 = c.take<float>(B);
  w.inl = c.take<uint8_t>(B * cap);
  if (bytes) *bytes = c.bytes;
  return w;
}

bool refine_params_ok(const einx_pose_refine_params* p) {
  return p && p->struct_size == sizeof(einx_pose_refine_params) && p->B > 0 && p->cap > 0 && (p->cols == 2 || p->cols == 3) &&
         (p->kp_yx == 0 || p->kp_yx == 1) && (p->k_f64 == 0 || p->k_f64 == 1) && p->rounds >= 1 && p->rounds <= 4 && p->lm_iters >= 1 &&
         p->lm_iters <= 50 && p->thresh > 0.0 && p->thresh <= 1.7976931348623157e308;
}

struct RefineArgs {
  const int32_t* nmatch;
  const double *R_in, *t_in;
  const uint8_t* mask_in;
  const int32_t* status_in;
  const double* T;
  double *R_out, *t_out, *rows_out, *cost_out;
  uint8_t* mask_out;
  int32_t* info_out;
  RefineWs w;
  int cap, rounds, lm_iters;
};

// the normalisation of pose_norm_kernel into the refinement's workspace (no scan state to start)
__global__ void pose_refine_norm_kernel(const PoseArgs a) {
  const int b = blockIdx.y;
  const int n = min(a.nmatch[b], a.p.cap);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  if (a.p.k_f64)
    norm_pair<double>(a, b, t);
  else
    norm_pair<float>(a, b, t);
}

struct PoseRefineLds {
  double red[4][RF_SUMS];
  double tot[RF_SUMS];
  double cur[RF_SUMS];  // the sums at the accepted pose
  double M[5][6];       // the damped system [A + lambda diag(A) | J^T r]
  double fac[5];
  double m[12];         // the accepted pose: R row-major, t
  double mn[12];        // the trial pose
  double EG[6][9];      // E = [t]x R of the pose last linearised and its five directions
  int cnt[4];
};

__device__ __forceinline__ int tri5(int j, int k) { return j * 5 - j * (j - 1) / 2 + (k - j); }  // packed upper triangle, j <= k

// [v]x M
__device__ __forceinline__ void skew_mul(const double* v, const double* M, double* out) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    out[j] = v[1] * M[6 + j] - v[2] * M[3 + j];
    out[3 + j] = v[2] * M[j] - v[0] * M[6 + j];
    out[6 + j] = v[0] * M[3 + j] - v[1] * M[j];
  }
}

// the tangent plane of the unit sphere at t: k = the smallest |t_i| (the first on ties), b1 = e_k x t normalised, b2 = t x b1
__device__ __forceinline__ void tangent_basis(const double* t, double* b1, double* b2) {
  const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
  int k = 0;
  double am = a0;
  if (a1 < am) {
    k = 1;
    am = a1;
  }
  if (a2 < am) k = 2;
  double c0 = 0.0, c1 = -t[2], c2 = t[1];
  if (k == 1) {
    c0 = t[2];
    c1 = 0.0;
    c2 = -t[0];
  } else if (k == 2) {
    c0 = -t[1];
    c1 = t[0];
    c2 = 0.0;
  }
  const double nn = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  b1[0] = c0 / nn;
  b1[1] = c1 / nn;
  b1[2] = c2 / nn;
  b2[0] = t[1] * b1[2] - t[2] * b1[1];
  b2[1] = t[2] * b1[0] - t[0] * b1[2];
  b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// E and the five directions of E at the pose m into EG, matrix k by thread k < 6: E = [t]x R, then [t]x [e_k]x R for the
// rotation, then [b1]x R and [b2]x R.  Every matrix is [v]x N with v of (t, b1, b2) and N of (R, [e_k]x R).
__device__ __forceinline__ void refine_linearise(const double* m, double (*EG)[9], int k) {
  double R[9], t[3], b1[3], b2[3], N[9], v[3], out[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) R[e] = m[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) t[e] = m[9 + e];
  const double ek[3] = {k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, k == 3 ? 1.0 : 0.0};
  skew_mul(ek, R, N);
  tangent_basis(t, b1, b2);
#pragma unroll
  for (int e = 0; e < 9; ++e) N[e] = (k >= 1 && k <= 3) ? N[e] : R[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) v[e] = k == 4 ? b1[e] : k == 5 ? b2[e] : t[e];
  skew_mul(v, N, out);
#pragma unroll
  for (int e = 0; e < 9; ++e) EG[k][e] = out[e];
}

// the trial pose of the step d from m into mn (one thread): abs_pose.hip::apply_step's closed form of exp([w]x) for the rotation,
// t + d[3] b1 + d[4] b2 renormalised for the translation
__device__ __forceinline__ void refine_step(const double* m, const double* d, double* mn) {
  const double th = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  double A = 1.0, Bc = 0.5;
  if (th > 0.0) {
    A = sin(th) / th;
    const double h = sin(0.5 * th) / th;
    Bc = 2.0 * h * h;
  }
  const double W[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
  double X[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double w2 = (W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j]) + W[3 * i + 2] * W[6 + j];
      X[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * W[3 * i + j]) + Bc * w2;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) mn[3 * i + j] = (X[3 * i] * m[j] + X[3 * i + 1] * m[3 + j]) + X[3 * i + 2] * m[6 + j];
  double t[3], b1[3], b2[3], tn[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) t[e] = m[9 + e];
  tangent_basis(t, b1, b2);
#pragma unroll
  for (int e = 0; e < 3; ++e) tn[e] = (t[e] + d[3] * b1[e]) + d[4] * b2[e];
  const double nn = sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2]);
#pragma unroll
  for (int e = 0; e < 3; ++e) mn[9 + e] = tn[e] / nn;
}

// the Sampson inliers of E among the n matches (pose_score_kernel's compare): their count, uniform across the workgroup; with
// flags, each thread records its matches tid, tid + 256, ...
__device__ int refine_count(PoseRefineLds& L, const double* E, const double4* xn, int n, float thr2, uint8_t* flags) {
  const int tid = threadIdx.x;
  int c = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + tid;
    const bool in = j < n && sampson(E, xn[j < n ? j : 0]) <= thr2;  // a NaN error is never an inlier
    if (flags && j < n) flags[j] = in;
    c += __popcll(__ballot(in));
  }
  __syncthreads();
  if ((tid & 63) == 0) L.cnt[tid >> 6] = c;
  __syncthreads();
  return L.cnt[0] + L.cnt[1] + L.cnt[2] + L.cnt[3];
}

// J^T J (packed upper), J^T r and |r|^2 of r = d / sqrt(s) over the flagged matches at the pose linearised in L.EG, into L.tot:
// per thread over its matches, a butterfly inside each wave, then the waves in order (a fixed order)
__device__ void refine_pass(PoseRefineLds& L, const double4* xn, const uint8_t* flags, int n) {
  const int tid = threadIdx.x, wv = tid >> 6;
  double acc[RF_SUMS];
#pragma unroll
  for (int e = 0; e < RF_SUMS; ++e) acc[e] = 0.0;
  for (int j = tid; j < n; j += 256) {
    if (!flags[j]) continue;
    const double4 pt = xn[j];
    const double x1 = pt.x, y1 = pt.y, x2 = pt.z, y2 = pt.w;
    // E and the directions are read from LDS per match: hoisted out of the loop, the 54 loop-invariant doubles take 108 VGPRs
    // and the kernel 220 bytes of scratch (as in polish above)
    __asm__ volatile("" ::: "memory");
    const double* E = L.EG[0];
    const double a = E[0] * x1 + E[1] * y1 + E[2];
    const double b = E[3] * x1 + E[4] * y1 + E[5];
    const double c = E[6] * x1 + E[7] * y1 + E[8];
    const double p = E[0] * x2 + E[3] * y2 + E[6];
    const double q = E[1] * x2 + E[4] * y2 + E[7];
    const double d = x2 * a + y2 * b + c;
    const double s = a * a + b * b + p * p + q * q;
    const double rs = sqrt(s);
    const double r = d / rs;
    double J[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double* G = L.EG[1 + k];
      const double da = G[0] * x1 + G[1] * y1 + G[2];
      const double db = G[3] * x1 + G[4] * y1 + G[5];
      const double dc = G[6] * x1 + G[7] * y1 + G[8];
      const double dp = G[0] * x2 + G[3] * y2 + G[6];
      const double dq = G[1] * x2 + G[4] * y2 + G[7];
      const double dd = x2 * da + y2 * db + dc;
      const double ds = 2.0 * (a * da + b * db + p * dp + q * dq);
      J[k] = dd / rs - d * ds / (2.0 * s * rs);
    }
    int e = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int k = i; k < 5; ++k, ++e) acc[e] += J[i] * J[k];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[15 + i] += J[i] * r;
    acc[20] += r * r;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < RF_SUMS; ++k) {
    double x = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if ((tid & 63) == 0) L.red[wv][k] = x;
  }
  __syncthreads();
  if (tid < RF_SUMS) L.tot[tid] = ((L.red[0][tid] + L.red[1][tid]) + L.red[2][tid]) + L.red[3][tid];
  __syncthreads();
}

__global__ __launch_bounds__(256) void pose_refine_kernel(const RefineArgs a) {
  __shared__ PoseRefineLds L;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(a.nmatch[b], a.cap);
  const size_t cap = a.cap;
  uint8_t* mout = a.mask_out + b * cap;
  const uint8_t* min_ = a.mask_in + b * cap;
  uint8_t* inl = a.w.inl + b * cap;
  const double4* xn = a.w.xn + b * cap;
  double* Ro = a.R_out + (size_t)b * 9;
  double* to = a.t_out + (size_t)b * 3;
  double* rows = a.rows_out ? a.rows_out + (size_t)b * 4 : nullptr;
  double* cost = a.cost_out ? a.cost_out + (size_t)b * 2 : nullptr;
  int32_t* info = a.info_out + (size_t)b * 4;
  const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
  if (a.status_in[b] < 0) {  // no pose to refine (uniform across the workgroup)
    for (size_t j = tid; j < cap; j += 256) mout[j] = 0;
    if (tid != 0) return;
    for (int i = 0; i < 9; ++i) Ro[i] = 0.0;
    for (int i = 0; i < 3; ++i) to[i] = 0.0;
    if (rows) {
      rows[0] = rows[1] = rows[2] = inf;
      rows[3] = 0.0;
    }
    info[0] = -1;
    info[1] = info[2] = info[3] = 0;
    if (cost) cost[0] = cost[1] = nan;
    return;
  }
  if (tid < 9)
    L.m[tid] = a.R_in[(size_t)b * 9 + tid];
  else if (tid < 12)
    L.m[tid] = a.t_in[(size_t)b * 3 + (tid - 9)];
  __syncthreads();
  if (tid < 6) refine_linearise(L.m, L.EG, tid);
  __syncthreads();
  const float thr2 = n > 0 ? a.w.thr2[b] : 0.0f;
  const int c_in = refine_count(L, L.EG[0], xn, n, thr2, nullptr);
  int accepted = 0, ran = 0, last = 0;
  double cost0 = nan, cost1 = nan;
  for (int round = 0; round < a.rounds; ++round) {
    // L.EG is linearised at L.m here
    const int cs = refine_count(L, L.EG[0], xn, n, thr2, inl);
    if (cs < RF_MIN_SET) break;
    refine_pass(L, xn, inl, n);
    if (tid < RF_SUMS) L.cur[tid] = L.tot[tid];
    __syncthreads();
    ++ran;
    last = cs;
    cost0 = L.cur[20] / (double)cs;
    double lambda = 1e-3;
    for (int iter = 0; iter < a.lm_iters; ++iter) {
      if (tid < 30) {
        const int r = tid / 6, k = tid % 6;
        L.M[r][k] = k == 5 ? L.cur[15 + r] : L.cur[r <= k ? tri5(r, k) : tri5(k, r)] + (r == k ? lambda * L.cur[tri5(r, r)] : 0.0);
      }
      __syncthreads();
      if (!gauss_jordan<5, 6>(L.M, L.fac, 0.0)) break;
      double d[5], dmax = 0.0;
      bool fin = true;
#pragma unroll
      for (int e = 0; e < 5; ++e) {
        d[e] = -L.M[e][5];
        fin &= isfinite(d[e]);
        dmax = fmax(dmax, fabs(d[e]));
      }
      if (!fin) break;
      if (tid == 0) refine_step(L.m, d, L.mn);
      __syncthreads();
      if (tid < 6) refine_linearise(L.mn, L.EG, tid);
      __syncthreads();
      refine_pass(L, xn, inl, n);
      const double S = L.cur[20], Sd = L.tot[20];
      __syncthreads();
      if (Sd < S) {  // a non-finite trial cost is a rejection
        if (tid < 12) L.m[tid] = L.mn[tid];
        if (tid < RF_SUMS) L.cur[tid] = L.tot[tid];
        lambda = lambda / 10.0;
        ++accepted;
      } else {
        lambda = lambda * 10.0;
      }
      __syncthreads();
      if (dmax < FLT_EPS) break;
    }
    __syncthreads();
    if (tid < 6) refine_linearise(L.m, L.EG, tid);  // the last trial may have been rejected
    __syncthreads();
    cost1 = L.cur[20] / (double)cs;
  }
  const int c_ref = refine_count(L, L.EG[0], xn, n, thr2, inl);
  const bool kept = accepted > 0 && c_ref >= c_in;
  int nmask = 0;
  for (size_t j0 = 0; j0 < cap; j0 += 256) {
    const size_t j = j0 + tid;
    bool in = false;
    if (j < cap) {
      if (kept)
        in = j < (size_t)n && inl[j] && cheiral(L.m, L.m + 9, xn[j]);
      else
        in = min_[j] != 0;
      mout[j] = kept ? (uint8_t)in : min_[j];
    }
    nmask += __popcll(__ballot(in && j < (size_t)n));
  }
  __syncthreads();
  if ((tid & 63) == 0) L.cnt[tid >> 6] = nmask;
  __syncthreads();
  if (tid != 0) return;
  nmask = L.cnt[0] + L.cnt[1] + L.cnt[2] + L.cnt[3];
  const double* Rk = kept ? L.m : a.R_in + (size_t)b * 9;
  const double* tk = kept ? L.m + 9 : a.t_in + (size_t)b * 3;
  for (int i = 0; i < 9; ++i) Ro[i] = Rk[i];
  for (int i = 0; i < 3; ++i) to[i] = tk[i];
  info[0] = kept ? 1 : 0;
  info[1] = ran;
  info[2] = accepted;
  info[3] = last;
  if (cost) {
    cost[0] = cost0;
    cost[1] = cost1;
  }
  if (!rows) return;
  rows[3] = (double)nmask / (double)n;  // mask.mean()
  if (!a.T) {
    rows[0] = rows[1] = rows[2] = nan;
    return;
  }
  pose_error_rows(Rk, tk, a.T + (size_t)b * 16, rows);
}

}  // namespace

EINX_EXPORT size_t einx_relative_pose_ws_bytes(const einx_pose_params* p) {
  if (!p || p->struct_size != sizeof(einx_pose_params) || p->B <= 0 || p->cap <= 0 || p->max_iters <= 0) return 0;
  size_t bytes = 0;
  carve(p, nullptr, &bytes);
  return bytes;
}

EINX_EXPORT int einx_relative_pose(const einx_pose_params* p, const float* mk0, const float* mk1, const int32_t* nmatch, const void* K0,
                                   const void* K1, const double* T_0to1, void* ws, double* R_out, double* t_out, uint8_t* mask_out,
                                   int32_t* status, double* rows_out, void* stream) {
  EINX_CHECK_ARG(p && p->struct_size == sizeof(einx_pose_params), "einx_pose_params.struct_size mismatch");
  EINX_CHECK_ARG(mk0 && mk1 && nmatch && K0 && K1 && ws && R_out && t_out && mask_out && status, "null pointer");
  EINX_CHECK_ARG(p->B > 0 && p->cap > 0 && (p->cols == 2 || p->cols == 3), "bad shape");
  EINX_CHECK_ARG(p->max_iters > 0 && p->max_iters <= 65535, "max_iters out of range");
  EINX_CHECK_ARG(p->k_f64 == 0 || p->k_f64 == 1, "k_f64 is 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  PoseArgs a;
  a.mk0 = mk0;
  a.mk1 = mk1;
  a.nmatch = nmatch;
  a.K0 = K0;
  a.K1 = K1;
  a.T = T_0to1;
  a.R_out = R_out;
  a.t_out = t_out;
  a.rows_out = rows_out;
  a.mask_out = mask_out;
  a.status = status;
  a.p = *p;
  a.w = carve(p, ws);
  const unsigned B = (unsigned)p->B;
  hipLaunchKernelGGL(pose_norm_kernel, dim3((unsigned)einx_cdiv(p->cap, 256), B), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  // a failed launch ends the rounds and stays pending for the check below
  ransac_rounds(p->max_iters, [&](int it0, int it1) {
    hipLaunchKernelGGL(pose_solve_kernel, dim3((unsigned)(it1 - it0), B), dim3(64), 0, s, a, it0);
    if (hipPeekAtLastError() != hipSuccess) return false;
    hipLaunchKernelGGL(pose_score_kernel, dim3((unsigned)(it1 - it0), B), dim3(256), 0, s, a, it0);
    if (hipPeekAtLastError() != hipSuccess) return false;
    hipLaunchKernelGGL((ransac_select_kernel<5, 16, PoseModels>), dim3((unsigned)einx_cdiv(p->B, 64)), dim3(64), 0, s, a.w.scan, nmatch,
                       p->B, p->cap, p->max_iters, p->conf, it0, it1, PoseModels{a.w.nsol, a.w.cnt});
    return hipPeekAtLastError() == hipSuccess;
  });
  EINX_CHECK_LAUNCH();
  hipLaunchKernelGGL(pose_recover_kernel, dim3(B), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT int einx_essential_5pt(const double* x1, const double* x2, int n_problems, double* E_out, int32_t* n_solutions, void* stream) {
  EINX_CHECK_ARG(x1 && x2 && E_out && n_solutions, "null pointer");
  EINX_CHECK_ARG(n_problems > 0, "n_problems > 0");
  hipLaunchKernelGGL(essential_5pt_kernel, dim3((unsigned)n_problems), dim3(64), 0, (hipStream_t)stream, x1, x2, E_out, n_solutions);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}

EINX_EXPORT size_t einx_relative_pose_refine_ws_bytes(const einx_pose_refine_params* p) {
  if (!refine_params_ok(p)) return 0;
  size_t bytes = 0;
  carve(p, nullptr, &bytes);
  return bytes;
}

EINX_EXPORT int einx_relative_pose_refine(const einx_pose_refine_params* p, const float* mk0, const float* mk1, const int32_t* nmatch,
                                          const void* K0, const void* K1, const double* R_in, const double* t_in, const uint8_t* mask_in,
                                          const int32_t* status_in, const double* T_0to1, void* ws, double* R_out, double* t_out,
                                          uint8_t* mask_out, double* rows_out, int32_t* info_out, double* cost_out, void* stream) {
  EINX_CHECK_ARG(p && p->struct_size == sizeof(einx_pose_refine_params), "einx_pose_refine_params.struct_size mismatch");
  EINX_CHECK_ARG(mk0 && mk1 && nmatch && K0 && K1, "null pointer among the matches and intrinsics");
  EINX_CHECK_ARG(R_in && t_in && mask_in && status_in, "null pointer among the input pose (R_in, t_in, mask_in, status_in)");
  EINX_CHECK_ARG(ws && R_out && t_out && mask_out && info_out, "null pointer among ws, R_out, t_out, mask_out, info_out");
  EINX_CHECK_ARG(p->B > 0 && p->cap > 0 && (p->cols == 2 || p->cols == 3), "bad shape");
  EINX_CHECK_ARG(p->kp_yx == 0 || p->kp_yx == 1, "kp_yx is 0 or 1");
  EINX_CHECK_ARG(p->k_f64 == 0 || p->k_f64 == 1, "k_f64 is 0 or 1");
  EINX_CHECK_ARG(p->rounds >= 1 && p->rounds <= 4, "rounds is 1..4");
  EINX_CHECK_ARG(p->lm_iters >= 1 && p->lm_iters <= 50, "lm_iters is 1..50");
  EINX_CHECK_ARG(refine_params_ok(p), "thresh is a positive number of pixels");
  hipStream_t s = (hipStream_t)stream;
  const RefineWs w = carve(p, ws);
  PoseArgs na = {};  // what norm_pair reads: the matches, the intrinsics, the layout, the threshold, where xn and thr2 go
  na.mk0 = mk0;
  na.mk1 = mk1;
  na.nmatch = nmatch;
  na.K0 = K0;
  na.K1 = K1;
  na.w.xn = w.xn;
  na.w.thr2 = w.thr2;
  na.p.B = p->B;
  na.p.cap = p->cap;
  na.p.cols = p->cols;
  na.p.kp_yx = p->kp_yx;
  na.p.k_f64 = p->k_f64;
  na.p.thresh = p->thresh;
  const unsigned B = (unsigned)p->B;
  hipLaunchKernelGGL(pose_refine_norm_kernel, dim3((unsigned)einx_cdiv(p->cap, 256), B), dim3(256), 0, s, na);
  EINX_CHECK_LAUNCH();
  RefineArgs a;
  a.nmatch = nmatch;
  a.R_in = R_in;
  a.t_in = t_in;
  a.mask_in = mask_in;
  a.status_in = status_in;
  a.T = T_0to1;
  a.R_out = R_out;
  a.t_out = t_out;
  a.rows_out = rows_out;
  a.cost_out = cost_out;
  a.mask_out = mask_out;
  a.info_out = info_out;
  a.w = w;
  a.cap = p->cap;
  a.rounds = p->rounds;
  a.lm_iters = p->lm_iters;
  hipLaunchKernelGGL(pose_refine_kernel, dim3(B), dim3(256), 0, s, a);
  EINX_CHECK_LAUNCH();
  return EINX_OK;
}
