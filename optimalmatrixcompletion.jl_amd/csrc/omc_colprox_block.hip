// omc_colprox_block.hip -- the column prox (block F of DESIGN.md section 3.1, both modes of k_colprox) for DENSE columns: one 256-thread
// workgroup per (slot, column) and a blocked Cholesky factorization on 16 x 16 tiles whose panel solves and trailing updates are
// v_mfma_f64_16x16x4_f64 products.  k_colprox_pair / k_colprox_wide (omc_colprox.hip) stop at 64 observed rows; beyond,
// the one-wave colprox_body of omc_device.hip redoes a scalar wave Cholesky for every step of a Newton iteration out of a global slab.
//   storage    blocked lower triangle, CpBlockLayout (omc_layout.h): in dynamic LDS up to 176 rows (k_colprox_block<true>), above in a
//              per-(slot, column) global slab with the current panel staged in LDS (k_colprox_block<false>); one body, two pointer types
//   factor     right-looking: the diagonal tile on wave 0 (rows in registers, pivots by v_readlane), which also leaves the INVERSE of its
//              factor in the tile; panel  L(I,K) = A(I,K) inv(L(K,K))'  and trailing update  A(I,J) -= L(I,K) L(J,K)'  as MFMA products over
//              the four waves.  A last tile that the column does not fill is padded with the identity.
//   solves     blocked forward and back substitution on the same tiles (the diagonal tiles hold inverses: products only)
//   secular    the iteration of colprox_reg: Halley steps from the stored s inside [lo, hi], a failed factorization moves right, stop at
//              |ds| <= 1e-13 max(1, |s|), second-order Taylor finish under the same acceptance rule
// Every reduction has a fixed order and nothing is accumulated atomically: the result of a (slot, column) does not depend on the slot, the
// batch or the neighbours.  The reference has no counterpart (Mosek solves the node's conic program, OMC.jl:1482-1500, 1857); oracle:
// _prox_columns (oracle/omc_oracle.py:475-515).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "omc_device.h"
#include "omc_wave.h"

typedef double double4b __attribute__((ext_vector_type(4)));

// index of the tile row ii of the e-th tile of a lower triangle numbered row by row (e = ii (ii + 1) / 2 + jj, jj <= ii)
__device__ __forceinline__ int cpb_row_of(int e) {
  int ii = (int)((__builtin_sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  while (((ii * (ii + 1)) >> 1) > e) --ii;
  while ((((ii + 1) * (ii + 2)) >> 1) <= e) ++ii;
  return ii;
}

// T: the tiles (LDS or global slab), sm: the dynamic LDS block (tiles first in the LDS variant, panel first in the slab variant)
template <bool LDS, class PT>
__device__ __forceinline__ void colprox_block_body(const OmcWS& w, const int mode, const int b, const int j, const int off, const int c, PT T,
                                                   double* sm, double* s_inv, double* s_d, double* s_red, int* s_ok) {
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int n = w.n;
  const CpBlockLayout L = cp_block_layout(c, LDS ? 1 : 0);
  const int nb = L.nb, cp16 = nb * 16;
  double* pan = sm + L.panel;      // slab variant: tiles (K+1 .. nb-1, K) of the current panel
  double *va = sm + L.va, *vy = sm + L.vy, *vz = sm + L.vz, *vw = sm + L.vw, *vo = sm + L.vo;
  int* sidx = (int*)(sm + L.sidx);
  const double gm = w.gamma;
  const double* Y = w.Y + (size_t)b * n * n;
  const double* Yp = w.Yp + (size_t)b * n * n;
  const double* Yx = w.Yx ? w.Yx + (size_t)b * n * n : nullptr;
  double* alpha = ((mode == 0) ? w.alpha : w.alphaX) + (size_t)b * w.nnz + off;
  for (int p = tid; p < cp16; p += 256) {      // the padding beyond c: zero entries, row index 0 (col_idx is never read beyond c)
    const bool in = p < c;
    va[p] = in ? w.col_val[off + p] : 0.0;
    vo[p] = (in && mode == 0) ? alpha[p] : 0.0;
    sidx[p] = in ? w.col_idx[off + p] : 0;
  }
  __syncthreads();
  const double rho_f = w.rho_b[b] * w.rho_f_ratio;
  const double coef = (mode == 0) ? gm / (2.0 * rho_f) : 0.0;

  // ---- B + shift I into the tiles: thread (r, q) of every tile, four tiles per trip with the loads issued before the first use -----------
  auto gather = [&](const double shift) {
    const int r = tid & 15, q = tid >> 4;
    int I = 0, J = 0;
    for (int t0 = 0; t0 < L.ntiles; t0 += 4) {
      double y1[4], y2[4]; int pp[4], qq[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        pp[u] = 16 * I + r; qq[u] = 16 * J + q;      // beyond the last tile the indices stay inside the padded vectors (I <= nb - 1 is kept below)
        const size_t a = (size_t)sidx[qq[u]] * n + sidx[pp[u]];
        y1[u] = (mode == 0 && Yx) ? Yx[a] : Y[a];
        y2[u] = (mode == 0 && !Yx) ? Yp[a] : 0.0;
        if (t0 + u + 1 < L.ntiles) { if (++J > I) { ++I; J = 0; } }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (t0 + u < L.ntiles) {
          const int p = pp[u], q2 = qq[u];
          const double yv = (mode == 0 && !Yx) ? (2.0 * y1[u] - y2[u]) : y1[u];
          double v = gm * (yv - coef * vo[p] * vo[q2]);
          if (p == q2) v += 1.0 + shift;
          if (p >= c || q2 >= c) v = (p == q2) ? 1.0 : 0.0;      // identity padding of the last tile row / column
          T[(size_t)(t0 + u) * CPB_TILE + q * 16 + r] = v;
        }
      }
    }
    __syncthreads();
  };

  // ---- blocked Cholesky, right-looking.  On exit tile (I, K), I > K, holds L(I, K) and tile (K, K) holds inv(L(K, K)) (lower triangular, zeros
  // above).  Returns false (for every thread) as soon as a pivot is not positive ----------------------------------------------------------------
  auto factor = [&]() -> bool {
    for (int K = 0; K < nb; ++K) {
      PT D = T + (size_t)cpb_tile(K, K) * CPB_TILE;
      if (wv == 0) {
        // lane r (every group of 16 lanes does the same work; lanes 0..15 are read) holds row r of the tile's lower triangle
        double P[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) { const double x = D[q * 16 + li]; P[q] = (q <= li) ? x : 0.0; }
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const double piv = readlane_d(P[q], q);
          ok = ok && (piv > 1e-290);
          const double dq = 1.0 / sqrt(ok ? piv : 1.0);
          const double lr = P[q] * dq;      // L(r, q) for r >= q (zero above the diagonal)
          P[q] = (li == q) ? dq : lr;        // the diagonal keeps 1 / L(q, q): all the inversion below needs of it
#pragma unroll
          for (int q2 = q + 1; q2 < 16; ++q2) {
            const double lq = readlane_d(lr, q2);
            P[q2] = (li >= q2) ? fma(-lr, lq, P[q2]) : P[q2];
          }
        }
        if (lane < 16) {
#pragma unroll
          for (int q = 0; q < 16; ++q) s_d[q * 16 + lane] = P[q];
        }
        WAVE_SYNC();
        // lane jc < 16: column jc of inv(L), by forward substitution with broadcast reads of L (s_d: L below the diagonal, 1 / L(q, q) on it)
        double x[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          double acc = (r == li) ? 1.0 : 0.0;
#pragma unroll
          for (int t = 0; t < r; ++t) acc = fma(-s_d[t * 16 + r], x[t], acc);
          x[r] = acc * s_d[r * 16 + r];
        }
        if (lane < 16) {
#pragma unroll
          for (int r = 0; r < 16; ++r) { s_inv[lane * 16 + r] = x[r]; D[lane * 16 + r] = x[r]; }
        }
        if (lane == 0) *s_ok = ok ? 1 : 0;
      }
      __syncthreads();
      if (!*s_ok) return false;
      // panel: L(I, K) = A(I, K) inv(L(K, K))', computed as its transpose  D[j][i] = sum_t inv[j][t] A[i][t]  so that the stores are contiguous
      for (int I = K + 1 + wv; I < nb; I += 4) {
        PT A = T + (size_t)cpb_tile(I, K) * CPB_TILE;
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { av[u] = s_inv[(4 * u + lk) * 16 + li]; bv[u] = A[(4 * u + lk) * 16 + li]; }
        double4b acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          A[(lk + 4 * r) * 16 + li] = acc[r];
          if constexpr (!LDS) pan[(size_t)(I - K - 1) * CPB_TILE + (lk + 4 * r) * 16 + li] = acc[r];
        }
      }
      __syncthreads();
      // trailing update: A(I, J) -= L(I, K) L(J, K)' for K < J <= I, again as the transpose (the f64 MFMA returns row lk + 4 r, column li)
      const int t = nb - K - 1, ntr = (t * (t + 1)) >> 1;
      for (int e = wv; e < ntr; e += 4) {
        const int ii = cpb_row_of(e), jj = e - ((ii * (ii + 1)) >> 1);
        const int I = K + 1 + ii, J = K + 1 + jj;
        PT Cm = T + (size_t)cpb_tile(I, J) * CPB_TILE;
        double av[4], bv[4];
        if constexpr (LDS) {
          PT PI = T + (size_t)cpb_tile(I, K) * CPB_TILE; PT PJ = T + (size_t)cpb_tile(J, K) * CPB_TILE;
#pragma unroll
          for (int u = 0; u < 4; ++u) { av[u] = PJ[(4 * u + lk) * 16 + li]; bv[u] = PI[(4 * u + lk) * 16 + li]; }
        } else {
          const double* PI = pan + (size_t)ii * CPB_TILE; const double* PJ = pan + (size_t)jj * CPB_TILE;
#pragma unroll
          for (int u = 0; u < 4; ++u) { av[u] = PJ[(4 * u + lk) * 16 + li]; bv[u] = PI[(4 * u + lk) * 16 + li]; }
        }
        double4b acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = Cm[(lk + 4 * r) * 16 + li];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[u], bv[u], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Cm[(lk + 4 * r) * 16 + li] = acc[r];
      }
      __syncthreads();
    }
    return true;
  };

  // ---- x <- (L L')^-1 x, x a padded vector in LDS: blocked forward, then back substitution -------------------------------------------------
  auto solve = [&](double* x) {
    for (int K = 0; K < nb; ++K) {
      PT D = T + (size_t)cpb_tile(K, K) * CPB_TILE;
      if (wv == 0) {      // x_K <- inv(L(K,K)) x_K: lane (row li, quarter lk of the 16 terms)
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) s = fma(D[(4 * lk + u) * 16 + li], x[16 * K + 4 * lk + u], s);
        s += __shfl_xor(s, 16, WAVE);
        s += __shfl_xor(s, 32, WAVE);
        WAVE_SYNC();
        if (lane < 16) x[16 * K + lane] = s;
      }
      __syncthreads();
      for (int I = K + 1 + (tid >> 4); I < nb; I += 16) {      // x_I -= L(I, K) x_K: thread = row (tid & 15) of tile I
        PT A = T + (size_t)cpb_tile(I, K) * CPB_TILE;
        const int r = tid & 15;
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 16; ++t) s = fma(A[t * 16 + r], x[16 * K + t], s);
        x[16 * I + r] -= s;
      }
      __syncthreads();
    }
    for (int K = nb - 1; K >= 0; --K) {
      PT D = T + (size_t)cpb_tile(K, K) * CPB_TILE;
      if (wv == 0) {      // x_K <- inv(L(K,K))' x_K
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) s = fma(D[li * 16 + 4 * lk + u], x[16 * K + 4 * lk + u], s);
        s += __shfl_xor(s, 16, WAVE);
        s += __shfl_xor(s, 32, WAVE);
        WAVE_SYNC();
        if (lane < 16) x[16 * K + lane] = s;
      }
      __syncthreads();
      for (int J = (tid >> 4); J < K; J += 16) {      // x_J -= L(K, J)' x_K: thread = column q of tile J, rows taken in the rotated order (r + q) mod 16 (no LDS bank conflicts)
        PT A = T + (size_t)cpb_tile(K, J) * CPB_TILE;
        const int q = tid & 15;
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 16; ++t) { const int r = (t + q) & 15; s = fma(A[q * 16 + r], x[16 * K + r], s); }
        x[16 * J + q] -= s;
      }
      __syncthreads();
    }
  };
  auto copy = [&](double* dst, const double* src) {
    for (int p = tid; p < cp16; p += 256) dst[p] = src[p];
    __syncthreads();
  };
  // (x'x, x'y, y'y) in every thread, summed in a fixed order
  auto dots = [&](const double* x, const double* y, double& xx, double& xy, double& yy) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int p = tid; p < cp16; p += 256) { const double xv = x[p], yv = y[p]; a0 = fma(xv, xv, a0); a1 = fma(xv, yv, a1); a2 = fma(yv, yv, a2); }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if (lane == 0) { s_red[3 * wv] = a0; s_red[3 * wv + 1] = a1; s_red[3 * wv + 2] = a2; }
    __syncthreads();
    xx = (s_red[0] + s_red[3]) + (s_red[6] + s_red[9]);
    xy = (s_red[1] + s_red[4]) + (s_red[7] + s_red[10]);
    yy = (s_red[2] + s_red[5]) + (s_red[8] + s_red[11]);
    __syncthreads();
  };

  if (mode == 0) {
    const double cp = gm * gm / (2.0 * rho_f);
    const double sprev = w.sval[(size_t)b * w.m + j];
    double s = (sprev > 0.0) ? sprev : 0.0;
    double lo = 0.0, hi = -1.0;  // hi < 0: unknown
    bool lo_valid = false;       // the factorization succeeded at lo and phi(lo) >= 0
    bool fin = false;
    int nfact = 0;
    for (int it = 0; it < 60; ++it) {
      ++nfact;
      gather(cp * s);
      if (!factor()) {  // s below the positive definite range: move right
        lo = s; lo_valid = false;
        s = (hi > 0.0) ? 0.5 * (s + hi) : (2.0 * s + 1.0);
        continue;
      }
      copy(vy, va); solve(vy);
      copy(vz, vy); solve(vz);
      double yy, yz, zz;
      dots(vy, vz, yy, yz, zz);
      const double ph = yy - s, dph = -2.0 * cp * yz - 1.0, ddph = 6.0 * cp * cp * zz;
      if (ph >= 0.0) { lo = s; lo_valid = true; } else { hi = s; }
      const double den = 2.0 * dph * dph - ph * ddph;
      double sn = s + ((den > dph * dph) ? (-2.0 * ph * dph / den) : (-ph / dph));
      bool guarded = false;
      if (!(sn > lo) && !lo_valid) { sn = 0.5 * (lo + s); guarded = true; }
      if (sn < lo) { sn = lo; guarded = true; }
      if (hi > 0.0 && sn > hi) { sn = 0.5 * (lo + hi); guarded = true; }
      const double d = sn - s;
      if (fabs(d) <= 1e-13 * fmax(1.0, fabs(s))) { fin = true; break; }      // the current solve is the answer
      if (!guarded && yy > 0.0 && cp * fabs(d) * sqrt(zz / yy) < 1e-5) {       // alpha(s + d) = y - cp d z + cp^2 d^2 w
        copy(vw, vz); solve(vw);
        for (int p = tid; p < cp16; p += 256) vy[p] = vy[p] - cp * d * (vz[p] - cp * d * vw[p]);
        __syncthreads();
        s = sn; fin = true;
        break;
      }
      s = sn;
    }
    if (!fin) {
      ++nfact;
      gather(cp * s);
      factor();
      copy(vy, va); solve(vy);
    }
    double* lamD = w.lamD + ((size_t)b * w.m + j) * n;      // dense copy (zeros off the support) for the output-stationary Lambda Lambda'
    for (int p = tid; p < c; p += 256) { const double v = vy[p]; alpha[p] = v; lamD[sidx[p]] = v; }
    if (tid == 0) { w.sval[(size_t)b * w.m + j] = s; if (w.cp_nfact) w.cp_nfact[(size_t)b * w.m + j] = nfact; }
  } else {
    gather(0.0);
    if (!factor()) {  // Y not PSD enough on this block: report +inf objective contribution; the column's multiplier is 0, not what the slot held before
      for (int p = tid; p < c; p += 256) { alpha[p] = 0.0; if (w.lamDX) w.lamDX[((size_t)b * w.m + j) * n + sidx[p]] = 0.0; }
      if (tid == 0) { w.objcol[(size_t)b * w.m + j] = 1e300; w.c0col[(size_t)b * w.m + j] = 0.0; if (w.cp_nfact) w.cp_nfact[(size_t)b * w.m + j] = 1; }
      return;
    }
    copy(vy, va); solve(vy);
    double aa0, aa, al2;
    dots(va, vy, aa0, aa, al2);
    double* lamX = w.lamDX ? w.lamDX + ((size_t)b * w.m + j) * n : nullptr;
    for (int p = tid; p < c; p += 256) { const double v = vy[p]; alpha[p] = v; if (lamX) lamX[sidx[p]] = v; }
    if (tid == 0) { w.objcol[(size_t)b * w.m + j] = 0.5 * aa; w.c0col[(size_t)b * w.m + j] = aa - 0.5 * al2; if (w.cp_nfact) w.cp_nfact[(size_t)b * w.m + j] = 1; }   // summed in a fixed order by k_check_build
  }
}

// One workgroup per (active slot, list entry).  LDS = true: the columns of w.cp_block (tiles in LDS); false: those of w.cp_slab (tiles in the
// slab).  Two inlined copies of one body so that the LDS copy compiles to ds_read / ds_write instructions, as in k_colprox.
template <bool LDS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_colprox_block(OmcWS w, int mode) {
  extern __shared__ double smem[];
  __shared__ double s_inv[CPB_TILE], s_d[CPB_TILE], s_red[16];
  __shared__ int s_ok;
  const int nlist = LDS ? w.cp_nblock : w.cp_nslab;
  const int* list = LDS ? w.cp_block : w.cp_slab;
  const int id = xcd_block(w.cp_xcd);      // the workgroups of a slot on one XCD: its Yx is gathered from one L2
  const int bl = id / nlist, jj = id - bl * nlist;
  if (bl >= w.nB) return;
  const int b = slot_of(w, bl);
  if (w.done[b]) return;
  const int j = list[jj];
  const int off = w.col_ptr[j], c = w.col_ptr[j + 1] - off;
  if (c <= 0) return;      // never listed
  if constexpr (LDS) colprox_block_body<true>(w, mode, b, j, off, c, smem, smem, s_inv, s_d, s_red, &s_ok);
  else colprox_block_body<false>(w, mode, b, j, off, c, w.cp_bslab + ((size_t)b * w.cp_nslab + jj) * w.geo.cpb_slab_stride, smem, s_inv, s_d, s_red, &s_ok);
}

extern "C" void omc_launch_colprox_block(const OmcWS* w, int mode, hipStream_t s) {
  if (w->cp_nblock > 0) hipLaunchKernelGGL(k_colprox_block<true>, dim3(w->nB * w->cp_nblock), dim3(256), w->geo.cpb_lds_bytes, s, *w, mode);
  if (w->cp_nslab > 0) hipLaunchKernelGGL(k_colprox_block<false>, dim3(w->nB * w->cp_nslab), dim3(256), w->geo.cpb_slab_lds_bytes, s, *w, mode);
}

extern "C" int omc_colprox_block_set_lds(void) {
  const hipError_t e1 = hipFuncSetAttribute((const void*)k_colprox_block<true>, hipFuncAttributeMaxDynamicSharedMemorySize, OMC_MAX_DYN_LDS);
  const hipError_t e2 = hipFuncSetAttribute((const void*)k_colprox_block<false>, hipFuncAttributeMaxDynamicSharedMemorySize, OMC_MAX_DYN_LDS);
  return (e1 != hipSuccess) ? (int)e1 : (int)e2;
}
