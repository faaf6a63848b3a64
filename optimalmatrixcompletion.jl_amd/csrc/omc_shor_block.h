// omc_shor_block.h -- the arithmetic of one order-5 multiplier block Gamma_q of a Shor-mode certificate, as plain
// functions for the device (k_scert_clean / k_scert_minor of omc_shor_cert.hip, one lane per minor, everything in registers) and for a host
// compiler (tests/host/shor_block_check.cpp).  Nothing of HIP is included: a host compiler sees ordinary inline functions.
//
// Packed index of (r, c), r >= c: r (r + 1) / 2 + c -- the lower triangle by rows, which is the upper triangle by columns of include/omc.h.
//   0:(0,0) | 1:(1,0) 2:(1,1) | 3:(2,0) 4:(2,1) 5:(2,2) | 6:(3,0) 7:(3,1) 8:(3,2) 9:(3,3) | 10:(4,0) 11:(4,1) 12:(4,2) 13:(4,3) 14:(4,4)
// Rows: 0 = the constant 1, 1 = (i1,j1), 2 = (i1,j2), 3 = (i2,j1), 4 = (i2,j2).  The entries that multiply lifted variables: 4 and 13
// (V1 of rows i1, i2), 7 and 12 (V2 of columns j1, j2), 11 and 8 (V3, the same variable twice).
#ifndef OMC_SHOR_BLOCK_H
#define OMC_SHOR_BLOCK_H
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OMC_SB_FN __host__ __device__ inline
#define OMC_SB_UNROLL _Pragma("unroll")
#else
#define OMC_SB_FN inline
#define OMC_SB_UNROLL
#endif

struct ShorBlockEig { double w[5]; double v[5][5]; };      // eigenvalues (unsorted) and eigenvectors (column i of v belongs to w[i])

// Cyclic Jacobi on a symmetric order-5 matrix given by its packed triangle.  Every index is a compile-time constant after unrolling, so the
// working copy stays in registers on the device.  Backward stable: the computed pairs are exact for a matrix within a few eps ||g||_F of g.
template <bool VECTORS>
OMC_SB_FN void shor_block_jacobi(const double* g, ShorBlockEig& E) {
  double a[5][5];
OMC_SB_UNROLL
  for (int r = 0; r < 5; ++r)
OMC_SB_UNROLL
    for (int c = 0; c < 5; ++c) {
      a[r][c] = g[(r >= c) ? (r * (r + 1) / 2 + c) : (c * (c + 1) / 2 + r)];
      if (VECTORS) E.v[r][c] = (r == c) ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0.0, dg = 0.0;
OMC_SB_UNROLL
    for (int r = 0; r < 5; ++r) {
      dg += a[r][r] * a[r][r];
OMC_SB_UNROLL
      for (int c = 0; c < r; ++c) off += a[r][c] * a[r][c];
    }
    if (!(off > 1e-34 * dg)) break;      // converged, zero, or not finite
OMC_SB_UNROLL
    for (int p = 0; p < 4; ++p)
OMC_SB_UNROLL
      for (int q = p + 1; q < 5; ++q) {
        const double apq = a[p][q];
        if (fabs(apq) > 1e-300) {
          const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
          const double at = fabs(theta);
          double t = 1.0 / (at + sqrt(at * at + 1.0));
          t = (theta >= 0.0) ? t : -t;
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          a[p][p] -= t * apq; a[q][q] += t * apq; a[p][q] = 0.0; a[q][p] = 0.0;
OMC_SB_UNROLL
          for (int k = 0; k < 5; ++k) {
            if (k != p && k != q) {
              const double akp = a[k][p], akq = a[k][q];
              const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
              a[k][p] = np_; a[p][k] = np_; a[k][q] = nq_; a[q][k] = nq_;
            }
            if (VECTORS) {
              const double vkp = E.v[k][p], vkq = E.v[k][q];
              E.v[k][p] = c * vkp - s * vkq; E.v[k][q] = s * vkp + c * vkq;
            }
          }
        }
      }
  }
OMC_SB_UNROLL
  for (int i = 0; i < 5; ++i) E.w[i] = a[i][i];
}

// the smallest eigenvalue of the packed block
OMC_SB_FN double shor_block_min_eig(const double* g) {
  ShorBlockEig E;
  shor_block_jacobi<false>(g, E);
  double lo = E.w[0];
OMC_SB_UNROLL
  for (int i = 1; i < 5; ++i) lo = (E.w[i] < lo) ? E.w[i] : lo;
  return lo;
}

// g <- g - V min(w, 0) V': the PSD part taken as "the block minus its negative part", so that a block that is PSD up to rounding keeps its
// entries up to that rounding.  Returns the smallest eigenvalue of the block as given.
OMC_SB_FN double shor_block_remove_negative(double* g) {
  ShorBlockEig E;
  shor_block_jacobi<true>(g, E);
  double lo = E.w[0];
OMC_SB_UNROLL
  for (int i = 1; i < 5; ++i) lo = (E.w[i] < lo) ? E.w[i] : lo;
OMC_SB_UNROLL
  for (int r = 0; r < 5; ++r)
OMC_SB_UNROLL
    for (int c = 0; c <= r; ++c) {
      double acc = 0.0;
OMC_SB_UNROLL
      for (int i = 0; i < 5; ++i) acc += ((E.w[i] < 0.0) ? E.w[i] : 0.0) * E.v[r][i] * E.v[c][i];
      g[r * (r + 1) / 2 + c] -= acc;
    }
  return lo;
}

// the half-sum of the two copies of V3: what fails to cancel inside the block
OMC_SB_FN double shor_block_e3(const double* g) { return 0.5 * (g[11] + g[8]); }

// g <- g - E + ||E||_F I, E the symmetric correction with e12 at (1,2), e34 at (3,4), e13 at (1,3), e24 at (2,4) and e3 at (1,4) and (2,3).
// Returns ||E||_F.
OMC_SB_FN double shor_block_spread(double* g, double e12, double e34, double e13, double e24, double e3) {
  const double shift = sqrt(2.0 * (e12 * e12 + e34 * e34 + e13 * e13 + e24 * e24 + 2.0 * e3 * e3));
  g[4] -= e12; g[13] -= e34; g[7] -= e13; g[12] -= e24; g[11] -= e3; g[8] -= e3;
  g[0] += shift; g[2] += shift; g[5] += shift; g[9] += shift; g[14] += shift;
  return shift;
}

// g <- g + max(0, -lambda_min(g)) I: whatever came in, the block that enters the bound is PSD; a multiple of the identity leaves the V
// entries alone.  Returns the shift (0 for a block that was PSD up to 0.118 ||E||_F before the spread).
OMC_SB_FN double shor_block_final_shift(double* g) {
  const double lo = shor_block_min_eig(g);
  const double sh = (lo < 0.0) ? -lo : 0.0;      // NaN gives 0: the caller tests the entries for finiteness
  g[0] += sh; g[2] += sh; g[5] += sh; g[9] += sh; g[14] += sh;
  return sh;
}

OMC_SB_FN bool shor_block_finite(const double* g) {
  double s = 0.0;
OMC_SB_UNROLL
  for (int e = 0; e < 15; ++e) s += g[e] * 0.0;      // 0 for finite entries, NaN otherwise
  return s == 0.0;
}
#endif
