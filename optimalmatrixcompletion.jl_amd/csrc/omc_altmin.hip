// omc_altmin.hip -- alternating minimisation (OMC.jl:1979-2279), rank 1, one workgroup per problem.
//
// Both JuMP models of the reference minimise  1/2 sum_Omega ((UV)_ij - A_ij)^2 + 1/(2 gamma) sum_all (UV)_ij^2
// (OMC.jl:2193-2207, 2213-2227).  For k = 1:
//   V-step (model_V, unconstrained): v_j = sum_{i in O_j} u_i A_ij / (sum_{i in O_j} u_i^2 + u'u/gamma)   -- masked LS,
//          one coalesced pass over the CSC copy of (A, indices);
//   U-step (model_U): min 1/2 sum_i h_i u_i^2 - g_i u_i  s.t.  box rows, per-cut bounds lo <= x'u <= hi (OMC.jl:2047-2093),
//          ||u|| <= 1 (OMC.jl:2164-2171);  h_i = sum_{j in O_i} v_j^2 + v'v/gamma, g_i = sum_{j in O_i} A_ij v_j (CSR pass).
//          Solved exactly by duality: multiplier theta of the ball by safeguarded bisection, rows by the same active-set
//          NNQP as the relaxation (Gram matrix C diag(1/(h+theta)) C').
// The whole loop (<= max_iters iterations, convergence rules of OMC.jl:2234-2245 incl. quirk Q3) runs inside one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "omc_device.h"
#include "omc_wave.h"
#include "omc_altmin.h"

__device__ __forceinline__ double am_row_entry(const AltminWS& w, int b, int r, int i) {
  const int kind = w.rkind[(size_t)b * w.Rmax + r];
  const double cf = w.rcoef[(size_t)b * w.Rmax + r];
  if (kind == ROW_BOX) return (w.rbi[(size_t)b * w.Rmax + r] == i) ? cf : 0.0;
  return cf * w.cutx[((size_t)b * w.Lmax + w.rcut[(size_t)b * w.Rmax + r]) * w.n + i];
}

// time_limit of alternating_minimization (OMC.jl:1999-2003, 2186-2189) inside the launch: thread 0 stamps the device's constant-rate clock right
// before the loop and reads it again at the top of every iteration; its verdict goes through LDS, so the whole workgroup leaves together.
// The first iteration runs for any positive limit (the stamp is taken right before its check; `done == 0` makes that unconditional, so U and V
// always hold a completed iteration).
__device__ __forceinline__ long long am_clock_start(const AltminWS& w, int tid) { return (w.tl_ticks && tid == 0) ? (long long)wall_clock64() : 0; }
__device__ __forceinline__ bool am_out_of_time(const AltminWS& w, int tid, long long t_start, int done, int* s_late) {
  if (!w.tl_ticks || done == 0) return false;      // no limit, or nothing completed yet: same for every thread
  if (tid == 0) *s_late = ((long long)wall_clock64() - t_start >= w.tl_ticks) ? 1 : 0;
  __syncthreads();
  return *s_late != 0;                // rewritten only at the top of the next iteration, workgroup barriers later
}

#define AM_MAX_DOUBLINGS 64      // bracket search of the ball multiplier (theta <= 2^64 max|g|: beyond that model_U is infeasible)
#define AM_FEAS_TOL 1e-6         // largest row violation / excess of ||u||^2 - 1 accepted from a U-step (the oracle uses the same)
__device__ __forceinline__ double block_max(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (l == 0) red[wv] = v;
  __syncthreads();
  double s = red[0];
  for (int i = 1; i < nw; ++i) s = fmax(s, red[i]);
  return s;
}

__global__ void __launch_bounds__(256) k_altmin(AltminWS w) {
  extern __shared__ double sm_lds[];
  // problems that do not fit the LDS (config 5: 1000 x 1000) keep the same state in a per-problem global slab (L2 / HBM): same code, flat addresses
  double* sm = w.scratch ? w.scratch + (size_t)blockIdx.x * w.scratch_stride : sm_lds;
  __shared__ double red[32];
  __shared__ double s_Gp[NNQP_GP_DOUBLES];
  __shared__ double s_sv[NNQP_PMAX], s_tmp[NNQP_PMAX];
  __shared__ int s_pl[NNQP_PMAX];
  __shared__ int s_stop, s_ov, s_late;
  const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int n = w.n, m = w.m, R = w.R[b];
  const Altmin1Layout L = altmin1_layout(n, m, w.Rmax);
  double *u = sm, *v = sm + L.v, *h = sm + L.h, *g = sm + L.g;      // n, m, n, n
  double* u0 = sm + L.u0;    // n  unconstrained-in-rows point for the current theta
  double *cvec = sm + L.cvec, *mu = sm + L.mu;      // Rmax each
  double* G = w.G + (size_t)b * w.Rmax * w.Rmax;
  double* objs = w.objectives + (size_t)b * w.max_iters;
  for (int i = tid; i < n; i += T) u[i] = w.U0[(size_t)b * n + i];
  for (int r = tid; r < w.Rmax; r += T) mu[r] = 0.0;
  for (int t = tid; t < w.max_iters; t += T) objs[t] = __longlong_as_double(0x7ff8000000000000LL);  // NaN padding
  __syncthreads();
  double objective_current = 1e10;   // OMC.jl:2012
  int counter = 0, converged = 0, failed = 0;
  const long long t_start = am_clock_start(w, tid);
  while (counter < w.max_iters) {
    if (am_out_of_time(w, tid, t_start, counter, &s_late)) break;      // OMC.jl:2186-2189: counter < max_iters && elapsed < time_limit
    ++counter;
    // ---- V-step ------------------------------------------------------------------------------------------
    double uu = 0.0;
    for (int i = tid; i < n; i += T) uu += u[i] * u[i];
    uu = block_sum(uu, red) / w.gamma;
    for (int j = tid; j < m; j += T) {
      double num = 0.0, den = uu;
      for (int p = w.col_ptr[j]; p < w.col_ptr[j + 1]; ++p) { double ui = u[w.col_idx[p]]; num += ui * w.col_val[p]; den += ui * ui; }
      v[j] = (den > 0.0) ? num / den : 0.0;
    }
    __syncthreads();
    // ---- U-step quantities -------------------------------------------------------------------------------
    double vv = 0.0;
    for (int j = tid; j < m; j += T) vv += v[j] * v[j];
    vv = block_sum(vv, red) / w.gamma;
    for (int i = tid; i < n; i += T) {
      double hh = vv, gg = 0.0;
      for (int p = w.row_ptr[i]; p < w.row_ptr[i + 1]; ++p) { double vj = v[w.row_idx[p]]; hh += vj * vj; gg += vj * w.row_val[p]; }
      h[i] = hh; g[i] = gg;
    }
    __syncthreads();
    // ---- QP: theta by bisection, rows by NNQP ----------------------------------------------------------------
    // solve(theta): minimiser over the rows for a fixed ball multiplier; returns ||u||^2 (same value in every thread)
    auto solve = [&](double theta) -> double {
      for (int i = tid; i < n; i += T) u0[i] = g[i] / (h[i] + theta);
      __syncthreads();
      // one thread per Gram entry / per row (R is small: serial dot products of length n beat R^2 block reductions)
      for (int e = tid; e < R * R; e += T) {
        int r1 = e / R, r2 = e - r1 * R;
        if (r2 < r1) continue;
        double acc = 0.0;
        for (int i = 0; i < n; ++i) { double a1 = am_row_entry(w, b, r1, i); if (a1 != 0.0) acc += a1 * am_row_entry(w, b, r2, i) / (h[i] + theta); }
        G[(size_t)r1 * w.Rmax + r2] = acc; G[(size_t)r2 * w.Rmax + r1] = acc;
      }
      for (int r = tid; r < R; r += T) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += am_row_entry(w, b, r, i) * u0[i];
        cvec[r] = acc - w.rrhs[(size_t)b * w.Rmax + r];
      }
      __syncthreads();
      if (R > 0 && tid < 64) { const int ov = wave_nnqp<true>(G, w.Rmax, cvec, mu, R, s_Gp, s_sv, s_tmp, s_pl, tid); if (tid == 0) s_ov = ov; }
      __syncthreads();
      double nn = 0.0;
      for (int i = tid; i < n; i += T) {
        double corr = 0.0;
        for (int r = 0; r < R; ++r) { double mv = mu[r]; if (mv != 0.0) corr += mv * am_row_entry(w, b, r, i); }
        double ui = u0[i] - corr / (h[i] + theta);
        u[i] = ui; nn += ui * ui;
      }
      return block_sum(nn, red);
    };
    if (tid == 0) s_ov = 0;
    __syncthreads();
    if (solve(0.0) > 1.0) {                       // ball active (OMC.jl:2164-2171)
      double lo_t = 0.0, hi_t = 1.0;
      for (int i = 0; i < n; ++i) hi_t = fmax(hi_t, fabs(g[i]));
      // an infeasible model_U (contradictory cut bounds, or rows that leave no point inside the unit ball) never enters the ball:
      // the bracket search is capped and the feasibility test below reports the failure
      for (int dbl = 0; dbl < AM_MAX_DOUBLINGS && solve(hi_t) > 1.0; ++dbl) hi_t *= 2.0;
      for (int it = 0; it < 200; ++it) {
        const double theta = 0.5 * (lo_t + hi_t);
        if (solve(theta) > 1.0) lo_t = theta; else hi_t = theta;
        if (hi_t - lo_t <= 1e-15 * fmax(1.0, hi_t)) break;
      }
      solve(hi_t);
    }
    // ---- did model_U have a solution?  (OMC.jl:2231, 2263-2265: a failed solve ends the loop with converged = false) ---------
    {
      double viol = 0.0, nn = 0.0;
      for (int r = tid; r < R; r += T) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += am_row_entry(w, b, r, i) * u[i];
        viol = fmax(viol, acc - w.rrhs[(size_t)b * w.Rmax + r]);
      }
      for (int i = tid; i < n; i += T) nn += u[i] * u[i];
      nn = block_sum(nn, red);
      viol = block_max(viol, red);
      const bool bad = !(viol <= AM_FEAS_TOL) || !(nn <= 1.0 + AM_FEAS_TOL) || s_ov;
      __syncthreads();
      if (bad) { failed = 1; break; }
    }
    // ---- objective of model_U (OMC.jl:2232) ------------------------------------------------------------------
    double q = 0.0;
    for (int i = tid; i < n; i += T) q += 0.5 * h[i] * u[i] * u[i] - g[i] * u[i];
    const double objective_new = block_sum(q, red) + 0.5 * w.sumA2;
    if (tid == 0) {
      objs[counter - 1] = objective_new;
      int conv = 0;
      const double diff = fabs((objective_new - objective_current) / objective_current);
      if (diff < w.eps) conv = 1;                                                  // OMC.jl:2235
      else if (counter > 5) {                                                      // OMC.jl:2237-2243 (quirk Q3)
        conv = 1;
        for (int i2 = 0; i2 < 5; ++i2) if (!(objs[counter - 1 - i2] > objs[counter - 6])) conv = 0;
      }
      s_stop = conv;
    }
    __syncthreads();
    converged = s_stop;
    __syncthreads();
    if (converged) break;
    objective_current = objective_new;
  }
  for (int i = tid; i < n; i += T) w.U[(size_t)b * n + i] = u[i];
  for (int j = tid; j < m; j += T) w.V[(size_t)b * m + j] = v[j];
  if (tid == 0) { w.converged[b] = failed ? 0 : converged; w.n_iters[b] = counter; }
  {   // evaluate_objective(U V) from the factors (OMC.jl:920, 925-927): 1/2 sum_Omega (u_i v_j - A_ij)^2 + ||u||^2 ||v||^2 / (2 gamma)
    __syncthreads();
    double fit = 0.0, uu2 = 0.0, vv2 = 0.0;
    for (int i = tid; i < n; i += T) {
      const double ui = u[i]; uu2 += ui * ui;
      for (int p = w.row_ptr[i]; p < w.row_ptr[i + 1]; ++p) { const double d = ui * v[w.row_idx[p]] - w.row_val[p]; fit += d * d; }
    }
    for (int j = tid; j < m; j += T) vv2 += v[j] * v[j];
    fit = block_sum(fit, red); uu2 = block_sum(uu2, red); vv2 = block_sum(vv2, red);
    if (tid == 0) w.mobj[b] = 0.5 * fit + uu2 * vv2 / (2.0 * w.gamma);
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// Rank 2 <= k <= 4 (ranks 5 .. 8: k_altmin_w below, same algorithm).  model_U has k^2 quadratic constraints sum_i (w_c' u_i)^2 <= r_c: the k unit balls (OMC.jl:2164-2171) and,
// per pair of columns, ||U_j1 +- U_j2||^2 <= 2 (OMC.jl:2029-2045).  Their multipliers theta_c >= 0 shift every row Hessian by
// the same k x k matrix S(theta) = 2 sum_c theta_c w_c w_c'; for fixed theta the problem is the row-separable QP with linear
// rows of the rank-1 case (active-set NNQP on the Gram matrix C H(theta)^-1 C').  Outer: projected Newton on the concave dual
// (gradient q_c = constraint values, Jacobian by forward differences, symmetrised, Levenberg-Marquardt damping, ascent test on
// the dual value) -- exactly the oracle's _ustep_dual_newton.  V-step: one k x k normal-equation solve per column.
// ---------------------------------------------------------------------------------------------------------------------
#define AK_KMAX 4
#define AK_QMAX 16

__device__ __forceinline__ double ak_row_x(const AltminWS& w, int b, int r, int i) {
  const int kind = w.rkind[(size_t)b * w.Rmax + r];
  const double cf = w.rcoef[(size_t)b * w.Rmax + r];
  if (kind == ROW_BOX) return (w.rbi[(size_t)b * w.Rmax + r] == i) ? cf : 0.0;
  return cf * w.cutx[((size_t)b * w.Lmax + w.rcut[(size_t)b * w.Rmax + r]) * w.n + i];
}
// A pivot of the V-step's normal equations at or below k u max_a M_aa (u = 2^-53) is a null direction of the positive semidefinite matrix
// (a zero column of U, two equal columns): the right-hand side lies in the range of M, so leaving that row and column out and giving the
// component 0 is a minimiser of model_V, and U V is the unique one.
#define AM_NULL_PIVOT_U 1.1102230246251565e-16
// in-place Gauss-Jordan inverse of a k x k symmetric positive definite matrix held in registers; false if a pivot is not positive.
// null_tol >= 0: a pivot <= null_tol is not used -- with d = 0 its row and its column of the result become 0 and no other entry changes
// (the pseudo-inverse on the other coordinates); pivots above it go through the same arithmetic as without a tolerance.
__device__ __forceinline__ bool ak_inv(double (&a)[AK_KMAX][AK_KMAX], int k, double null_tol = -1.0) {
  bool ok = true;
#pragma unroll
  for (int p = 0; p < AK_KMAX; ++p) {
    if (p >= k) continue;
    const double piv = a[p][p];
    const bool nul = null_tol >= 0.0 && !(piv > null_tol);
    if (!(piv > 0.0) && !nul) ok = false;
    const double d = nul ? 0.0 : 1.0 / piv;
    a[p][p] = 1.0;
#pragma unroll
    for (int c = 0; c < AK_KMAX; ++c) if (c < k) a[p][c] *= d;
#pragma unroll
    for (int r = 0; r < AK_KMAX; ++r) {
      if (r >= k || r == p) continue;
      const double f = a[r][p];
      a[r][p] = 0.0;
#pragma unroll
      for (int c = 0; c < AK_KMAX; ++c) if (c < k) a[r][c] -= f * a[p][c];
    }
  }
  return ok;
}

__global__ void __launch_bounds__(256) k_altmin_k(AltminWS w) {
  extern __shared__ double sm_lds[];
  double* sm = w.scratch ? w.scratch + (size_t)blockIdx.x * w.scratch_stride : sm_lds;
  __shared__ double red[32];
  __shared__ double s_Gp[NNQP_GP_DOUBLES];
  __shared__ double s_sv[NNQP_PMAX], s_tmp[NNQP_PMAX];
  __shared__ int s_pl[NNQP_PMAX];
  __shared__ double s_th[AK_QMAX], s_th2[AK_QMAX], s_q[AK_QMAX], s_qt[AK_QMAX], s_W[AK_QMAX * AK_KMAX], s_rad[AK_QMAX];
  __shared__ double s_J[AK_QMAX * AK_QMAX], s_P[AK_QMAX * AK_QMAX], s_L[AK_QMAX * AK_QMAX], s_step[AK_QMAX];
  __shared__ int s_act[AK_QMAX], s_nact, s_flag, s_stop, s_ov, s_late;
  const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int n = w.n, m = w.m, k = w.k, kk = k * k, mq = k * k, R = w.R[b];
  const AltminKLayout L = altmink_layout(n, m, k, w.Rmax);
  double* u = sm;                 // n*k, row i at u + i*k  (accepted iterate)
  double* ut = sm + L.ut;         // candidate of the last evaluation
  double *u0 = sm + L.u0, *g = sm + L.g;
  double *H = sm + L.H, *Hinv = sm + L.Hinv;      // n*k*k each
  double* v = sm + L.v;           // k*m, column j at v + j*k
  double *cvec = sm + L.cvec, *mu = sm + L.mu;
  double* G = w.G + (size_t)b * w.Rmax * w.Rmax;
  double* objs = w.objectives + (size_t)b * w.max_iters;
  for (int e = tid; e < n * k; e += T) { const int i = e % n, a = e / n; u[i * k + a] = w.U0[(size_t)b * n * k + e]; }   // input is column-major n x k
  for (int r = tid; r < w.Rmax; r += T) mu[r] = 0.0;
  for (int t = tid; t < w.max_iters; t += T) objs[t] = __longlong_as_double(0x7ff8000000000000LL);
  if (tid == 0) {   // quadratic constraint vectors: balls, then (+, -) per pair  (quadratic_constraint_vectors in the oracle)
    int c = 0;
    for (int j = 0; j < k; ++j) { for (int a = 0; a < k; ++a) s_W[c * AK_KMAX + a] = (a == j) ? 1.0 : 0.0; s_rad[c] = 1.0; ++c; }
    for (int j1 = 0; j1 < k - 1; ++j1)
      for (int j2 = j1 + 1; j2 < k; ++j2)
        for (int sg = 0; sg < 2; ++sg) {
          for (int a = 0; a < k; ++a) s_W[c * AK_KMAX + a] = (a == j1) ? 1.0 : (a == j2) ? (sg ? -1.0 : 1.0) : 0.0;
          s_rad[c] = 2.0; ++c;
        }
  }
  __syncthreads();
  // ---- one evaluation of the inner problem for multipliers th: candidate ut, constraint values qout, primal quadratic value
  auto evaluate = [&](const double* th, double* qout) -> double {
    double S[AK_KMAX][AK_KMAX];
#pragma unroll
    for (int a = 0; a < AK_KMAX; ++a)
#pragma unroll
      for (int c2 = 0; c2 < AK_KMAX; ++c2) S[a][c2] = 0.0;
    for (int c = 0; c < mq; ++c) {
      const double t2 = 2.0 * th[c];
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a)
#pragma unroll
        for (int c2 = 0; c2 < AK_KMAX; ++c2) if (a < k && c2 < k) S[a][c2] += t2 * s_W[c * AK_KMAX + a] * s_W[c * AK_KMAX + c2];
    }
    for (int i = tid; i < n; i += T) {
      double a_[AK_KMAX][AK_KMAX];
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a)
#pragma unroll
        for (int c2 = 0; c2 < AK_KMAX; ++c2) a_[a][c2] = (a < k && c2 < k) ? H[i * kk + a * k + c2] + S[a][c2] : ((a == c2) ? 1.0 : 0.0);
      ak_inv(a_, k);
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a) {
        if (a >= k) continue;
        double acc = 0.0;
#pragma unroll
        for (int c2 = 0; c2 < AK_KMAX; ++c2) if (c2 < k) { Hinv[i * kk + a * k + c2] = a_[a][c2]; acc += a_[a][c2] * g[i * k + c2]; }
        u0[i * k + a] = acc;
      }
    }
    __syncthreads();
    for (int e = tid; e < R * R; e += T) {
      const int r1 = e / R, r2 = e - r1 * R;
      if (r2 < r1) continue;
      const int j1 = w.rbj[(size_t)b * w.Rmax + r1], j2 = w.rbj[(size_t)b * w.Rmax + r2];
      double acc = 0.0;
      for (int i = 0; i < n; ++i) { const double x1 = ak_row_x(w, b, r1, i); if (x1 != 0.0) acc += x1 * ak_row_x(w, b, r2, i) * Hinv[i * kk + j1 * k + j2]; }
      G[(size_t)r1 * w.Rmax + r2] = acc; G[(size_t)r2 * w.Rmax + r1] = acc;
    }
    for (int r = tid; r < R; r += T) {
      const int j = w.rbj[(size_t)b * w.Rmax + r];
      double acc = 0.0;
      for (int i = 0; i < n; ++i) acc += ak_row_x(w, b, r, i) * u0[i * k + j];
      cvec[r] = acc - w.rrhs[(size_t)b * w.Rmax + r];
    }
    __syncthreads();
    if (R > 0 && tid < 64) { const int ov = wave_nnqp<true>(G, w.Rmax, cvec, mu, R, s_Gp, s_sv, s_tmp, s_pl, tid); if (tid == 0 && ov) s_ov = 1; }
    __syncthreads();
    double pv = 0.0;
    double qa[AK_QMAX];
#pragma unroll
    for (int c = 0; c < AK_QMAX; ++c) qa[c] = 0.0;
    for (int i = tid; i < n; i += T) {
      double ui[AK_KMAX];
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a) ui[a] = (a < k) ? u0[i * k + a] : 0.0;
      for (int r = 0; r < R; ++r) {
        const double mv = mu[r];
        if (mv == 0.0) continue;
        const double x = ak_row_x(w, b, r, i);
        if (x == 0.0) continue;
        const int j = w.rbj[(size_t)b * w.Rmax + r];
#pragma unroll
        for (int a = 0; a < AK_KMAX; ++a) if (a < k) ui[a] -= mv * x * Hinv[i * kk + a * k + j];
      }
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a) {
        if (a >= k) continue;
        ut[i * k + a] = ui[a];
        double hu = 0.0;
#pragma unroll
        for (int c2 = 0; c2 < AK_KMAX; ++c2) if (c2 < k) hu += H[i * kk + a * k + c2] * ui[c2];
        pv += ui[a] * (0.5 * hu - g[i * k + a]);
      }
#pragma unroll
      for (int c = 0; c < AK_QMAX; ++c) {
        if (c >= mq) continue;
        double d = 0.0;
#pragma unroll
        for (int a = 0; a < AK_KMAX; ++a) if (a < k) d += s_W[c * AK_KMAX + a] * ui[a];
        qa[c] += d * d;
      }
    }
#pragma unroll
    for (int c = 0; c < AK_QMAX; ++c) {
      if (c >= mq) continue;
      const double qs = block_sum(qa[c], red);
      if (tid == 0) qout[c] = qs - s_rad[c];
    }
    pv = block_sum(pv, red);
    __syncthreads();
    return pv;
  };
  auto kkt_res = [&](const double* th, const double* q) { double r_ = 0.0; for (int c = 0; c < mq; ++c) r_ = fmax(r_, fabs(fmin(th[c], -q[c]))); return r_; };
  auto dotq = [&](const double* th, const double* q) { double r_ = 0.0; for (int c = 0; c < mq; ++c) r_ += th[c] * q[c]; return r_; };

  double objective_current = 1e10;   // OMC.jl:2012
  int counter = 0, converged = 0, failed = 0;
  const long long t_start = am_clock_start(w, tid);
  while (counter < w.max_iters) {
    if (am_out_of_time(w, tid, t_start, counter, &s_late)) break;      // OMC.jl:2186-2189: counter < max_iters && elapsed < time_limit
    ++counter;
    // ---- V-step (model_V, OMC.jl:2192-2209): (sum_{i in O_j} u_i u_i' + U'U / gamma) v_j = sum_{i in O_j} A_ij u_i ---------
    double utu[AK_KMAX][AK_KMAX];
#pragma unroll
    for (int a = 0; a < AK_KMAX; ++a)
#pragma unroll
      for (int c2 = 0; c2 < AK_KMAX; ++c2) {
        double acc = 0.0;
        if (a < k && c2 < k) { for (int i = tid; i < n; i += T) acc += u[i * k + a] * u[i * k + c2]; acc = block_sum(acc, red) / w.gamma; }
        utu[a][c2] = acc;
      }
    for (int j = tid; j < m; j += T) {
      double a_[AK_KMAX][AK_KMAX], rhs[AK_KMAX];
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a) { rhs[a] = 0.0;
#pragma unroll
        for (int c2 = 0; c2 < AK_KMAX; ++c2) a_[a][c2] = (a < k && c2 < k) ? utu[a][c2] : ((a == c2) ? 1.0 : 0.0); }
      for (int p = w.col_ptr[j]; p < w.col_ptr[j + 1]; ++p) {
        const int i = w.col_idx[p]; const double av = w.col_val[p];
#pragma unroll
        for (int a = 0; a < AK_KMAX; ++a) {
          if (a >= k) continue;
          const double ua = u[i * k + a];
          rhs[a] += av * ua;
#pragma unroll
          for (int c2 = 0; c2 < AK_KMAX; ++c2) if (c2 < k) a_[a][c2] += ua * u[i * k + c2];
        }
      }
      double dmax = 0.0;
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a) if (a < k) dmax = fmax(dmax, a_[a][a]);
      ak_inv(a_, k, k * AM_NULL_PIVOT_U * dmax);
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a) {
        if (a >= k) continue;
        double acc = 0.0;
#pragma unroll
        for (int c2 = 0; c2 < AK_KMAX; ++c2) if (c2 < k) acc += a_[a][c2] * rhs[c2];
        v[j * k + a] = acc;
      }
    }
    __syncthreads();
    // ---- U-step quantities: H_i = sum_{j in O_i} v_j v_j' + V V' / gamma, g_i = sum_{j in O_i} A_ij v_j --------------------------
    double vvt[AK_KMAX][AK_KMAX];
#pragma unroll
    for (int a = 0; a < AK_KMAX; ++a)
#pragma unroll
      for (int c2 = 0; c2 < AK_KMAX; ++c2) {
        double acc = 0.0;
        if (a < k && c2 < k) { for (int j = tid; j < m; j += T) acc += v[j * k + a] * v[j * k + c2]; acc = block_sum(acc, red) / w.gamma; }
        vvt[a][c2] = acc;
      }
    for (int i = tid; i < n; i += T) {
      double hh[AK_KMAX][AK_KMAX], gg[AK_KMAX];
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a) { gg[a] = 0.0;
#pragma unroll
        for (int c2 = 0; c2 < AK_KMAX; ++c2) hh[a][c2] = vvt[a][c2]; }
      for (int p = w.row_ptr[i]; p < w.row_ptr[i + 1]; ++p) {
        const int j = w.row_idx[p]; const double av = w.row_val[p];
#pragma unroll
        for (int a = 0; a < AK_KMAX; ++a) {
          if (a >= k) continue;
          const double va = v[j * k + a];
          gg[a] += av * va;
#pragma unroll
          for (int c2 = 0; c2 < AK_KMAX; ++c2) if (c2 < k) hh[a][c2] += va * v[j * k + c2];
        }
      }
#pragma unroll
      for (int a = 0; a < AK_KMAX; ++a) {
        if (a >= k) continue;
        g[i * k + a] = gg[a];
#pragma unroll
        for (int c2 = 0; c2 < AK_KMAX; ++c2) if (c2 < k) H[i * kk + a * k + c2] = hh[a][c2];
      }
    }
    if (tid == 0) for (int c = 0; c < mq; ++c) s_th[c] = 0.0;
    __syncthreads();
    // ---- U-step: projected Newton on the dual ------------------------------------------------------------------------------
    if (tid == 0) s_ov = 0;
    __syncthreads();
    double pv = evaluate(s_th, s_q);
    for (int e = tid; e < n * k; e += T) u[e] = ut[e];
    __syncthreads();
    double dv = pv + dotq(s_th, s_q), res = kkt_res(s_th, s_q), lm = 1e-10;
    for (int nit = 0; nit < 60 && res > 1e-12; ++nit) {
      if (tid == 0) { int na = 0; for (int c = 0; c < mq; ++c) if (s_th[c] > 0.0 || s_q[c] > 0.0) s_act[na++] = c; s_nact = na; }
      __syncthreads();
      const int na = s_nact;
      for (int a = 0; a < na; ++a) {
        const int c = s_act[a];
        const double dl = 1e-7 * fmax(1.0, s_th[c]);
        if (tid == 0) { for (int c2 = 0; c2 < mq; ++c2) s_th2[c2] = s_th[c2]; s_th2[c] += dl; }
        __syncthreads();
        evaluate(s_th2, s_qt);
        if (tid == 0) for (int a2 = 0; a2 < na; ++a2) s_J[a2 * AK_QMAX + a] = (s_qt[s_act[a2]] - s_q[s_act[a2]]) / dl;
        __syncthreads();
      }
      double tr = 0.0;
      if (tid == 0) for (int a = 0; a < na; ++a) for (int a2 = 0; a2 < na; ++a2) s_P[a * AK_QMAX + a2] = -0.5 * (s_J[a * AK_QMAX + a2] + s_J[a2 * AK_QMAX + a]);
      __syncthreads();
      for (int a = 0; a < na; ++a) tr += s_P[a * AK_QMAX + a];
      const double scale = fmax(tr, 1e-300) / na;
      bool accepted = false;
      for (int tr_ = 0; tr_ < 40; ++tr_) {
        if (tid == 0) {   // (P + lm scale I) step = q_act by Cholesky; candidate multipliers
          int ok = 1;
          for (int c = 0; c < na && ok; ++c) {
            double dg = s_P[c * AK_QMAX + c] + lm * scale;
            for (int q2 = 0; q2 < c; ++q2) dg -= s_L[c * AK_QMAX + q2] * s_L[c * AK_QMAX + q2];
            if (!(dg > 0.0)) { ok = 0; break; }
            dg = sqrt(dg); s_L[c * AK_QMAX + c] = dg;
            for (int r2 = c + 1; r2 < na; ++r2) {
              double vv = s_P[r2 * AK_QMAX + c];
              for (int q2 = 0; q2 < c; ++q2) vv -= s_L[r2 * AK_QMAX + q2] * s_L[c * AK_QMAX + q2];
              s_L[r2 * AK_QMAX + c] = vv / dg;
            }
          }
          if (ok) {
            for (int i = 0; i < na; ++i) { double vv = s_q[s_act[i]]; for (int q2 = 0; q2 < i; ++q2) vv -= s_L[i * AK_QMAX + q2] * s_step[q2]; s_step[i] = vv / s_L[i * AK_QMAX + i]; }
            for (int i = na - 1; i >= 0; --i) { double vv = s_step[i]; for (int q2 = i + 1; q2 < na; ++q2) vv -= s_L[q2 * AK_QMAX + i] * s_step[q2]; s_step[i] = vv / s_L[i * AK_QMAX + i]; }
            for (int c = 0; c < mq; ++c) s_th2[c] = s_th[c];
            for (int i = 0; i < na; ++i) s_th2[s_act[i]] = fmax(s_th[s_act[i]] + s_step[i], 0.0);
          }
          s_flag = ok;
        }
        __syncthreads();
        if (!s_flag) { lm *= 10.0; __syncthreads(); continue; }
        const double pvn = evaluate(s_th2, s_qt);
        const double dn = pvn + dotq(s_th2, s_qt), rn = kkt_res(s_th2, s_qt);
        double lin = 0.0;
        for (int c = 0; c < mq; ++c) lin += s_q[c] * (s_th2[c] - s_th[c]);
        const bool ok2 = (dn >= dv + 1e-4 * lin - 1e-14 * fmax(1.0, fabs(dv))) && (dn > dv || rn < res);
        __syncthreads();
        if (ok2) {
          if (tid == 0) for (int c = 0; c < mq; ++c) { s_th[c] = s_th2[c]; s_q[c] = s_qt[c]; }
          for (int e = tid; e < n * k; e += T) u[e] = ut[e];
          __syncthreads();
          res = rn; dv = dn; pv = pvn; lm = fmax(lm * 0.1, 1e-12); accepted = true;
          break;
        }
        lm *= 10.0;
      }
      if (!accepted) break;
    }
    // ---- did model_U have a solution?  (OMC.jl:2231, 2263-2265: a failed solve ends the loop with converged = false) ---------
    {
      double viol = 0.0;
      for (int r = tid; r < R; r += T) {
        const int j = w.rbj[(size_t)b * w.Rmax + r];
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += ak_row_x(w, b, r, i) * u[i * k + j];
        viol = fmax(viol, acc - w.rrhs[(size_t)b * w.Rmax + r]);
      }
      for (int c = 0; c < mq; ++c) viol = fmax(viol, s_q[c]);
      viol = block_max(viol, red);
      // s_ov is sticky over the evaluations of this U-step: a rejected trial may have set it, so it is only trusted together with a violation
      const bool bad = !(viol <= AM_FEAS_TOL) || (s_ov && viol > 1e-9);
      __syncthreads();
      if (bad) { failed = 1; break; }
    }
    // ---- objective of model_U (OMC.jl:2232) and the convergence rules (2234-2245, quirk Q3) ---------------------------------
    const double objective_new = pv + 0.5 * w.sumA2;
    if (tid == 0) {
      objs[counter - 1] = objective_new;
      int conv = 0;
      const double diff = fabs((objective_new - objective_current) / objective_current);
      if (diff < w.eps) conv = 1;
      else if (counter > 5) {
        conv = 1;
        for (int i2 = 0; i2 < 5; ++i2) if (!(objs[counter - 1 - i2] > objs[counter - 6])) conv = 0;
      }
      s_stop = conv;
    }
    __syncthreads();
    converged = s_stop;
    __syncthreads();
    if (converged) break;
    objective_current = objective_new;
  }
  for (int e = tid; e < n * k; e += T) { const int i = e % n, a = e / n; w.U[(size_t)b * n * k + e] = u[i * k + a]; }
  for (int e = tid; e < k * m; e += T) w.V[(size_t)b * k * m + e] = v[e];      // k x m column-major = v[j*k + a]
  if (tid == 0) { w.converged[b] = failed ? 0 : converged; w.n_iters[b] = counter; }
  {   // evaluate_objective(U V) from the factors: masked fit over the CSR rows + tr((U'U)(V V')) / (2 gamma)
    __syncthreads();
    double fit = 0.0;
    for (int i = tid; i < n; i += T) {
      for (int p = w.row_ptr[i]; p < w.row_ptr[i + 1]; ++p) {
        const int j = w.row_idx[p];
        double x = 0.0;
        for (int a = 0; a < k; ++a) x += u[i * k + a] * v[j * k + a];
        const double d = x - w.row_val[p]; fit += d * d;
      }
    }
    fit = block_sum(fit, red);
    double reg = 0.0;
    for (int a = 0; a < k; ++a)
      for (int c2 = 0; c2 < k; ++c2) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = tid; i < n; i += T) s1 += u[i * k + a] * u[i * k + c2];
        for (int j = tid; j < m; j += T) s2 += v[j * k + a] * v[j * k + c2];
        s1 = block_sum(s1, red); s2 = block_sum(s2, red);
        reg += s1 * s2;
      }
    if (tid == 0) w.mobj[b] = 0.5 * fit + reg / (2.0 * w.gamma);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Ranks 5 <= k <= 8 (k_altmin_w): the algorithm of k_altmin_k, organised without per-thread k x k or k^2 arrays.
//   * every k x k solve (H_i + S(theta) per row i, the normal equations per column j) belongs to a group of 8 lanes: lane a holds row a of
//     the matrix in 8 registers, Gauss-Jordan with in-group shuffles (the steps of ak_inv, same pivot test), 32 matrices per pass of the workgroup;
//   * the k^2 constraint values come from the k x k Gram matrix U'U: ball j = G_jj - 1, pair (a, b, +-) = G_aa + G_bb +- 2 G_ab - 2;
//   * multiplier vectors, Jacobian, model matrix and Cholesky factor of the dual Newton method live in the working block (altminw_layout,
//     leading dimension k^2); the damped Cholesky and its two triangular solves run on wave 0 (wave_cholesky / wave_chol_solve);
//   * scalar decisions (Newton residual, ascent test, damping) are taken by thread 0, published through LDS and read after a barrier.
// ---------------------------------------------------------------------------------------------------------------------
#define AW_KMAX ALTMIN_KMAX
#define AW_QMAX (AW_KMAX * AW_KMAX)

// in-place Gauss-Jordan inverse of a symmetric positive definite matrix spread over 8 lanes (lane a = row a; rows and columns >= k are the
// identity); false, for the whole group, if a pivot is not positive.  null_tol as in ak_inv (the same value in the 8 lanes of a group).
__device__ __forceinline__ bool aw_inv8(double (&row)[AW_KMAX], int k, int a, double null_tol = -1.0) {
  bool ok = true;
#pragma unroll
  for (int p = 0; p < AW_KMAX; ++p) {
    if (p >= k) continue;                            // k is the same in every thread
    const double piv = __shfl(row[p], p, AW_KMAX);
    const bool nul = null_tol >= 0.0 && !(piv > null_tol);
    if (!(piv > 0.0) && !nul) ok = false;
    const double d = nul ? 0.0 : 1.0 / piv;
    if (a == p) {
      row[p] = 1.0;
#pragma unroll
      for (int c = 0; c < AW_KMAX; ++c) row[c] *= d;
    }
    double pr[AW_KMAX];
#pragma unroll
    for (int c = 0; c < AW_KMAX; ++c) pr[c] = __shfl(row[c], p, AW_KMAX);
    if (a != p) {
      const double f = row[p];
      row[p] = 0.0;
#pragma unroll
      for (int c = 0; c < AW_KMAX; ++c) row[c] -= f * pr[c];
    }
  }
  return ok;
}

// out[a * AW_KMAX + c] = scale * sum_t x[t * k + a] x[t * k + c] (both triangles): one wave per pair a <= c; ends with a workgroup barrier
__device__ __forceinline__ void aw_gram(const double* x, int cnt, int k, double scale, double* out) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int np = k * (k + 1) / 2;
  for (int p = wv; p < np; p += nw) {                // wave-uniform
    int a = 0, rest = p;
    while (rest >= k - a) { rest -= k - a; ++a; }
    const int c = a + rest;
    double acc = 0.0;
    for (int t = lane; t < cnt; t += WAVE) acc += x[(size_t)t * k + a] * x[(size_t)t * k + c];
    acc = wave_sum(acc) * scale;
    if (lane == 0) { out[a * AW_KMAX + c] = acc; out[c * AW_KMAX + a] = acc; }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(256) k_altmin_w(AltminWS w) {
  extern __shared__ double sm_lds[];
  double* sm = w.scratch ? w.scratch + (size_t)blockIdx.x * w.scratch_stride : sm_lds;
  __shared__ double red[32];
  __shared__ double s_Gp[NNQP_GP_DOUBLES];
  __shared__ double s_sv[NNQP_PMAX], s_tmp[NNQP_PMAX];
  __shared__ int s_pl[NNQP_PMAX];
  __shared__ double s_S[AW_QMAX], s_Gu[AW_QMAX], s_Gv[AW_QMAX], s_sg[AW_QMAX];      // S(theta), Gram matrices (k x k in 8 x 8), sign of a pair constraint
  __shared__ int s_j1[AW_QMAX], s_j2[AW_QMAX];                                      // columns of a constraint (s_j2 = -1: ball)
  __shared__ double s_res, s_dv, s_pv, s_lm, s_scale;                               // Newton scalars, owned by thread 0
  __shared__ int s_nact, s_flag, s_stop, s_ov, s_late;
  const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int n = w.n, m = w.m, k = w.k, kk = k * k, mq = k * k, R = w.R[b];
  const int grp = tid >> 3, ga = tid & 7, NG = T >> 3;      // 8-lane group of the k x k solves, row held by this lane
  const int gac = ga < k ? ga : 0;                          // clamped row: padding lanes load in range and discard
  const AltminWLayout L = altminw_layout(n, m, k, w.Rmax);
  double* u = sm;                 // n*k, row i at u + i*k  (accepted iterate)
  double* ut = sm + L.ut;         // candidate of the last evaluation
  double *u0 = sm + L.u0, *g = sm + L.g;
  double *H = sm + L.H, *Hinv = sm + L.Hinv;      // n*k*k each
  double* v = sm + L.v;           // k*m, column j at v + j*k
  double *cvec = sm + L.cvec, *mu = sm + L.mu;
  double *th = sm + L.th, *th2 = sm + L.th2, *q = sm + L.q, *qt = sm + L.qt, *step = sm + L.step, *tmpv = sm + L.tmp;
  int* act = (int*)(sm + L.act);
  double *J = sm + L.J, *P = sm + L.P, *Lc = sm + L.Lc;
  double* G = w.G + (size_t)b * w.Rmax * w.Rmax;
  double* objs = w.objectives + (size_t)b * w.max_iters;
  for (int e = tid; e < n * k; e += T) { const int i = e % n, a = e / n; u[i * k + a] = w.U0[(size_t)b * n * k + e]; }   // input is column-major n x k
  for (int r = tid; r < w.Rmax; r += T) mu[r] = 0.0;
  for (int t = tid; t < w.max_iters; t += T) objs[t] = __longlong_as_double(0x7ff8000000000000LL);
  if (tid == 0) {   // quadratic constraints: balls, then (+, -) per pair  (quadratic_constraint_vectors in the oracle)
    int c = 0;
    for (int j = 0; j < k; ++j) { s_j1[c] = j; s_j2[c] = -1; s_sg[c] = 0.0; ++c; }
    for (int j1 = 0; j1 < k - 1; ++j1)
      for (int j2 = j1 + 1; j2 < k; ++j2)
        for (int sg = 0; sg < 2; ++sg) { s_j1[c] = j1; s_j2[c] = j2; s_sg[c] = sg ? -1.0 : 1.0; ++c; }
  }
  __syncthreads();
  // ---- one evaluation of the inner problem for multipliers tha: candidate ut, constraint values qout, primal quadratic value
  auto evaluate = [&](const double* tha, double* qout) -> double {
    if (tid < AW_QMAX) {      // S(theta) = 2 sum_c theta_c w_c w_c'
      const int a = tid >> 3, c2 = tid & 7;
      double acc = 0.0;
      for (int c = 0; c < mq; ++c) {
        const int j1 = s_j1[c], j2 = s_j2[c];
        const double wa = (a == j1) ? 1.0 : (a == j2) ? s_sg[c] : 0.0, wc = (c2 == j1) ? 1.0 : (c2 == j2) ? s_sg[c] : 0.0;
        acc += 2.0 * tha[c] * wa * wc;
      }
      s_S[tid] = acc;
    }
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += NG) {      // (H_i + S)^-1 and u0_i = (H_i + S)^-1 g_i, one row i per 8-lane group
      const int i = i0 + grp; const bool valid = i < n; const int ic = valid ? i : n - 1;
      double row[AW_KMAX];
#pragma unroll
      for (int c = 0; c < AW_KMAX; ++c) {
        const double hv = H[ic * kk + gac * k + (c < k ? c : 0)] + s_S[gac * AW_KMAX + c];
        row[c] = (ga < k && c < k) ? hv : ((ga == c) ? 1.0 : 0.0);
      }
      aw_inv8(row, k, ga);
      const double gv = g[ic * k + gac];
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < AW_KMAX; ++c) { const double gc = __shfl(gv, c, AW_KMAX); if (c < k) acc += row[c] * gc; }
      if (valid && ga < k) {
#pragma unroll
        for (int c = 0; c < AW_KMAX; ++c) if (c < k) Hinv[i * kk + ga * k + c] = row[c];
        u0[i * k + ga] = acc;
      }
    }
    __syncthreads();
    for (int e = tid; e < R * R; e += T) {
      const int r1 = e / R, r2 = e - r1 * R;
      if (r2 < r1) continue;
      const int j1 = w.rbj[(size_t)b * w.Rmax + r1], j2 = w.rbj[(size_t)b * w.Rmax + r2];
      double acc = 0.0;
      for (int i = 0; i < n; ++i) { const double x1 = ak_row_x(w, b, r1, i); if (x1 != 0.0) acc += x1 * ak_row_x(w, b, r2, i) * Hinv[i * kk + j1 * k + j2]; }
      G[(size_t)r1 * w.Rmax + r2] = acc; G[(size_t)r2 * w.Rmax + r1] = acc;
    }
    for (int r = tid; r < R; r += T) {
      const int j = w.rbj[(size_t)b * w.Rmax + r];
      double acc = 0.0;
      for (int i = 0; i < n; ++i) acc += ak_row_x(w, b, r, i) * u0[i * k + j];
      cvec[r] = acc - w.rrhs[(size_t)b * w.Rmax + r];
    }
    __syncthreads();
    if (R > 0 && tid < 64) { const int ov = wave_nnqp<true>(G, w.Rmax, cvec, mu, R, s_Gp, s_sv, s_tmp, s_pl, tid); if (tid == 0 && ov) s_ov = 1; }
    __syncthreads();
    for (int e = tid; e < n * k; e += T) {      // ut = u0 - sum_r mu_r x_r(i) Hinv_i[:, j_r]
      const int i = e / k, a = e - i * k;
      double ui = u0[e];
      for (int r = 0; r < R; ++r) {
        const double mv = mu[r];
        if (mv == 0.0) continue;
        const double x = ak_row_x(w, b, r, i);
        if (x == 0.0) continue;
        ui -= mv * x * Hinv[i * kk + a * k + w.rbj[(size_t)b * w.Rmax + r]];
      }
      ut[e] = ui;
    }
    __syncthreads();
    double pv = 0.0;
    for (int e = tid; e < n * k; e += T) {
      const int i = e / k, a = e - i * k;
      double hu = 0.0;
      for (int c2 = 0; c2 < k; ++c2) hu += H[i * kk + a * k + c2] * ut[i * k + c2];
      pv += ut[e] * (0.5 * hu - g[e]);
    }
    pv = block_sum(pv, red);
    aw_gram(ut, n, k, 1.0, s_Gu);
    if (tid < mq) {
      const int j1 = s_j1[tid], j2 = s_j2[tid];
      qout[tid] = (j2 < 0) ? s_Gu[j1 * AW_KMAX + j1] - 1.0
                           : s_Gu[j1 * AW_KMAX + j1] + s_Gu[j2 * AW_KMAX + j2] + s_sg[tid] * 2.0 * s_Gu[j1 * AW_KMAX + j2] - 2.0;
    }
    __syncthreads();
    return pv;
  };
  // thread 0 only
  auto kkt_res = [&](const double* tha, const double* qa) { double r_ = 0.0; for (int c = 0; c < mq; ++c) r_ = fmax(r_, fabs(fmin(tha[c], -qa[c]))); return r_; };
  auto dotq = [&](const double* tha, const double* qa) { double r_ = 0.0; for (int c = 0; c < mq; ++c) r_ += tha[c] * qa[c]; return r_; };

  double objective_current = 1e10;   // OMC.jl:2012
  int counter = 0, converged = 0, failed = 0;
  const long long t_start = am_clock_start(w, tid);
  while (counter < w.max_iters) {
    if (am_out_of_time(w, tid, t_start, counter, &s_late)) break;      // OMC.jl:2186-2189: counter < max_iters && elapsed < time_limit
    ++counter;
    // ---- V-step (model_V, OMC.jl:2192-2209): (sum_{i in O_j} u_i u_i' + U'U / gamma) v_j = sum_{i in O_j} A_ij u_i ---------
    aw_gram(u, n, k, 1.0 / w.gamma, s_Gu);
    for (int j0 = 0; j0 < m; j0 += NG) {
      const int j = j0 + grp; const bool valid = j < m; const int jc = valid ? j : m - 1;
      double row[AW_KMAX], rhs = 0.0;
#pragma unroll
      for (int c = 0; c < AW_KMAX; ++c) row[c] = (ga < k && c < k) ? s_Gu[ga * AW_KMAX + c] : ((ga == c) ? 1.0 : 0.0);
      for (int p = w.col_ptr[jc]; p < w.col_ptr[jc + 1]; ++p) {
        const int i = w.col_idx[p]; const double av = w.col_val[p];
        const double ua = u[i * k + gac];
        rhs += av * ua;
#pragma unroll
        for (int c = 0; c < AW_KMAX; ++c) { const double uc = u[i * k + (c < k ? c : 0)]; if (ga < k && c < k) row[c] += ua * uc; }
      }
      double dmax = 0.0;                       // largest diagonal entry of the k x k block: this lane's, then over the group
#pragma unroll
      for (int c = 0; c < AW_KMAX; ++c) if (c == ga && c < k) dmax = row[c];
      for (int o = AW_KMAX >> 1; o > 0; o >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, o, AW_KMAX));
      aw_inv8(row, k, ga, k * AM_NULL_PIVOT_U * dmax);
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < AW_KMAX; ++c) { const double rc = __shfl(rhs, c, AW_KMAX); if (c < k) acc += row[c] * rc; }
      if (valid && ga < k) v[j * k + ga] = acc;
    }
    __syncthreads();
    // ---- U-step quantities: H_i = sum_{j in O_i} v_j v_j' + V V' / gamma, g_i = sum_{j in O_i} A_ij v_j --------------------------
    aw_gram(v, m, k, 1.0 / w.gamma, s_Gv);
    for (int i0 = 0; i0 < n; i0 += NG) {
      const int i = i0 + grp;
      if (i >= n || ga >= k) continue;       // no cross-lane traffic in this loop
      double hh[AW_KMAX], gg = 0.0;
#pragma unroll
      for (int c = 0; c < AW_KMAX; ++c) hh[c] = s_Gv[ga * AW_KMAX + c];
      for (int p = w.row_ptr[i]; p < w.row_ptr[i + 1]; ++p) {
        const int j = w.row_idx[p]; const double av = w.row_val[p];
        const double va = v[j * k + ga];
        gg += av * va;
#pragma unroll
        for (int c = 0; c < AW_KMAX; ++c) if (c < k) hh[c] += va * v[j * k + c];
      }
      g[i * k + ga] = gg;
#pragma unroll
      for (int c = 0; c < AW_KMAX; ++c) if (c < k) H[i * kk + ga * k + c] = hh[c];
    }
    if (tid < mq) th[tid] = 0.0;
    if (tid == 0) s_ov = 0;
    __syncthreads();
    // ---- U-step: projected Newton on the dual ------------------------------------------------------------------------------
    {
      const double pv0 = evaluate(th, q);
      for (int e = tid; e < n * k; e += T) u[e] = ut[e];
      if (tid == 0) { s_pv = pv0; s_dv = pv0 + dotq(th, q); s_res = kkt_res(th, q); s_lm = 1e-10; }
      __syncthreads();
    }
    for (int nit = 0; nit < 60; ++nit) {
      if (!(s_res > 1e-12)) break;           // written by thread 0 before the last barrier; the next write is barriers away
      if (tid == 0) { int na = 0; for (int c = 0; c < mq; ++c) if (th[c] > 0.0 || q[c] > 0.0) act[na++] = c; s_nact = na; }
      __syncthreads();
      const int na = s_nact;
      for (int a = 0; a < na; ++a) {         // forward-difference Jacobian of q over the active set, column a
        const int c = act[a];
        const double dl = 1e-7 * fmax(1.0, th[c]);
        if (tid < mq) th2[tid] = th[tid] + ((tid == c) ? dl : 0.0);
        __syncthreads();
        evaluate(th2, qt);
        if (tid < na) J[tid * mq + a] = (qt[act[tid]] - q[act[tid]]) / dl;
        __syncthreads();
      }
      for (int e = tid; e < na * na; e += T) { const int a = e / na, a2 = e - a * na; P[a * mq + a2] = -0.5 * (J[a * mq + a2] + J[a2 * mq + a]); }
      __syncthreads();
      if (tid == 0) { double tr = 0.0; for (int a = 0; a < na; ++a) tr += P[a * mq + a]; s_scale = fmax(tr, 1e-300) / na; }
      __syncthreads();
      int accepted = 0;
      for (int tr_ = 0; tr_ < 40; ++tr_) {
        if (tid < WAVE) {   // wave 0: (P + lm scale I) step = q_act by Cholesky; candidate multipliers
          const double damp = s_lm * s_scale;
          for (int e = tid; e < na * na; e += WAVE) { const int a = e / na, a2 = e - a * na; if (a2 <= a) Lc[TRI(a, a2)] = P[a * mq + a2] + ((a == a2) ? damp : 0.0); }
          WAVE_SYNC();
          const bool ok = wave_cholesky(Lc, na, tid);
          if (ok) {
            for (int i = tid; i < na; i += WAVE) tmpv[i] = q[act[i]];
            WAVE_SYNC();
            wave_chol_solve(Lc, na, tmpv, step, tid);
            for (int c = tid; c < mq; c += WAVE) th2[c] = th[c];
            WAVE_SYNC();
            for (int i = tid; i < na; i += WAVE) th2[act[i]] = fmax(th[act[i]] + step[i], 0.0);
          }
          if (tid == 0) { s_flag = ok ? 1 : 0; if (!ok) s_lm *= 10.0; }
        }
        __syncthreads();
        if (!s_flag) { __syncthreads(); continue; }
        const double pvn = evaluate(th2, qt);
        if (tid == 0) {
          const double dv = s_dv, res = s_res;
          const double dn = pvn + dotq(th2, qt), rn = kkt_res(th2, qt);
          double lin = 0.0;
          for (int c = 0; c < mq; ++c) lin += q[c] * (th2[c] - th[c]);
          const bool ok2 = (dn >= dv + 1e-4 * lin - 1e-14 * fmax(1.0, fabs(dv))) && (dn > dv || rn < res);
          if (ok2) { s_res = rn; s_dv = dn; s_pv = pvn; s_lm = fmax(s_lm * 0.1, 1e-12); }
          else s_lm *= 10.0;
          s_stop = ok2 ? 1 : 0;
        }
        __syncthreads();
        accepted = s_stop;
        if (accepted) {
          if (tid < mq) { th[tid] = th2[tid]; q[tid] = qt[tid]; }
          for (int e = tid; e < n * k; e += T) u[e] = ut[e];
        }
        __syncthreads();
        if (accepted) break;
      }
      if (!accepted) break;
    }
    // ---- did model_U have a solution?  (OMC.jl:2231, 2263-2265: a failed solve ends the loop with converged = false) ---------
    {
      double viol = 0.0;
      for (int r = tid; r < R; r += T) {
        const int j = w.rbj[(size_t)b * w.Rmax + r];
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += ak_row_x(w, b, r, i) * u[i * k + j];
        viol = fmax(viol, acc - w.rrhs[(size_t)b * w.Rmax + r]);
      }
      for (int c = tid; c < mq; c += T) viol = fmax(viol, q[c]);
      viol = block_max(viol, red);
      // s_ov is sticky over the evaluations of this U-step: a rejected trial may have set it, so it is only trusted together with a violation
      const bool bad = !(viol <= AM_FEAS_TOL) || (s_ov && viol > 1e-9);
      __syncthreads();
      if (bad) { failed = 1; break; }
    }
    // ---- objective of model_U (OMC.jl:2232) and the convergence rules (2234-2245, quirk Q3) ---------------------------------
    const double objective_new = s_pv + 0.5 * w.sumA2;
    if (tid == 0) {
      objs[counter - 1] = objective_new;
      int conv = 0;
      const double diff = fabs((objective_new - objective_current) / objective_current);
      if (diff < w.eps) conv = 1;
      else if (counter > 5) {
        conv = 1;
        for (int i2 = 0; i2 < 5; ++i2) if (!(objs[counter - 1 - i2] > objs[counter - 6])) conv = 0;
      }
      s_stop = conv;
    }
    __syncthreads();
    converged = s_stop;
    __syncthreads();
    if (converged) break;
    objective_current = objective_new;
  }
  __syncthreads();
  for (int e = tid; e < n * k; e += T) { const int i = e % n, a = e / n; w.U[(size_t)b * n * k + e] = u[i * k + a]; }
  for (int e = tid; e < k * m; e += T) w.V[(size_t)b * k * m + e] = v[e];      // k x m column-major = v[j*k + a]
  if (tid == 0) { w.converged[b] = failed ? 0 : converged; w.n_iters[b] = counter; }
  {   // evaluate_objective(U V) from the factors: masked fit over the CSR rows + tr((U'U)(V V')) / (2 gamma)
    double fit = 0.0;
    for (int i = tid; i < n; i += T) {
      for (int p = w.row_ptr[i]; p < w.row_ptr[i + 1]; ++p) {
        const int j = w.row_idx[p];
        double x = 0.0;
        for (int a = 0; a < k; ++a) x += u[i * k + a] * v[j * k + a];
        const double d = x - w.row_val[p]; fit += d * d;
      }
    }
    fit = block_sum(fit, red);
    aw_gram(u, n, k, 1.0, s_Gu);
    aw_gram(v, m, k, 1.0, s_Gv);
    if (tid == 0) {
      double reg = 0.0;
      for (int a = 0; a < k; ++a) for (int c2 = 0; c2 < k; ++c2) reg += s_Gu[a * AW_KMAX + c2] * s_Gv[a * AW_KMAX + c2];
      w.mobj[b] = 0.5 * fit + reg / (2.0 * w.gamma);
    }
  }
}

extern "C" void omc_launch_altmin(const AltminWS* w, hipStream_t s) {      // rank-1 or rank-k kernel, launch bytes from the descriptor (altmin_plan)
  const int var = altmin_variant(w->k);
  if (var == 1) hipLaunchKernelGGL(k_altmin, dim3(w->B), dim3(256), w->lds_bytes, s, *w);
  else if (var == 2) hipLaunchKernelGGL(k_altmin_k, dim3(w->B), dim3(256), w->lds_bytes, s, *w);
  else hipLaunchKernelGGL(k_altmin_w, dim3(w->B), dim3(256), w->lds_bytes, s, *w);
}
extern "C" int omc_altmin_set_lds(void) {
  // k_altmin_k holds ~20 KB of static LDS (Newton scratch, NNQP): its dynamic budget is 128 KB
  if (hipFuncSetAttribute((const void*)k_altmin_k, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024) != hipSuccess) (void)hipGetLastError();
  if (hipFuncSetAttribute((const void*)k_altmin_w, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024) != hipSuccess) (void)hipGetLastError();      // ~21 KB static
  return (int)hipFuncSetAttribute((const void*)k_altmin, hipFuncAttributeMaxDynamicSharedMemorySize, OMC_MAX_DYN_LDS - 8 * 1024);   // ~18 KB static (NNQP scratch)
}
