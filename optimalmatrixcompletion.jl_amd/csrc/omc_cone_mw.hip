// omc_cone_mw.hip -- the spectral projection of k_cone_ws (omc_device.hip) spread over the device: block one-sided Jacobi, one launch per
// round of the tournament.  Same mathematics: G = (M + sigma I) V_prev (or M + sigma I), sigma = 1.5 ||M||_F, columns of G rotated until
// they are orthogonal, lambda_t = ||g_t|| - sigma, v_t = g_t / ||g_t||; same outputs (Vrow / vvalid, W1, the seeds of k_cone_sub, evsum).
//   k_mw_prepare  tiles x slots    G by v_mfma_f64_16x16x4_f64, column-major in the per-slot slab (MwLayout, omc_layout.h)
//   k_mw_round    pairs x slots    one workgroup per pair of 16-column blocks: 32 x 32 Gram matrix of its N x 32 panel (MFMA), its
//                                  eigenvectors Q by one-sided Jacobi in LDS, panel <- panel Q (MFMA)
//   k_mw_norms    blocks x slots   squared column norms, eigenvalues, Vrow
//   k_mw_select   slots            clip selection, seeds of the tracked subspace, evsum, sweep statistics
//   k_mw_rebuild  tiles x slots    W1 = base M + sum wgt g g' (MFMA rank-c update, symmetric stores)
// The plain operations (CONE_SEP, CONE_TOPK of k_cone: separation vector, the k dominant eigenvectors) as a sequence on the same round kernel:
//   k_mw_plain_fro      row tiles x slots   partial sums of squares of the symmetrised input (U U' - Y, or Y), one per 16-row tile
//   k_mw_plain_prepare  tiles x slots       sigma from the partials in a fixed order, G = M + sigma I with the zero padding
//   k_mw_round                              rotation threshold and stop rule MW_TAU_PLAIN (the cold kernel's 1e-14)
//   k_mw_plain_norms    blocks x slots      squared column norms, eigenvalues
//   k_mw_plain_pick     slots               the selection of k_cone in these modes: lmin, bx / U
// Workgroups of one launch never wait for each other; rounds are ordered by the stream.  The host cannot see convergence inside a call: it
// enqueues mw_budget sweeps, every round kernel records the largest squared relative cross product its pair showed BEFORE rotating
// (atomicMax on the sweep's word: order-independent, so results are run-to-run identical), and the workgroups of sweep s leave at once when
// sweep s - 1 recorded a maximum below the stop threshold (then every later sweep leaves too: its own word stays zero).
#include <hip/hip_runtime.h>
#include "omc_device.h"
#include "omc_wave.h"

typedef double double4m __attribute__((ext_vector_type(4)));

// the thresholds of the clip and certificate sequence (MwRound carries them; the plain sequence passes MW_TAU_PLAIN squared for both)
#define MW_TAU2 1e-20      // rotation threshold 1e-10 on the relative cross product, as k_cone_ws: a pair below it is left alone
#define MW_STOP2 1e-18     // stop rule: a sweep whose largest relative cross product was below 1e-9 is the last one.  Inside a cluster of
                           // eigenvalues a rotation angle is not small however small the cross product, so the last sweep can leave cross
                           // products of the order of the largest it met: 1e-7 left 1.2e-8 at order 2000, 1e-5 (what k_cone_ws's `big` test
                           // amounts to) 4.6e-6 ||M|| in the projection
#define MW_LDW 65          // leading dimension of the Jacobi work array: 32 rows of the Gram matrix, 32 of the accumulated rotation, odd

// the slot filter of k_cone_ws, from the fields it reads
// plain = CONE_SEP or CONE_TOPK: the filter of k_cone in that mode instead (harvested slots; no separation where k_cone_sub<2> has delivered it)
struct MwFilter { const int *slot_list, *done, *ws_first, *cone_done, *confirm; int sub_enable, ws_mode, ws_phase, cert_enable; int plain; const int *fin, *sep_done; };
static MwFilter mw_filter(const OmcWS* w) { return {w->slot_list, w->done, w->ws_first, w->cone_done, w->confirm, w->sub_enable, w->ws_mode, w->ws_phase, w->cert_enable, 0, nullptr, nullptr}; }
static MwFilter mw_plain_filter(const OmcWS* w, int mode) { MwFilter f = {}; f.slot_list = w->slot_list; f.plain = mode; f.fin = w->fin; f.sep_done = w->sep_done; return f; }
__device__ __forceinline__ int mw_slot(const MwFilter& f, int i) {      // slot of this workgroup, -1: nothing to do for it
  const int b = f.slot_list ? f.slot_list[i] : i;
  if (f.plain) return (!f.fin[b] || (f.plain == CONE_SEP && f.sep_done && f.sep_done[b])) ? -1 : b;
  if (f.done[b]) return -1;
  if (!f.ws_mode && f.sub_enable) {
    if (f.ws_phase == 1) { if (!f.ws_first[b]) return -1; }
    else if (f.cone_done[b]) return -1;
  }
  if (f.ws_mode && f.cert_enable && !f.confirm[b]) return -1;
  return b;
}
// sigma of k_cone_ws; a zero matrix takes 1 (any positive shift projects it exactly, 1e-300 would underflow in the squared norms)
__device__ __forceinline__ double mw_sigma(double fro2) { return fro2 > 0.0 ? 1.5 * sqrt(fro2) + 1e-300 : 1.0; }
__device__ __forceinline__ double mw_word(unsigned long long v) { return __longlong_as_double((long long)v); }

// ---- prepare -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mw_prepare(OmcWS w, MwFilter f) {
  const int b = mw_slot(f, blockIdx.y);
  if (b < 0) return;
  const int N = w.n, NP = w.np16, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const MwLayout L = w.geo.mwl;
  double* Gm = w.cone_scratch + (size_t)b * w.geo.ws.slab_stride;
  const int evals_only = w.ws_mode;
  const double* Mb = (evals_only ? w.MbufC : w.Mbuf) + (size_t)b * NP * NP;
  const double* Vr = (evals_only ? w.VrowC : w.Vrow) + (size_t)b * NP * NP;
  const int warm = (evals_only ? w.vvalidC : w.vvalid)[b];
  const double sigma = mw_sigma(evals_only ? w.fro2c[b] : w.fro2[b]);
  if (blockIdx.x == 0 && tid < MW_MAXSW) ((unsigned long long*)(Gm + L.smax))[tid] = 0ull;
  const int nti = NP >> 4, ntj = L.Ncp >> 4;
  const int tile = blockIdx.x * 4 + wv;
  if (tile >= nti * ntj) return;
  const int ti = tile % nti, tj = tile / nti, i0 = ti << 4, j0 = tj << 4;
  const int li = lane & 15, lk = lane >> 4, jb = j0 + li;
  double4m acc = {0.0, 0.0, 0.0, 0.0};
  if (j0 < NP) {
    if (!warm) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { const int row = i0 + lk + 4 * r; acc[r] = Mb[(size_t)jb * NP + row] + ((row == jb) ? sigma : 0.0); }
    } else {
      // the K loop of k_cone_ws: depth-PF pipeline without conditionals, K over the whole zero-padded NP, the prefetch index wraps
      constexpr int PF = 4;
      const int ia = i0 + li;
      const double* Ma = Mb + ia;
      const double* Vb = Vr + jb;
      double aq[PF], bq[PF];
#pragma unroll
      for (int u = 0; u < PF; ++u) { const int kk = 4 * u + lk; aq[u] = Ma[(size_t)kk * NP]; bq[u] = Vb[(size_t)kk * NP]; }
      for (int k0 = 0; k0 < NP; k0 += 4 * PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
          const double a = aq[u] + ((ia == k0 + 4 * u + lk) ? sigma : 0.0), bv = bq[u];
          int kn = k0 + 4 * (PF + u) + lk;
          kn = (kn < NP) ? kn : kn - NP;
          aq[u] = Ma[(size_t)kn * NP];
          bq[u] = Vb[(size_t)kn * NP];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc, 0, 0, 0);
        }
      }
    }
  }
  // the whole tile is stored: rows and columns beyond N are the zero padding the round kernels rely on
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int row = i0 + lk + 4 * r; Gm[(size_t)jb * L.ld + row] = (row < N && jb < N) ? acc[r] : 0.0; }
}

// ---- round -------------------------------------------------------------------------------------------------------------------------------
// tau2, stop2: rotation threshold and stop rule, squared.  unit_q (the plain sequence, whose eigenvalues ||g|| - sigma are compared at the level of
// the cold kernel's error): a column meets 31 rotations per inner sweep, several inner sweeps per round and nb - 1 rounds per outer sweep, some ten
// times what the cold kernel's sweep applies to it, and c^2 + s^2 - 1 of every one of them stays in its norm: with Q applied as accumulated the
// eigenvalues come out 7 - 10 e_ref off at every order from 145 to 1040 (e_ref: tests/test_plain_multi.py), with its columns scaled to unit length
// first 0.25 e_ref.  (c by division instead of rsqrt, alone, leaves 5 e_ref and adds nothing to the scaling.)  The clip sequence applies Q as it
// is: its results stay what they were bit for bit.
struct MwRound { MwFilter f; double* slab; size_t stride, smax; int ld, NP, nb; double tau2, stop2; int unit_q; };

__global__ void __launch_bounds__(256) k_mw_round(MwRound a, int sweep, int round) {
  __shared__ double s_part[4][3][256];      // Gram partials of the four waves (each sums a quarter of the rows)
  __shared__ double s_W[32 * MW_LDW];
  __shared__ double s_nrm[32], s_red[4];
  const int b = mw_slot(a.f, blockIdx.y);
  if (b < 0) return;
  double* Gm = a.slab + (size_t)b * a.stride;
  unsigned long long* smax = (unsigned long long*)(Gm + a.smax);
  if (sweep > 0 && mw_word(smax[sweep - 1]) < a.stop2) return;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4, ld = a.ld;
  int bp, bq;
  rr_pair(round, blockIdx.x, a.nb, bp, bq);
  auto col = [&](int c) { return (c < MW_B) ? bp * MW_B + c : bq * MW_B + (c - MW_B); };
  // ---- Gram matrix C = panel' panel: tiles (p,p), (q,p), (q,q); a lane feeds rows 4 lk .. 4 lk + 3 of a 16-row step to four MFMAs -----------
  {
    double4m c00 = {0.0, 0.0, 0.0, 0.0}, c10 = c00, c11 = c00;
    const double* gp = Gm + (size_t)col(li) * ld + 4 * lk;
    const double* gq = Gm + (size_t)col(MW_B + li) * ld + 4 * lk;
    for (int r0 = wv * 16; r0 < a.NP; r0 += 64) {
      const double4m x = *(const double4m*)(gp + r0), y = *(const double4m*)(gq + r0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u], x[u], c00, 0, 0, 0);
        c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(y[u], x[u], c10, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(y[u], y[u], c11, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { s_part[wv][0][r * 64 + lane] = c00[r]; s_part[wv][1][r * 64 + lane] = c10[r]; s_part[wv][2][r * 64 + lane] = c11[r]; }
  }
  __syncthreads();
  for (int e = tid; e < 3 * 256; e += 256) {
    const int t = e >> 8, rem = e & 255, r = rem >> 6, l = rem & 63, i = (l >> 4) + 4 * r, j = l & 15;
    const double v = ((s_part[0][t][rem] + s_part[1][t][rem]) + s_part[2][t][rem]) + s_part[3][t][rem];
    if (t == 0) s_W[j * MW_LDW + i] = v;
    else if (t == 2) s_W[(16 + j) * MW_LDW + 16 + i] = v;
    else { s_W[j * MW_LDW + 16 + i] = v; s_W[(16 + i) * MW_LDW + j] = v; }
  }
  __syncthreads();
  // ---- largest squared relative cross product of the pair, before any rotation ----------------------------------------------------------------
  double mx = 0.0;
  for (int e = tid; e < 32 * 32; e += 256) {
    const int i = e & 31, j = e >> 5;
    if (i > j) {
      const double g = s_W[j * MW_LDW + i], ab = s_W[i * MW_LDW + i] * s_W[j * MW_LDW + j];
      if (ab > 0.0) mx = fmax(mx, g * g / ab);
    }
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, WAVE));
  if (lane == 0) s_red[wv] = mx;
  __syncthreads();
  mx = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
  if (tid == 0) atomicMax(&smax[sweep], (unsigned long long)__double_as_longlong(mx));
  if (!(mx > a.tau2)) return;      // already diagonal to the rotation threshold: no write-back
  // ---- eigenvectors of C: one-sided Jacobi on the columns of [C; I] (rows 32 .. 63 accumulate Q), 16 pairs x 16 lanes, the sweep of
  // jacobi_sweeps_t (cached squared norms, fp64 tangent) with jacobi16_fast's ending: a sweep without a relative cross product above
  // 1e-7 leaves them below 1e-14 ---------------------------------------------------------------------------------------------------------------
  for (int e = tid; e < 32 * 32; e += 256) { const int i = e & 31, j = e >> 5; s_W[j * MW_LDW + 32 + i] = (i == j) ? 1.0 : 0.0; }
  __syncthreads();
  {
    const int grp = tid >> 4, lg = tid & 15;
    const double tau = 1e-14, tau2 = tau * tau;
    for (int sw = 0; sw < 16; ++sw) {
      if (tid < 32) { double s = 0.0; for (int r = 0; r < 32; ++r) { const double x = s_W[tid * MW_LDW + r]; s += x * x; } s_nrm[tid] = s; }
      __syncthreads();
      int big = 0;
      for (int step = 0; step < 31; ++step) {
        int p, q;
        rr_pair(step, grp, 32, p, q);
        double* wp = s_W + p * MW_LDW; double* wq = s_W + q * MW_LDW;
        const double x0 = wp[lg], x1 = wp[lg + 16], x2 = wp[lg + 32], x3 = wp[lg + 48];
        const double y0 = wq[lg], y1 = wq[lg + 16], y2 = wq[lg + 32], y3 = wq[lg + 48];
        const double gm = group_sum_dpp<16>(x0 * y0 + x1 * y1);
        const double na = s_nrm[p], nb = s_nrm[q], g2 = gm * gm, ab = na * nb;
        if (g2 > tau2 * ab && ab > 0.0) {
          const double zeta = (nb - na) / (2.0 * gm), az = fabs(zeta);
          double tt = 1.0 / (az + sqrt(1.0 + az * az));
          tt = (zeta >= 0.0) ? tt : -tt;
          const double cs = rsqrt(1.0 + tt * tt), sn = cs * tt;
          wp[lg] = cs * x0 - sn * y0; wq[lg] = sn * x0 + cs * y0;
          wp[lg + 16] = cs * x1 - sn * y1; wq[lg + 16] = sn * x1 + cs * y1;
          wp[lg + 32] = cs * x2 - sn * y2; wq[lg + 32] = sn * x2 + cs * y2;
          wp[lg + 48] = cs * x3 - sn * y3; wq[lg + 48] = sn * x3 + cs * y3;
          if (lg == 0) { s_nrm[p] = na - tt * gm; s_nrm[q] = nb + tt * gm; }
          if (g2 > tau * ab) big = 1;
        }
        __syncthreads();
      }
      if (!__syncthreads_or(big)) break;
    }
  }
  if (a.unit_q) {      // unit columns of Q (the barrier above ended the sweeps)
    if (tid < 32) {
      double* q = s_W + tid * MW_LDW + 32;
      double s = 0.0;
      for (int r = 0; r < 32; ++r) s += q[r] * q[r];
      const double sc = 1.0 / sqrt(s);
      for (int r = 0; r < 32; ++r) q[r] *= sc;
    }
    __syncthreads();
  }
  // ---- panel <- panel Q, transposed so that loads and stores run along the rows: out'[j][i] = sum_k Q[k][j] panel[i][k] ------------------------
  double qa[2][8];
#pragma unroll
  for (int jb = 0; jb < 2; ++jb)
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) qa[jb][kk] = s_W[(16 * jb + li) * MW_LDW + 32 + 4 * kk + lk];
  for (int r0 = wv * 16; r0 < a.NP; r0 += 64) {      // a wave owns its 16 rows: all 32 columns are read before any is written
    double pv[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) pv[kk] = Gm[(size_t)col(4 * kk + lk) * ld + r0 + li];
    double4m o0 = {0.0, 0.0, 0.0, 0.0}, o1 = o0;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      o0 = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[0][kk], pv[kk], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[1][kk], pv[kk], o1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Gm[(size_t)col(lk + 4 * r) * ld + r0 + li] = o0[r];
      Gm[(size_t)col(16 + lk + 4 * r) * ld + r0 + li] = o1[r];
    }
  }
}

// ---- norms: squared column norms, eigenvalues, the eigenvectors for the next call ----------------------------------------------------------
__global__ void __launch_bounds__(256) k_mw_norms(OmcWS w, MwFilter f) {
  __shared__ double s_ev[16];
  const int b = mw_slot(f, blockIdx.y);
  if (b < 0) return;
  const int N = w.n, NP = w.np16, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const MwLayout L = w.geo.mwl;
  double* Gm = w.cone_scratch + (size_t)b * w.geo.ws.slab_stride;
  const int evals_only = w.ws_mode;
  double* Vr = (evals_only ? w.VrowC : w.Vrow) + (size_t)b * NP * NP;
  const double sigma = mw_sigma(evals_only ? w.fro2c[b] : w.fro2[b]);
  const int t0 = blockIdx.x * 16;
  for (int q = 0; q < 4; ++q) {
    const int t = t0 + 4 * wv + q;
    double s = 0.0;
    for (int r = lane; r < NP; r += WAVE) { const double x = Gm[(size_t)t * L.ld + r]; s += x * x; }
    s = wave_sum(s);
    if (lane == 0) {
      s_ev[4 * wv + q] = s; Gm[L.ev + t] = s;
      const double lam = sqrt(s) - sigma;
      Gm[L.lam + t] = lam;
      if (w.ev_out && t < N) w.ev_out[(size_t)b * NP + t] = lam;
    }
  }
  __syncthreads();
  for (int e = tid; e < 16 * N; e += 256) {
    const int tl = e & 15, kk = e >> 4, t = t0 + tl;
    if (t < N) Vr[(size_t)kk * NP + t] = Gm[(size_t)t * L.ld + kk] * rsqrt(s_ev[tl]);
  }
}

// ---- select: steps 3 - 4 of k_cone_ws after the norms, and its ws_mode = 1 branch -------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_mw_select(OmcWS w, MwFilter f) {
  __shared__ int s_nkeep, s_top[SUBP];
  const int b = mw_slot(f, blockIdx.x);
  if (b < 0) return;
  const int N = w.n, NP = w.np16, tid = threadIdx.x, T = blockDim.x;
  const MwLayout L = w.geo.mwl;
  double* Gm = w.cone_scratch + (size_t)b * w.geo.ws.slab_stride;
  const double* ev = Gm + L.ev; const double* lam = Gm + L.lam;
  double* wgt = Gm + L.wgt; int* sel = (int*)(Gm + L.sel);
  const int evals_only = w.ws_mode;
  if (tid == 0) {
    (evals_only ? w.vvalidC : w.vvalid)[b] = 1;
    // sweeps that ran: sweep s ran when sweep s - 1 recorded a maximum at or above the stop threshold
    const unsigned long long* smax = (const unsigned long long*)(Gm + L.smax);
    int sweeps = 1;
    while (sweeps < w.mw_budget && mw_word(smax[sweeps - 1]) >= MW_STOP2) ++sweeps;
    const int exhausted = sweeps == w.mw_budget && mw_word(smax[sweeps - 1]) >= MW_STOP2;
    w.sweeps[b] += sweeps;
    int* st = w.mw_stat + 4 * b;
    st[0] += 1; st[1] = sweeps; st[2] += exhausted; if (sweeps > st[3]) st[3] = sweeps;
  }
  if (evals_only) {
    if (w.cert_enable && N >= 3 * SUBP) {     // seed the certificate block with the SUBP most negative eigenpairs (largest of -Mchk)
      if (tid == 0) {
        for (int j = 0; j < SUBP; ++j) {
          int bi = -1; double bl = 1e300;
          for (int t = 0; t < N; ++t) {
            bool used = false;
            for (int q = 0; q < j; ++q) if (s_top[q] == t) used = true;
            if (!used && lam[t] < bl) { bl = lam[t]; bi = t; }
          }
          s_top[j] = bi;
          w.sub_thetaC[(size_t)b * SUBP + j] = -bl;
        }
        w.sub_onC[b] = 1;
      }
      __syncthreads();
      double* Xg = w.XsC + (size_t)b * NP * SUBP;
      for (int e = tid; e < SUBP * NP; e += T) {
        const int j = e / NP, r = e - j * NP;
        Xg[e] = (r < N) ? Gm[(size_t)s_top[j] * L.ld + r] * rsqrt(ev[s_top[j]]) : 0.0;
      }
    }
    if (tid == 0) {
      const int k = w.k;
      double best[8]; const int kk2 = (k < 8) ? k : 8;
      for (int i = 0; i < kk2; ++i) best[i] = 1e300;
      for (int t = 0; t < N; ++t) {
        double lamv = lam[t];
        for (int i = 0; i < kk2; ++i) if (lamv < best[i]) { const double tmp = best[i]; best[i] = lamv; lamv = tmp; }
      }
      double s2 = 0.0;
      for (int i = 0; i < kk2; ++i) s2 += fmin(best[i], 0.0);
      w.evsum[b] = s2;
    }
    return;
  }
  const double hi = w.clip_hi;
  if (tid == 0) {
    int ndef = 0, nkeep = 0;
    for (int t = 0; t < N; ++t) {
      const double lamv = lam[t];
      if (lamv < 0.0 || lamv > hi) ++ndef;
      if (lamv > 0.0) ++nkeep;
    }
    s_nkeep = nkeep;
    int c = 0;
    if (ndef <= nkeep) {
      for (int t = 0; t < N; ++t) {
        const double lamv = lam[t];
        if (lamv < 0.0) { sel[c] = t; wgt[c] = -lamv / ev[t]; ++c; }
        else if (lamv > hi) { sel[c] = t; wgt[c] = -(lamv - hi) / ev[t]; ++c; }
      }
      Gm[L.head] = 1.0;
    } else {
      for (int t = 0; t < N; ++t) {
        const double lamv = lam[t];
        if (lamv > 0.0) { sel[c] = t; wgt[c] = fmin(lamv, hi) / ev[t]; ++c; }      // weight / nu^2
      }
      Gm[L.head] = 0.0;
    }
    ((int*)(Gm + L.head + 1))[0] = c; ((int*)(Gm + L.head + 1))[1] = nkeep;
  }
  __syncthreads();
  if (w.sub_enable) {      // seed the tracked subspace (k_cone_sub) with the SUBP dominant eigenvectors when few eigenvalues are positive
    const bool seed = s_nkeep <= SUBP - w.sub_guard && N >= 3 * SUBP;
    if (seed) {
      for (int t = tid; t < N; t += T) {
        const double lt = lam[t];
        int rk = 0;
        for (int u = 0; u < N; ++u) { const double lu = lam[u]; rk += (lu > lt || (lu == lt && u < t)) ? 1 : 0; }
        if (rk < SUBP) { s_top[rk] = t; w.sub_theta[(size_t)b * SUBP + rk] = lt; }
      }
      __syncthreads();
      double* Xg = w.Xs + (size_t)b * NP * SUBP;
      for (int e = tid; e < SUBP * NP; e += T) {
        const int j = e / NP, r = e - j * NP;
        Xg[e] = (r < N) ? Gm[(size_t)s_top[j] * L.ld + r] * rsqrt(ev[s_top[j]]) : 0.0;
      }
      if (tid == 0) atomicAdd(&w.sub_stat[8 * b + 3], 1);
    }
    if (tid == 0) w.sub_on[b] = seed ? 1 : 0;
  }
}

// ---- rebuild: the two cases of spectral_rebuild as a rank-c MFMA update, one wave per 16 x 16 tile of the lower triangle ------------------------
__global__ void __launch_bounds__(256) k_mw_rebuild(OmcWS w, MwFilter f) {
  const int b = mw_slot(f, blockIdx.y);
  if (b < 0) return;
  const int N = w.n, NP = w.np16, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const MwLayout L = w.geo.mwl;
  const double* Gm = w.cone_scratch + (size_t)b * w.geo.ws.slab_stride;
  const double* wgt = Gm + L.wgt; const int* sel = (const int*)(Gm + L.sel);
  const double base = Gm[L.head];
  int nsel = ((const int*)(Gm + L.head + 1))[0];
  nsel = nsel < N ? nsel : N;
  if (blockIdx.x == 0 && tid == 0 && w.ws_phase == 1) w.cone_done[b] = 1;      // read by later launches only
  const int nt = NP >> 4, tile = blockIdx.x * 4 + wv;
  if (tile >= nt * (nt + 1) / 2) return;
  int ti = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > tile) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  const int tj = tile - ti * (ti + 1) / 2, i0 = ti << 4, j0 = tj << 4;
  double4m acc = {0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < nsel; s0 += 4) {      // selected columns in ascending order, four per MFMA (rows beyond N are zero in G)
    const int s = s0 + lk;
    double x = 0.0, y = 0.0;
    if (s < nsel) { const double* g = Gm + (size_t)sel[s] * L.ld; x = g[i0 + li]; y = g[j0 + li] * wgt[s]; }
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
  }
  const double* Mb = w.Mbuf + (size_t)b * NP * NP;
  double* Wout = w.W1 + (size_t)b * N * N;
  const int j = j0 + li;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + lk + 4 * r;
    if (i < N && j < N && i >= j) {
      const double v = (base != 0.0 ? base * Mb[(size_t)j * NP + i] : 0.0) + acc[r];
      Wout[(size_t)j * N + i] = v; Wout[(size_t)i * N + j] = v;
    }
  }
}

extern "C" void omc_launch_cone_mw(const OmcWS* w, hipStream_t s) {
  const MwLayout L = w->geo.mwl;
  const MwFilter f = mw_filter(w);
  const int nti = w->np16 >> 4, ntj = L.Ncp >> 4, nlow = nti * (nti + 1) / 2;
  const int budget = w->mw_budget < 1 ? 1 : (w->mw_budget > MW_MAXSW ? MW_MAXSW : w->mw_budget);
  OmcWS wq = *w; wq.mw_budget = budget;
  hipLaunchKernelGGL(k_mw_prepare, dim3((nti * ntj + 3) / 4, w->nB), dim3(256), 0, s, wq, f);
  const MwRound a = {f, w->cone_scratch, w->geo.ws.slab_stride, L.smax, L.ld, w->np16, L.nb, MW_TAU2, MW_STOP2, 0};
  for (int sw = 0; sw < budget; ++sw)
    for (int r = 0; r < L.nb - 1; ++r) hipLaunchKernelGGL(k_mw_round, dim3(L.nb / 2, w->nB), dim3(256), 0, s, a, sw, r);
  hipLaunchKernelGGL(k_mw_norms, dim3(L.Ncp / 16, w->nB), dim3(256), 0, s, wq, f);
  hipLaunchKernelGGL(k_mw_select, dim3(w->nB), dim3(1024), 0, s, wq, f);
  if (!w->ws_mode) hipLaunchKernelGGL(k_mw_rebuild, dim3((nlow + 3) / 4, w->nB), dim3(256), 0, s, wq, f);
}

// ---- the plain operations: CONE_SEP and CONE_TOPK of k_cone (omc_device.hip) on the round kernel, always cold ----------------------------------
// They read (Y, U) and write the slab, lmin / bx or U and pmw_stat: nothing of the warm-started projection (Vrow, vvalid, Mbuf, fro2, sweeps,
// mw_stat), so a harvest may run behind k_state_save and beside the next interval of the live slots.
// entry (i, j) of the input as eig_frontend forms it, 1/2 (entry(i, j) + entry(j, i)) of cone_M_entry: U U' - Y (ui = row i of U), or Y
__device__ __forceinline__ double mw_plain_entry(const double* Y, const double* Ub, const double* ui, int n, int k, int i, int j) {
  const double yij = Y[(size_t)j * n + i], yji = Y[(size_t)i * n + j];
  if (!Ub) return 0.5 * (yij + yji);
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < 8; ++t) if (t < k) s += ui[t] * Ub[(size_t)t * n + j];      // k <= 8; unrolled: ui stays in registers
  return 0.5 * ((s - yij) + (s - yji));
}
// ||M||_F^2 from the partial sums of the row tiles, in one order whichever wave forms it: a lane's stride, then the sum over the wave
__device__ __forceinline__ double mw_plain_fro2(const double* part, int nt, int lane) {
  double s = 0.0;
  for (int t = lane; t < nt; t += WAVE) s += part[t];
  return wave_sum(s);
}

__global__ void __launch_bounds__(256) k_mw_plain_fro(OmcWS w, MwFilter f) {
  __shared__ double s_red[4];
  const int b = mw_slot(f, blockIdx.y);
  if (b < 0) return;
  const int n = w.n, k = w.k, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const MwLayout L = w.geo.mwl;
  double* Gm = w.cone_scratch + (size_t)b * w.geo.ws.slab_stride;
  const double* Y = w.Y + (size_t)b * n * n;
  const double* Ub = (f.plain == CONE_SEP) ? w.U + (size_t)b * n * k : nullptr;
  const int i = blockIdx.x * 16 + (tid & 15);
  double ui[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < 8; ++t) if (Ub && i < n && t < k) ui[t] = Ub[(size_t)t * n + i];
  double acc = 0.0;
  if (i < n)
    for (int j = tid >> 4; j < n; j += 16) { const double v = mw_plain_entry(Y, Ub, ui, n, k, i, j); acc += v * v; }
  acc = wave_sum(acc);
  if (lane == 0) s_red[wv] = acc;
  __syncthreads();
  if (tid == 0) Gm[L.fro + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ void __launch_bounds__(256) k_mw_plain_prepare(OmcWS w, MwFilter f) {
  const int b = mw_slot(f, blockIdx.y);
  if (b < 0) return;
  const int n = w.n, k = w.k, NP = w.np16, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const MwLayout L = w.geo.mwl;
  double* Gm = w.cone_scratch + (size_t)b * w.geo.ws.slab_stride;
  if (blockIdx.x == 0 && tid < MW_MAXSW) ((unsigned long long*)(Gm + L.smax))[tid] = 0ull;
  const int nti = NP >> 4, ntj = L.Ncp >> 4;
  const int tile = blockIdx.x * 4 + wv;
  if (tile >= nti * ntj) return;
  const double sigma = mw_sigma(mw_plain_fro2(Gm + L.fro, nti, lane));
  const double* Y = w.Y + (size_t)b * n * n;
  const double* Ub = (f.plain == CONE_SEP) ? w.U + (size_t)b * n * k : nullptr;
  const int ti = tile % nti, tj = tile / nti, i = (ti << 4) + (lane & 15);
  double ui[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < 8; ++t) if (Ub && i < n && t < k) ui[t] = Ub[(size_t)t * n + i];
  // the whole tile is stored (16 rows of a column per quarter wave): rows beyond N up to NP and columns up to Ncp are the zero padding
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = (tj << 4) + (lane >> 4) + 4 * r;
    double v = 0.0;
    if (i < n && j < n) v = mw_plain_entry(Y, Ub, ui, n, k, i, j) + ((i == j) ? sigma : 0.0);
    Gm[(size_t)j * L.ld + i] = v;
  }
}

__global__ void __launch_bounds__(256) k_mw_plain_norms(OmcWS w, MwFilter f) {
  const int b = mw_slot(f, blockIdx.y);
  if (b < 0) return;
  const int NP = w.np16, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const MwLayout L = w.geo.mwl;
  double* Gm = w.cone_scratch + (size_t)b * w.geo.ws.slab_stride;
  const double sigma = mw_sigma(mw_plain_fro2(Gm + L.fro, NP >> 4, lane));
  for (int q = 0; q < 4; ++q) {
    const int t = blockIdx.x * 16 + 4 * wv + q;
    double s = 0.0;
    for (int r = lane; r < NP; r += WAVE) { const double x = Gm[(size_t)t * L.ld + r]; s += x * x; }
    s = wave_sum(s);
    if (lane == 0) { Gm[L.ev + t] = s; Gm[L.lam + t] = sqrt(s) - sigma; }
  }
}

// the larger value, the lower index among equal ones (what a strict comparison over ascending indices keeps); i < 0: no candidate
__device__ __forceinline__ void mw_take(double& v, int& i, double ov, int oi) {
  if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
}
__device__ __forceinline__ int mw_block_argmax(double v, int i, double* s_rv, int* s_ri) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int o = 32; o > 0; o >>= 1) { const double ov = __shfl_xor(v, o, WAVE); const int oi = __shfl_xor(i, o, WAVE); mw_take(v, i, ov, oi); }
  __syncthreads();      // the words of the previous call have been read
  if (lane == 0) { s_rv[wv] = v; s_ri[wv] = i; }
  __syncthreads();
  v = s_rv[0]; i = s_ri[0];
  for (int q = 1; q < 4; ++q) mw_take(v, i, s_rv[q], s_ri[q]);
  return i;
}
// column c of G: 1 / ||g_c|| with the canonical sign (the first entry of largest magnitude is positive)
__device__ __forceinline__ double mw_column_scale(const double* g, double ev, int N, double* s_rv, int* s_ri) {
  double v = 0.0; int i = -1;
  for (int r = threadIdx.x; r < N; r += 256) mw_take(v, i, fabs(g[r]), r);
  i = mw_block_argmax(v, i, s_rv, s_ri);
  return ((g[i] >= 0.0) ? 1.0 : -1.0) / sqrt(ev);
}

__global__ void __launch_bounds__(256) k_mw_plain_pick(OmcWS w, MwFilter f) {
  __shared__ double s_rv[4], s_sg[8], s_wt[2];
  __shared__ int s_ri[4], s_top[8];
  const int b = mw_slot(f, blockIdx.x);
  if (b < 0) return;
  const int N = w.n, k = w.k, tid = threadIdx.x;
  const MwLayout L = w.geo.mwl;
  const double* Gm = w.cone_scratch + (size_t)b * w.geo.ws.slab_stride;
  const double* ev = Gm + L.ev; const double* lam = Gm + L.lam;
  if (tid == 0 && w.pmw_stat) {      // sweeps that ran, as k_mw_select counts them
    const unsigned long long* smax = (const unsigned long long*)(Gm + L.smax);
    const double stop2 = MW_TAU_PLAIN * MW_TAU_PLAIN;
    int sweeps = 1;
    while (sweeps < MW_PLAIN_SWEEPS && mw_word(smax[sweeps - 1]) >= stop2) ++sweeps;
    const int exhausted = sweeps == MW_PLAIN_SWEEPS && mw_word(smax[sweeps - 1]) >= stop2;
    int* st = w.pmw_stat + 4 * b;
    st[0] += 1; st[1] = sweeps; st[2] += exhausted; if (sweeps > st[3]) st[3] = sweeps;
  }
  const int sep = f.plain == CONE_SEP, npick = sep ? 2 : (k < 8 ? k : 8);
  for (int j = 0; j < npick; ++j) {      // the two smallest / the k largest eigenvalues, one after the other; ties go to the lowest column
    double v = 0.0; int i = -1;
    for (int t = tid; t < N; t += 256) {
      bool used = false;
      for (int q = 0; q < j; ++q) used = used || s_top[q] == t;
      if (!used) mw_take(v, i, sep ? -lam[t] : lam[t], t);
    }
    i = mw_block_argmax(v, i, s_rv, s_ri);
    const double sg = mw_column_scale(Gm + (size_t)i * L.ld, ev[i], N, s_rv, s_ri);
    if (tid == 0) { s_top[j] = i; s_sg[j] = sg; }
    __syncthreads();
  }
  if (sep) {
    const double l1 = lam[s_top[0]], l2 = lam[s_top[1]];
    if (tid == 0) {
      w.lmin[2 * b] = l1; w.lmin[2 * b + 1] = l2;
      if (w.breakpoints == 2 && l2 < -1e-10) {       // OMC.jl:2471-2473
        const double nn = sqrt(l1 * l1 + l2 * l2);
        s_wt[0] = fabs(l1) / nn; s_wt[1] = fabs(l2) / nn;
      } else { s_wt[0] = 1.0; s_wt[1] = 0.0; }
    }
    __syncthreads();
    const double* g1 = Gm + (size_t)s_top[0] * L.ld; const double* g2 = Gm + (size_t)s_top[1] * L.ld;
    for (int r = tid; r < N; r += 256) w.bx[(size_t)b * N + r] = s_wt[0] * s_sg[0] * g1[r] + s_wt[1] * s_sg[1] * g2[r];
    return;
  }
  for (int e = tid; e < N * npick; e += 256) {
    const int j = e / N, r = e - j * N;
    w.U[(size_t)b * N * k + e] = s_sg[j] * Gm[(size_t)s_top[j] * L.ld + r];
  }
}

extern "C" void omc_launch_cone_plain_mw(const OmcWS* w, int mode, hipStream_t s) {
  const MwLayout L = w->geo.mwl;
  const MwFilter f = mw_plain_filter(w, mode);
  const int nti = w->np16 >> 4, ntj = L.Ncp >> 4;
  hipLaunchKernelGGL(k_mw_plain_fro, dim3(nti, w->nB), dim3(256), 0, s, *w, f);
  hipLaunchKernelGGL(k_mw_plain_prepare, dim3((nti * ntj + 3) / 4, w->nB), dim3(256), 0, s, *w, f);
  const double tau2 = MW_TAU_PLAIN * MW_TAU_PLAIN;
  const MwRound a = {f, w->cone_scratch, w->geo.ws.slab_stride, L.smax, L.ld, w->np16, L.nb, tau2, tau2, 1};
  for (int sw = 0; sw < MW_PLAIN_SWEEPS; ++sw)
    for (int r = 0; r < L.nb - 1; ++r) hipLaunchKernelGGL(k_mw_round, dim3(L.nb / 2, w->nB), dim3(256), 0, s, a, sw, r);
  hipLaunchKernelGGL(k_mw_plain_norms, dim3(L.Ncp / 16, w->nB), dim3(256), 0, s, *w, f);
  hipLaunchKernelGGL(k_mw_plain_pick, dim3(w->nB), dim3(256), 0, s, *w, f);
}
