// omc_shor_cert.hip -- CDNA4 (gfx950) kernels of omc_shor_dual_bound_batch: the Lagrangian bound of a Shor-mode node (rank 1) from multipliers
// the caller supplies (certificate.evaluate_shor / shor_dual_bound restated for the device).
//
//   k_scert_clean   one LANE per minor of every evaluated node: Jacobi in registers, smallest eigenvalue of the block as given (a defect), and with
//                   `store` the block minus its negative part into GamC (way 1 of sanitise = 1)
//   k_scert_keys    one thread per V1 / V2 key of every view: mean of the entries that multiply the key over the blocks that share it
//   k_scert_minor   one LANE per minor of every view: Gamma' = Gamma - E + ||E||_F I + max(0, -lambda_min) I; Gamma'[0,0] as a per-block
//                   partial sum, Gamma'[0,p] and Gamma'[p,p] into an 8-plane SoA scratch, the largest residual as a per-block partial
//   k_scert_cols    one WORKGROUP per (view, column): zmin, zeta, mu, phi, the column of phi sqrt(2 / (gamma mu)) in the dense n x m buffer
//                   from which k_dual_assemble forms M by the MFMA product, the column constants, the mu <= 0 rule
// No atomics; every sum has a fixed order (lane-strided partials, wave butterfly, waves in order, blocks in order), and a view reads nothing
// that belongs to another view, so a node's result does not depend on the batch around it.  The per-minor planes are SoA [entry][minor]
// with the caller's stride: a wave touches 64 consecutive doubles per plane.  HBM-bound streaming work with an order-5 Jacobi per lane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "omc_shor_cert.h"
#include "omc_shor_block.h"
#include "omc_wave.h"

// block-wide maximum (NaN operands are dropped), valid in every thread; red holds >= 8 doubles
__device__ __forceinline__ double scert_block_max(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
  const int nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
  for (int q = 1; q < nw; ++q) v = fmax(v, red[q]);
  return v;
}

__global__ void __launch_bounds__(SCERT_T) k_scert_clean(ShorCertWS w, int store) {
  __shared__ double red[8];
  const int v = blockIdx.y;
  if (w.view_way[v]) return;                                // once per node: at its first view
  const int b = w.view_node[v];
  const ShorGroupDev G = w.groups[w.node_group[b]];
  if ((long long)blockIdx.x * SCERT_T >= G.nq) return;      // uniform: this node's list is shorter
  const int q = blockIdx.x * SCERT_T + threadIdx.x;
  double lo = INFINITY;
  if (q < G.nq) {
    const double* src = w.Gam + (size_t)b * 15 * w.nqs + q;
    double g[15];
#pragma unroll
    for (int e = 0; e < 15; ++e) g[e] = src[(size_t)e * w.nqs];
    lo = shor_block_remove_negative(g);
    if (store) {
      double* dst = w.GamC + (size_t)b * 15 * w.nqs + q;
#pragma unroll
      for (int e = 0; e < 15; ++e) dst[(size_t)e * w.nqs] = g[e];
    }
  }
  lo = -scert_block_max(-lo, red);
  if (threadIdx.x == 0) w.cleanpart[(size_t)b * w.nmb + blockIdx.x] = lo;
}

__global__ void __launch_bounds__(SCERT_T) k_scert_keys(ShorCertWS w) {
  const int v = blockIdx.y, b = w.view_node[v];
  const ShorGroupDev G = w.groups[w.node_group[b]];
  const int t = blockIdx.x * SCERT_T + threadIdx.x;
  const double* Gm = (w.view_way[v] ? w.GamC : w.Gam) + (size_t)b * 15 * w.nqs;
  if (t < G.nv1) {
    double s = 0.0; const int p0 = G.v1ptr[t], p1 = G.v1ptr[t + 1];
    for (int p = p0; p < p1; ++p) { const int ent = G.v1ent[p]; s += Gm[(size_t)((ent & 1) ? 13 : 4) * w.nqs + (ent >> 1)]; }
    w.e1[(size_t)v * w.nv1max + t] = s / (double)(p1 - p0);
  }
  if (t < G.nv2) {
    double s = 0.0; const int p0 = G.v2ptr[t], p1 = G.v2ptr[t + 1];
    for (int p = p0; p < p1; ++p) { const int ent = G.v2ent[p]; s += Gm[(size_t)((ent & 1) ? 12 : 7) * w.nqs + (ent >> 1)]; }
    w.e2[(size_t)v * w.nv2max + t] = s / (double)(p1 - p0);
  }
}

__global__ void __launch_bounds__(SCERT_T) k_scert_minor(ShorCertWS w) {
  __shared__ double red[32];
  __shared__ double redm[8];
  const int v = blockIdx.y, b = w.view_node[v];
  const ShorGroupDev G = w.groups[w.node_group[b]];
  if ((long long)blockIdx.x * SCERT_T >= G.nq) return;      // uniform
  const int q = blockIdx.x * SCERT_T + threadIdx.x;
  double g00 = 0.0, res = 0.0;
  if (q < G.nq) {
    const int nq = G.nq;
    const double* src = (w.view_way[v] ? w.GamC : w.Gam) + (size_t)b * 15 * w.nqs + q;
    double g[15];
#pragma unroll
    for (int e = 0; e < 15; ++e) g[e] = src[(size_t)e * w.nqs];
    const double e12 = w.e1[(size_t)v * w.nv1max + G.kid[q]], e34 = w.e1[(size_t)v * w.nv1max + G.kid[nq + q]];
    const double e13 = w.e2[(size_t)v * w.nv2max + G.kid[2 * nq + q]], e24 = w.e2[(size_t)v * w.nv2max + G.kid[3 * nq + q]];
    const double e3 = shor_block_e3(g);
    res = fmax(fmax(fmax(fabs(e12), fabs(e34)), fmax(fabs(e13), fabs(e24))), fabs(e3));
    shor_block_spread(g, e12, e34, e13, e24, e3);
    if (shor_block_finite(g)) shor_block_final_shift(g);
    else g[0] = NAN;                                         // anything not finite on the way: the node's bound is -inf
    g00 = g[0];
    double* r8 = w.row8 + (size_t)v * 8 * w.nqs + q;
    r8[0] = g[1]; r8[(size_t)1 * w.nqs] = g[3]; r8[(size_t)2 * w.nqs] = g[6]; r8[(size_t)3 * w.nqs] = g[10];
    r8[(size_t)4 * w.nqs] = g[2]; r8[(size_t)5 * w.nqs] = g[5]; r8[(size_t)6 * w.nqs] = g[9]; r8[(size_t)7 * w.nqs] = g[14];
  }
  g00 = block_sum(g00, red);
  res = scert_block_max(res, redm);
  if (threadIdx.x == 0) {
    double* mp = w.minpart + ((size_t)v * w.nmb + blockIdx.x) * 2;
    mp[0] = g00; mp[1] = res;
  }
}

__global__ void __launch_bounds__(SCERT_T) k_scert_cols(ShorCertWS w) {
  __shared__ double red[32];
  __shared__ double redm[8];
  const int v = blockIdx.y, j = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int b = w.view_node[v];
  const ShorGroupDev G = w.groups[w.node_group[b]];
  const int n = w.n, m = w.m;
  const size_t nm = (size_t)n * m;
  const double sc = w.scale[b];
  const double* Xb = w.Xbar + b * nm + (size_t)j * n;
  const double* xi = w.xi + b * nm + (size_t)j * n;
  const uint8_t* ecl = G.eclass + (size_t)j * n;
  const uint8_t* msk = w.mask + (size_t)j * n;
  const double* A = w.A + (size_t)j * n;
  const int* cptr = G.cptr + (size_t)j * n;
  const double* r8 = w.row8 + (size_t)v * 8 * w.nqs;
  const int ct = G.ctype[j];
  const double cT = 1.0 / (2.0 * w.gamma) + ((ct == 1) ? 0.5 : 0.0);
  // pass 1: zmin = max over C of (sum_q Gamma'[p,p] - cW), sum of xi^2, the column's constants
  double zmin = -INFINITY, sxi2 = 0.0, cst = 0.0;
  for (int i = tid; i < n; i += T) {
    const int cl = ecl[i];
    const bool ob = msk[i] != 0;
    const double a = ob ? sc * A[i] : 0.0;
    const double qX = (ob && cl == 1 && ct == 0) ? 1.0 : 0.0;
    const double x = Xb[i];
    cst += 0.5 * a * a - ((qX != 0.0) ? 0.5 * x * x : 0.0);
    if (cl == 2) {
      const double cW = (ob ? 0.5 : 0.0) - ((ct == 1) ? 0.5 : 0.0);
      double gd = 0.0;
      for (int c = cptr[i]; c < cptr[i + 1]; ++c) {
        const int ent = G.cent[c];
        gd += r8[(size_t)(4 + (ent & 3)) * w.nqs + (ent >> 2)];
      }
      zmin = fmax(zmin, gd - cW);
    } else if (cl == 1 && ct != 2) {
      sxi2 += xi[i] * xi[i];
    }
  }
  zmin = scert_block_max(zmin, redm);
  sxi2 = block_sum(sxi2, red);
  cst = block_sum(cst, red);
  double zadm = w.zeta[(size_t)b * m + j];
  bool finite = (zadm - zadm) == 0.0;
  if (w.clamp_zeta && ct != 2) zadm = fmax(zadm, 0.0);
  const double zeta = (ct == 2) ? zmin : fmax(zadm, zmin);
  const double mu = cT - zeta;
  // pass 2: phi and the dense multiplier column
  double* Lx = w.lamDX + (size_t)v * nm + (size_t)j * n;
  const bool badmu = !(mu > 0.0);
  const double scl = badmu ? 0.0 : sqrt(2.0 / (w.gamma * mu));
  double anyphi = 0.0;
  for (int i = tid; i < n; i += T) {
    const int cl = ecl[i];
    const bool ob = msk[i] != 0;
    double phi = ob ? -0.5 * sc * A[i] : 0.0;
    if (ob && cl == 1 && ct == 0) phi += 0.5 * Xb[i];
    if (cl == 1 && ct != 2) phi += zeta * xi[i];
    if (cl == 2) {
      double g0 = 0.0;
      for (int c = cptr[i]; c < cptr[i + 1]; ++c) {
        const int ent = G.cent[c];
        g0 += r8[(size_t)(ent & 3) * w.nqs + (ent >> 2)];
      }
      phi -= g0;
    }
    anyphi += fabs(phi);
    Lx[i] = phi * scl;
  }
  anyphi = block_sum(anyphi, red);
  if (tid == 0) {
    double c0 = cst - ((ct != 2) ? zeta * sxi2 : 0.0);
    if (j == 0) {                                            // constants of the order-5 blocks, added in a fixed order
      const int nblk = (G.nq + SCERT_T - 1) / SCERT_T;
      double g = 0.0;
      for (int t = 0; t < nblk; ++t) g += w.minpart[((size_t)v * w.nmb + t) * 2];
      c0 -= g;
    }
    finite = finite && (anyphi - anyphi) == 0.0 && (c0 - c0) == 0.0 && (mu - mu) == 0.0;
    w.c0col[(size_t)v * m + j] = c0;
    w.colmu[(size_t)v * m + j] = mu;
    w.colbad[(size_t)v * m + j] = !finite ? 2 : (badmu && anyphi > 0.0) ? 1 : 0;
  }
}

extern "C" {
void omc_scert_launch_clean(const ShorCertWS* w, int store, hipStream_t s) {
  if (w->nmb > 0) hipLaunchKernelGGL(k_scert_clean, dim3(w->nmb, w->V), dim3(SCERT_T), 0, s, *w, store);
}
void omc_scert_launch_keys(const ShorCertWS* w, hipStream_t s) {
  const int mx = w->nv1max > w->nv2max ? w->nv1max : w->nv2max;
  if (mx > 0) hipLaunchKernelGGL(k_scert_keys, dim3((mx + SCERT_T - 1) / SCERT_T, w->V), dim3(SCERT_T), 0, s, *w);
}
void omc_scert_launch_minor(const ShorCertWS* w, hipStream_t s) {
  if (w->nmb > 0) hipLaunchKernelGGL(k_scert_minor, dim3(w->nmb, w->V), dim3(SCERT_T), 0, s, *w);
}
void omc_scert_launch_cols(const ShorCertWS* w, hipStream_t s) { hipLaunchKernelGGL(k_scert_cols, dim3(w->m, w->V), dim3(SCERT_T), 0, s, *w); }
}
