// omc_api_plain.cpp -- the operations of the driver outside a relaxation, behind the C ABI of include/omc.h.  They mirror these call sites
// of the reference driver (OMC.jl = its src/OptimalMatrixCompletion.jl):
//   omc_evaluate_objective  <- evaluate_objective OMC.jl:2330-2359
//   omc_separation_batch    <- eigs(U U' - Y) at OMC.jl:1274 and 2466-2477
//   omc_round_Y_batch, omc_left_singular_batch <- the roundings at OMC.jl:524, 564, 921
//   omc_altmin_batch        <- alternating_minimization OMC.jl:1979-2279 (omc_altmin_plan, omc_altmin_master_objectives)
// and omc_psd_project_batch / omc_column_prox_batch, single blocks of the ADMM iteration on their own, with the plans and statistics of all
// of them (omc_colprox_plan, omc_plain_multi_plan, omc_plain_multi_tau, omc_last_plain_multi_stats, omc_last_cone_multi_stats).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>

#include "omc_api_internal.h"
#include <chrono>

#include "omc_altmin.h"

int omc_evaluate_objective(omc_instance* h, int B, const double* X, double* objective) {
  if (!h || !X || !objective) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  HIPCHK(hipSetDevice(h->device));
  const size_t n = h->n, m = h->m;
  double* dX = nullptr;
  BIND(h->bXin, dX, (size_t)B * n * m + (size_t)B + 8);      // X, the B objectives behind it, 64 spare bytes
  double* dout = dX + (size_t)B * n * m;
  HIPCHK(hipMemcpyAsync(dX, X, 8 * (size_t)B * n * m, hipMemcpyHostToDevice, h->stream));
  omc_launch_eval_objective(B, (int)n, (int)m, h->gamma, h->dA.as<double>(), h->dmask.as<uint8_t>(), dX, dout, h->stream);
  HIPCHK(hipMemcpyAsync(objective, dout, 8 * (size_t)B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// The eigen-kernel of the three plain entry points below.  Where it is the multi-workgroup sequence (geo.plain_mw, omc_launch_cone_plain_mw) two
// events take its device time and, once the caller has synchronised the stream, collect() reads the slots' counters: omc_last_plain_multi_stats
// then speaks of this call alone (all zero where the cold kernel ran).
static_assert(MW_PLAIN_SWEEPS == MAX_SWEEPS, "the plain sequence enqueues the cold kernel's sweep limit");
struct PlainCall {
  EventPair ev;
  int launch(omc_instance* h, const OmcWS& w, int mode) {
    if (w.geo.plain_mw) { HIPCHK(ev.create()); HIPCHK(hipEventRecord(ev.e0, h->stream)); }
    omc_launch_cone(&w, mode, h->stream);
    if (w.geo.plain_mw) HIPCHK(hipEventRecord(ev.e1, h->stream));
    return 0;
  }
  int collect(omc_instance* h, const OmcWS& w, int B) {
    for (int q = 0; q < 4; ++q) h->pmw_tot[q] = 0;
    if (!w.geo.plain_mw) return 0;
    std::vector<int> st(4 * (size_t)B);
    HIPCHK(hipMemcpyAsync(st.data(), w.pmw_stat, sizeof(int) * st.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int b = 0; b < B; ++b) {
      h->pmw_tot[0] += st[4 * b]; h->pmw_tot[2] += st[4 * b + 2];
      h->pmw_tot[1] = std::max<long long>(h->pmw_tot[1], st[4 * b + 3]);
    }
    float msv = 0.f; HIPCHK(hipEventElapsedTime(&msv, ev.e0, ev.e1));
    h->pmw_tot[3] = (long long)(1000.0 * msv);
    return 0;
  }
};

int omc_separation_batch(omc_instance* h, int B, int breakpoints, const double* Y, const double* U, double* eigvals,
                         double* x, int* feasible) {
  if (!h || !Y || !U) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (breakpoints != OMC_SMALLEST_1_EIGVEC && breakpoints != OMC_SMALLEST_2_EIGVEC)
    return fail(OMC_ERR_INVALID_ENUM, "Invalid input for disjunctive cuts breakpoints (OMC.jl:2440-2446)");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  // stage an empty batch to get a workspace of the right size, then overwrite (Y, U)
  std::vector<int> L(B, 0);
  omc_relax_params P = h->params; P.breakpoints = breakpoints; P.slots = B;   // identity slot map: the state arrays are addressed by node
  int rc = omc_relax_stage(h, B, &P, OMC_CUT_LINEAR, L.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc) return rc;
  const OmcWS& w = h->ws;
  const size_t n = h->n, k = h->k;
  HIPCHK(hipMemcpyAsync(w.Y, Y, 8 * (size_t)B * n * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(w.U, U, 8 * (size_t)B * n * k, hipMemcpyHostToDevice, h->stream));
  PlainCall pc;
  if ((rc = pc.launch(h, w, CONE_SEP))) return rc;
  std::vector<double> ev(2 * (size_t)B);
  HIPCHK(hipMemcpyAsync(ev.data(), w.lmin, 16 * (size_t)B, hipMemcpyDeviceToHost, h->stream));
  if (x) HIPCHK(hipMemcpyAsync(x, w.bx, 8 * (size_t)B * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  if ((rc = pc.collect(h, w, B))) return rc;
  for (int b = 0; b < B; ++b) {
    if (eigvals) { eigvals[2 * b] = ev[2 * b]; eigvals[2 * b + 1] = ev[2 * b + 1]; }
    if (feasible) feasible[b] = ev[2 * b] >= -1e-6 ? 1 : 0;   // OMC.jl:1274-1276 projection_tolerance
  }
  h->staged = false;
  return 0;
}

int omc_round_Y_batch(omc_instance* h, int B, const double* Y, double* U_rounded) {
  if (!h || !Y || !U_rounded) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  std::vector<int> L(B, 0);
  omc_relax_params P = h->params; P.slots = B;
  int rc = omc_relax_stage(h, B, &P, OMC_CUT_LINEAR, L.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc) return rc;
  const OmcWS& w = h->ws;
  const size_t n = h->n, k = h->k;
  HIPCHK(hipMemcpyAsync(w.Y, Y, 8 * (size_t)B * n * n, hipMemcpyHostToDevice, h->stream));
  PlainCall pc;
  if ((rc = pc.launch(h, w, CONE_TOPK))) return rc;
  HIPCHK(hipMemcpyAsync(U_rounded, w.U, 8 * (size_t)B * n * k, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  if ((rc = pc.collect(h, w, B))) return rc;
  h->staged = false;
  return 0;
}

// svd(X).U[:, 1:k] of B matrices X (n x m): the k dominant eigenvectors of X X' (Gram product on the matrix cores, then the eigen-kernel of
// omc_round_Y_batch); same canonical sign.  The singular values are well separated from zero for the matrices the driver rounds (products U V of
// rank k, OMC.jl:564, 921; the zero-filled A of the root, OMC.jl:524), so squaring the condition number costs nothing that matters.
int omc_left_singular_batch(omc_instance* h, int B, const double* X, double* U_out) {
  if (!h || !X || !U_out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  std::vector<int> L(B, 0);
  omc_relax_params P = h->params; P.slots = B;
  int rc = omc_relax_stage(h, B, &P, OMC_CUT_LINEAR, L.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc) return rc;
  const OmcWS& w = h->ws;
  const size_t n = h->n, m = h->m, k = h->k;
  double* dX = nullptr;
  BIND(h->bXin, dX, (size_t)B * n * m);
  HIPCHK(hipMemcpyAsync(dX, X, 8 * (size_t)B * n * m, hipMemcpyHostToDevice, h->stream));
  omc_launch_gram_XXt(&w, dX, B, h->stream);
  PlainCall pc;
  if ((rc = pc.launch(h, w, CONE_TOPK))) return rc;
  HIPCHK(hipMemcpyAsync(U_out, w.U, 8 * (size_t)B * n * k, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  if ((rc = pc.collect(h, w, B))) return rc;
  h->staged = false;
  return 0;
}

// Spectral clip of B symmetric matrices of order N by the eigen-kernels of the relaxation, on their own (OMC.jl:1554-1556 are the cones they
// serve).  A private view of the workspace (n = N, its own Mbuf / Vrow / W1 / slab) goes through omc_launch_cone_ws / omc_launch_cone: no
// second copy of a kernel.  The kernels clip at 0 from below: lo must be 0.  Where k_cone_ws does not exist (orders 129 - 144, above 1024)
// the single-workgroup path is the cold kernel k_cone, which returns P only.
int omc_psd_project_batch(omc_instance* h, int B, int N, const double* M, double lo, double hi, int algo, const double* V0, double* P,
                          double* evals, double* V) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (!M || !P) return fail(OMC_ERR_ARGUMENT, "M / P is NULL");
  if (B < 1) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  if (N < 2) return fail(OMC_ERR_ARGUMENT, "N must be at least 2");
  if (!(lo <= hi)) return fail(OMC_ERR_ARGUMENT, "lo must not exceed hi");
  if (algo < 0 || algo > 2) return fail(OMC_ERR_ARGUMENT, "algo must be 0, 1 or 2");
  if (lo != 0.0) return fail(OMC_ERR_UNSUPPORTED, "omc_psd_project_batch: the eigen-kernels clip at 0 from below, lo must be 0");
  if (N > MW_MAX_ORDER) return fail(OMC_ERR_UNSUPPORTED, "omc_psd_project_batch: order above 4096");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t sB = (size_t)B, NP = (size_t)((N + 15) & ~15);
  OmcWS w;
  memset(&w, 0, sizeof(w));
  w.nB = w.B = w.Btot = B; w.n = N; w.np16 = (int)NP; w.k = 1; w.max_sweeps = MAX_SWEEPS; w.mw_budget = MAX_SWEEPS;
  w.clip_hi = hi < 1e300 ? hi : 1e300;
  w.geo = omc_plan_geometry(N, (int)NP, 1, 1, 1, 1, 0, algo == 1 ? MW_MAX_ORDER + 1 : h->tun.cone_multi_min, MW_MAX_ORDER + 1);
  if (algo == 2 && !w.geo.mw) geom_set_mw(w.geo, N);
  const bool cold = !w.geo.mw && !w.geo.ws_lpp;      // no k_cone_ws at this order (129 .. 144, above 1024): the cold kernel k_cone, as in a relaxation
  if (cold && (evals || V)) return fail(OMC_ERR_UNSUPPORTED, "omc_psd_project_batch: the cold single-workgroup kernel (orders 129 - 144 and above 1024) returns P only");
  BIND(h->pjM, w.Mbuf, sB * NP * NP); BIND(h->pjW, w.W1, sB * N * N);
  if (V0) BIND(h->pjV, w.Vrow, sB * NP * NP); else BIND(h->pjV, w.Vrow, sB * NP * NP, s);      // no starting basis: zeroed (0 x garbage could be NaN)
  int* ints_end = nullptr;
  ENS_CARVE(h->pjD, [&](Carve& c) { walk_project_doubles(c, sB, NP, w); });
  ENS_CARVE(h->pjI, [&](Carve& c) { walk_project_ints(c, sB, w, ints_end); });
  if (w.geo.ws.slab_stride) BIND(h->pjS, w.cone_scratch, sB * w.geo.ws.slab_stride);
  int* ip = w.done;      // done, vvalid, sweeps, mw_stat: one host image goes up and comes back, indexed as the walk placed the arrays
  // symmetrised, zero-padded input, its squared Frobenius norm, the starting basis as the row-major Vrow
  std::vector<double> hM(sB * NP * NP, 0.0), hV(V0 ? sB * NP * NP : 0, 0.0), hf(sB, 0.0);
  for (size_t b = 0; b < sB; ++b) {
    const double* Mb = M + b * N * N; double* Mo = hM.data() + b * NP * NP;
    double f2 = 0.0;
    for (int j = 0; j < N; ++j)
      for (int i = 0; i < N; ++i) { const double v = 0.5 * (Mb[(size_t)j * N + i] + Mb[(size_t)i * N + j]); Mo[(size_t)j * NP + i] = v; f2 += v * v; }
    hf[b] = f2;
    if (V0)
      for (int t = 0; t < N; ++t)
        for (int kk = 0; kk < N; ++kk) hV[b * NP * NP + (size_t)kk * NP + t] = V0[b * N * N + (size_t)t * N + kk];
  }
  std::vector<int> hi_((size_t)(ints_end - ip), 0);
  if (V0) for (size_t b = 0; b < sB; ++b) hi_[(w.vvalid - ip) + b] = 1;
  HIPCHK(hipMemcpyAsync(w.Mbuf, hM.data(), hM.size() * 8, hipMemcpyHostToDevice, s));
  if (V0) HIPCHK(hipMemcpyAsync(w.Vrow, hV.data(), hV.size() * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.fro2, hf.data(), sB * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(ip, hi_.data(), hi_.size() * sizeof(int), hipMemcpyHostToDevice, s));
  EventPair ev;      // device time of the projection alone (uploads and downloads outside)
  HIPCHK(ev.create());
  HIPCHK(hipEventRecord(ev.e0, s));
  if (cold) omc_launch_cone(&w, CONE_BIG, s); else omc_launch_cone_ws(&w, s);
  HIPCHK(hipEventRecord(ev.e1, s));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(P, w.W1, sB * N * N * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hi_.data(), ip, hi_.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  std::vector<double> lam;
  if (evals || V) {
    hV.resize(sB * NP * NP);
    HIPCHK(hipMemcpyAsync(hV.data(), w.Vrow, hV.size() * 8, hipMemcpyDeviceToHost, s));
    if (w.geo.mw) { lam.resize(sB * NP); HIPCHK(hipMemcpyAsync(lam.data(), w.ev_out, lam.size() * 8, hipMemcpyDeviceToHost, s)); }
  }
  HIPCHK(hipStreamSynchronize(s));
  // sweep statistics of this call (omc_last_cone_multi_stats): calls, most sweeps of a matrix, exhausted budgets, the same maximum
  h->mw_tot[0] = B; h->mw_tot[1] = 0; h->mw_tot[2] = 0;
  for (size_t b = 0; b < sB; ++b) {
    h->mw_tot[1] = std::max<long long>(h->mw_tot[1], hi_[(w.sweeps - ip) + b]);
    if (w.geo.mw) h->mw_tot[2] += hi_[(w.mw_stat - ip) + 4 * b + 2];
  }
  h->mw_tot[3] = h->mw_tot[1];
  { float msv = 0.f; HIPCHK(hipEventElapsedTime(&msv, ev.e0, ev.e1)); h->mw_tot[4] = (long long)(1000.0 * msv); }
  if (evals || V) {      // ascending eigenvalues, V permuted with them (the kernels leave the columns in no particular order)
    std::vector<double> lb(N); std::vector<int> perm(N);
    for (size_t b = 0; b < sB; ++b) {
      const double* Vr = hV.data() + b * NP * NP; const double* Mo = hM.data() + b * NP * NP;
      if (w.geo.mw) for (int t = 0; t < N; ++t) lb[t] = lam[b * NP + t];
      else {      // k_cone_ws keeps its eigenvalues in LDS: Rayleigh quotients of the returned eigenvectors
        for (int t = 0; t < N; ++t) {
          double q = 0.0;
          for (int j = 0; j < N; ++j) { const double vj = Vr[(size_t)j * NP + t]; double a = 0.0; for (int i = 0; i < N; ++i) a += Mo[(size_t)j * NP + i] * Vr[(size_t)i * NP + t]; q += a * vj; }
          lb[t] = q;
        }
      }
      for (int t = 0; t < N; ++t) perm[t] = t;
      std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) { return lb[x] < lb[y]; });
      for (int t = 0; t < N; ++t) {
        if (evals) evals[b * N + t] = lb[perm[t]];
        if (V) for (int kk = 0; kk < N; ++kk) V[b * N * N + (size_t)t * N + kk] = Vr[(size_t)kk * NP + perm[t]];
      }
    }
  }
  return 0;
}

// The column prox (block F of the ADMM iteration; the exact multipliers of the certificate in mode 1) on its own, through the launcher the solver
// uses: an empty batch is staged for a workspace of the right size with the identity slot map (as omc_separation_batch does), the inputs are
// written over it and omc_launch_colprox runs once.
int omc_column_prox_batch(omc_instance* h, int B, int mode, int algo, const double* Y, const double* alpha_old, const double* rho_f,
                          const double* s0, double* alpha, double* s, double* objcol, double* c0col, int* nfact) {
  if (mode != 0 && mode != 1) return fail(OMC_ERR_ARGUMENT, "omc_column_prox_batch: mode must be 0 or 1");
  if (algo < 0 || algo > 2) return fail(OMC_ERR_ARGUMENT, "omc_column_prox_batch: algo must be 0, 1 or 2");
  if (!h) return fail(OMC_ERR_ARGUMENT, "omc_column_prox_batch: handle is NULL");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "omc_column_prox_batch: B must be positive");
  if (!Y || !alpha) return fail(OMC_ERR_ARGUMENT, "omc_column_prox_batch: Y / alpha is NULL");
  if (mode == 0 && (!rho_f || !s)) return fail(OMC_ERR_ARGUMENT, "omc_column_prox_batch: mode 0 needs rho_f and s");
  if (mode == 1 && (!objcol || !c0col)) return fail(OMC_ERR_ARGUMENT, "omc_column_prox_batch: mode 1 needs objcol and c0col");
  std::vector<int> Lz(B, 0);
  const omc_relax_params keep = h->params;
  omc_relax_params P = keep; P.slots = B; P.accel = 0;      // identity slot map; without acceleration the workspace has Yx
  StageMode stage_mode;
  stage_mode.colprox_force = algo;
  int rc = stage_base(h, B, &P, OMC_CUT_LINEAR, Lz.data(), nullptr, nullptr, nullptr, nullptr, nullptr, stage_mode);
  h->params = keep;
  if (rc) return rc;
  h->staged = false;
  OmcWS w = h->ws;
  w.rho_f_ratio = 1.0;      // rho_b carries the caller's rho_f itself
  const size_t sB = (size_t)B, n = h->n, m = h->m, nnz = h->nnz;
  hipStream_t st = h->stream;
  BIND(h->bnfact, w.cp_nfact, sB * m);
  HIPCHK(hipMemsetAsync(w.cp_nfact, 0xFF, sB * m * sizeof(int), st));      // -1: the kernel that ran the column does not count (k_colprox_pair, k_colprox_wide)
  HIPCHK(hipMemsetAsync(w.done, 0, sB * sizeof(int), st));
  HIPCHK(hipMemcpyAsync(mode == 0 ? w.Yx : w.Y, Y, sB * n * n * 8, hipMemcpyHostToDevice, st));
  std::vector<double> hs;
  if (mode == 0) {
    HIPCHK(hipMemcpyAsync(w.rho_b, rho_f, sB * 8, hipMemcpyHostToDevice, st));
    if (alpha_old) HIPCHK(hipMemcpyAsync(w.alpha, alpha_old, sB * nnz * 8, hipMemcpyHostToDevice, st));
    else HIPCHK(hipMemsetAsync(w.alpha, 0, sB * nnz * 8, st));
    if (s0) HIPCHK(hipMemcpyAsync(w.sval, s0, sB * m * 8, hipMemcpyHostToDevice, st));
    else { hs.assign(sB * m, -1.0); HIPCHK(hipMemcpyAsync(w.sval, hs.data(), sB * m * 8, hipMemcpyHostToDevice, st)); }
  } else {
    hs.assign(sB, 1.0);      // unused by mode 1 beyond being finite
    HIPCHK(hipMemcpyAsync(w.rho_b, hs.data(), sB * 8, hipMemcpyHostToDevice, st));
  }
  omc_launch_colprox(&w, mode, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(alpha, mode == 0 ? w.alpha : w.alphaX, sB * nnz * 8, hipMemcpyDeviceToHost, st));
  if (mode == 0) HIPCHK(hipMemcpyAsync(s, w.sval, sB * m * 8, hipMemcpyDeviceToHost, st));
  else {
    HIPCHK(hipMemcpyAsync(objcol, w.objcol, sB * m * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(c0col, w.c0col, sB * m * 8, hipMemcpyDeviceToHost, st));
  }
  if (nfact) HIPCHK(hipMemcpyAsync(nfact, w.cp_nfact, sB * m * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return 0;
}

// The row projection of k_global (step 4) on its own, one wave per problem, in a buffer of its own: nothing of the instance is touched
// beyond its device and stream.
int omc_row_project_batch(omc_instance* h, int B, int R, int Rmax, int which, const double* G, const double* c, const double* lam0,
                          double* lam, int* overflow) {
  if (which != 0 && which != 1) return fail(OMC_ERR_ARGUMENT, "omc_row_project_batch: which must be 0 or 1");
  if (!h) return fail(OMC_ERR_ARGUMENT, "omc_row_project_batch: handle is NULL");
  if (B <= 0 || R <= 0 || Rmax < R) return fail(OMC_ERR_ARGUMENT, "omc_row_project_batch: need B > 0 and 0 < R <= Rmax");
  if (!G || !c || !lam || !overflow) return fail(OMC_ERR_ARGUMENT, "omc_row_project_batch: G / c / lam / overflow is NULL");
  HIPCHK(hipSetDevice(h->device));
  const size_t sB = (size_t)B, sR = (size_t)Rmax;
  DevBuf buf;
  double *dG = nullptr, *dc = nullptr, *dl = nullptr; int* dov = nullptr;
  ENS_CARVE(buf, [&](Carve& cv) { dG = cv.take<double>(sB * sR * sR); dc = cv.take<double>(sB * sR); dl = cv.take<double>(sB * sR); dov = cv.take<int>(sB); });
  hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(dG, G, sB * sR * sR * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dc, c, sB * sR * 8, hipMemcpyHostToDevice, st));
  if (lam0) HIPCHK(hipMemcpyAsync(dl, lam0, sB * sR * 8, hipMemcpyHostToDevice, st));
  else HIPCHK(hipMemsetAsync(dl, 0, sB * sR * 8, st));
  omc_launch_row_project(B, R, Rmax, which, dG, dc, dl, dov, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(lam, dl, sB * sR * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(overflow, dov, sB * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return 0;
}

int omc_colprox_plan(int n, int cmax, int block_min, int64_t* out) {
  if (!out) return fail(OMC_ERR_ARGUMENT, "out is NULL");
  if (n <= 0 || cmax <= 0 || cmax > n) return fail(OMC_ERR_ARGUMENT, "omc_colprox_plan: need 0 < cmax <= n");
  long long o[5];
  cp_block_plan(cmax, block_min, o);
  for (int q = 0; q < 5; ++q) out[q] = o[q];
  return 0;
}

int omc_plain_multi_plan(int n, int plain_multi_min, int64_t* out) {
  if (!out) return fail(OMC_ERR_ARGUMENT, "out is NULL");
  if (n <= 0) return fail(OMC_ERR_ARGUMENT, "omc_plain_multi_plan: n must be positive");
  const int np16 = (n + 15) & ~15;
  const OmcGeom g = omc_plan_geometry(n, np16, 1, 1, 1, 1, 0, MW_MAX_ORDER + 1, plain_multi_min);
  const MwLayout L = mw_layout(n);
  out[0] = g.plain_mw; out[1] = np16; out[2] = L.Ncp; out[3] = L.nb; out[4] = (int64_t)L.bytes; out[5] = mw_plain_launches(L, MAX_SWEEPS);
  return 0;
}

double omc_plain_multi_tau(void) { return MW_TAU_PLAIN; }

int omc_last_plain_multi_stats(omc_instance* h, int64_t* out) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  for (int q = 0; q < 4; ++q) out[q] = h->pmw_tot[q];
  return 0;
}

int omc_last_cone_multi_stats(omc_instance* h, int64_t* out) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  for (int q = 0; q < 5; ++q) out[q] = h->mw_tot[q];
  return 0;
}

int omc_altmin_batch(omc_instance* h, int B, int cut_type, int reference_quirk_q1, const int* L, const double* cut_x,
                     const double* cut_Uhat, const int8_t* cut_dir, const double* U_initial, double eps, int max_iters,
                     double time_limit, double* U, double* V, int* converged, int* n_iters, double* objectives,
                     double* solve_time) {
  if (!h || !U_initial || !U || !V) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (B <= 0 || max_iters <= 0) return fail(OMC_ERR_ARGUMENT, "B and max_iters must be positive");
  if (cut_type != OMC_CUT_LINEAR && cut_type != OMC_CUT_LINEAR2 && cut_type != OMC_CUT_LINEAR3)
    return fail(OMC_ERR_INVALID_ENUM, "Invalid input for disjunctive cuts type (OMC.jl:1456-1462)");
  if (!(time_limit > 0.0)) {      // OMC.jl:2186-2189: the loop condition fails at once -- nothing is solved (a positive limit is checked inside the launch, at the top of every iteration)
    const size_t nk = (size_t)h->n * h->k, mk = (size_t)h->m * h->k;
    for (int b = 0; b < B; ++b) { if (converged) converged[b] = 0; if (n_iters) n_iters[b] = 0; if (solve_time) solve_time[b] = 0.0; }
    memset(U, 0, sizeof(double) * nk * B); memset(V, 0, sizeof(double) * mk * B);
    if (objectives) for (size_t e = 0; e < (size_t)B * max_iters; ++e) objectives[e] = NAN;
    h->amobj_B = 0;
    return 0;
  }
  if (h->k > ALTMIN_KMAX) return fail(OMC_ERR_UNSUPPORTED, "omc_altmin_batch: rank k > 8 is not supported");
  HIPCHK(hipSetDevice(h->device));
  const int n = h->n, m = h->m, k = h->k;
  auto t0 = std::chrono::steady_clock::now();
  int Lmax = 1; long Ltot = 0;
  for (int b = 0; b < B; ++b) { int Lb = L ? L[b] : 0; if (Lb < 0) return fail(OMC_ERR_ARGUMENT, "negative cut count"); Lmax = std::max(Lmax, Lb); Ltot += Lb; }
  if (Ltot > 0 && (!cut_x || !cut_Uhat || !cut_dir)) return fail(OMC_ERR_ARGUMENT, "cut arrays are NULL but L > 0");
  // rows of model_U: box entries not implied by ||U_j|| <= 1 (defaults OMC.jl:1989-1996: U[n-k+j.., j] >= 0), per-cut bounds on
  // every column (2047-2093)
  const int Rmax = k * (k + 1) / 2 + 2 * k * Lmax;
  const size_t sB = (size_t)B;
  std::vector<int> hR(B, 0), hk(sB * Rmax, 0), hc(sB * Rmax, 0), hbi(sB * Rmax, 0), hbj(sB * Rmax, 0);
  std::vector<double> hcoef(sB * Rmax, 0.0), hrhs(sB * Rmax, 0.0), hx(sB * Lmax * n, 0.0);
  long cutbase = 0;
  for (int b = 0; b < B; ++b) {
    int r = 0;
    auto add = [&](int kind, int cut, int bi, int bj, double cf, double rhs) {
      hk[(size_t)b * Rmax + r] = kind; hc[(size_t)b * Rmax + r] = cut; hbi[(size_t)b * Rmax + r] = bi; hbj[(size_t)b * Rmax + r] = bj;
      hcoef[(size_t)b * Rmax + r] = cf; hrhs[(size_t)b * Rmax + r] = rhs; ++r;
    };
    for (int j = 0; j < k; ++j)
      for (int i = n - k + j; i < n; ++i) add(ROW_BOX, -1, i, j, -1.0, 0.0);     // -U[i,j] <= 0  (symmetry breaking, OMC.jl:1991-1993)
    const int Lb = L ? L[b] : 0;
    for (int l = 0; l < Lb; ++l) {
      const double* x = cut_x + (size_t)(cutbase + l) * n;
      for (int j = 0; j < k; ++j) {
        const double* Uh = cut_Uhat + ((size_t)(cutbase + l) * k + j) * n;
        double vhat = 0.0;
        for (int i = 0; i < n; ++i) vhat += Uh[i] * x[i];      // OMC.jl:2053
        double lo, hi, sl, ic;
        if (cut_piece(cut_type, cut_dir[(size_t)(cutbase + l) * k + j], vhat, reference_quirk_q1, &lo, &hi, &sl, &ic))
          return fail(OMC_ERR_INVALID_ENUM, "direction code invalid for this cut type (OMC.jl:2056-2091)");
        add(ROW_BOUND, l, -1, j, 1.0, hi);
        add(ROW_BOUND, l, -1, j, -1.0, -lo);
      }
      memcpy(&hx[((size_t)b * Lmax + l) * n], x, sizeof(double) * n);
    }
    hR[b] = r; cutbase += Lb;
  }
  int rc_ = 0;
  hipStream_t s = h->stream;
  if ((rc_ = upload(h->aR, hR.data(), sizeof(int) * B, s))) return rc_;
  if ((rc_ = upload(h->arkind, hk.data(), sizeof(int) * hk.size(), s))) return rc_;
  if ((rc_ = upload(h->arcut, hc.data(), sizeof(int) * hc.size(), s))) return rc_;
  if ((rc_ = upload(h->arbi, hbi.data(), sizeof(int) * hbi.size(), s))) return rc_;
  if ((rc_ = upload(h->arbj, hbj.data(), sizeof(int) * hbj.size(), s))) return rc_;
  if ((rc_ = upload(h->arcoef, hcoef.data(), sizeof(double) * hcoef.size(), s))) return rc_;
  if ((rc_ = upload(h->arrhs, hrhs.data(), sizeof(double) * hrhs.size(), s))) return rc_;
  if ((rc_ = upload(h->acutx, hx.data(), sizeof(double) * hx.size(), s))) return rc_;
  if ((rc_ = upload(h->aU0, U_initial, sizeof(double) * sB * n * k, s))) return rc_;
  AltminWS w{};
  BIND(h->aU, w.U, sB * n * k); BIND(h->aV, w.V, sB * m * k); BIND(h->aobj, w.objectives, sB * max_iters);
  BIND(h->aint, w.converged, sB * 2); w.n_iters = w.converged + B;
  BIND(h->amobj, w.mobj, sB);
  h->amobj_B = B;
  BIND(h->aG, w.G, sB * Rmax * Rmax);
  w.B = B; w.n = n; w.m = m; w.k = k; w.Rmax = Rmax; w.Lmax = Lmax; w.max_iters = max_iters;
  w.gamma = h->gamma; w.eps = eps; w.sumA2 = h->sumA2;
  {   // time_limit in clock ticks (at least 1); 0 = no limit: clock rate unknown, or a value that is not finite or does not fit
    const double ticks = time_limit * 1000.0 * (double)h->wall_khz;
    w.tl_ticks = (h->wall_khz > 0 && std::isfinite(ticks) && ticks < 4.0e18) ? std::max<long long>(1, (long long)ticks) : 0;
  }
  w.col_ptr = h->dcol_ptr.as<int>(); w.col_idx = h->dcol_idx.as<int>(); w.col_val = h->dcol_val.as<double>();
  w.row_ptr = h->drow_ptr.as<int>(); w.row_idx = h->drow_idx.as<int>(); w.row_val = h->drow_val.as<double>();
  w.R = h->aR.as<int>(); w.rkind = h->arkind.as<int>(); w.rcut = h->arcut.as<int>(); w.rbi = h->arbi.as<int>(); w.rbj = h->arbj.as<int>();
  w.rcoef = h->arcoef.as<double>(); w.rrhs = h->arrhs.as<double>(); w.cutx = h->acutx.as<double>();
  w.U0 = h->aU0.as<double>();
  // a problem that does not fit the LDS (config 5: 1000 x 1000, k = 2 needs 144 KB) runs the same kernel on a per-problem global slab
  const KernelPlan ap = altmin_plan(n, m, k, Rmax, h->tun.altmin_nolds);
  w.scratch = nullptr; w.scratch_stride = ap.slab_stride; w.lds_bytes = ap.lds_bytes;
  if (ap.slab_stride) BIND(h->aG2, w.scratch, (size_t)B * ap.slab_stride);
  omc_launch_altmin(&w, s);
  HIPCHK(hipMemcpyAsync(U, w.U, 8 * sB * n * k, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(V, w.V, 8 * sB * m * k, hipMemcpyDeviceToHost, s));
  if (objectives) HIPCHK(hipMemcpyAsync(objectives, w.objectives, 8 * sB * max_iters, hipMemcpyDeviceToHost, s));
  if (converged) HIPCHK(hipMemcpyAsync(converged, w.converged, 4 * sB, hipMemcpyDeviceToHost, s));
  if (n_iters) HIPCHK(hipMemcpyAsync(n_iters, w.n_iters, 4 * sB, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (solve_time) for (int b = 0; b < B; ++b) solve_time[b] = el;
  return 0;
}

int omc_altmin_plan(int n, int m, int k, int max_cuts, int nolds, int64_t* out) {
  if (!out) return fail(OMC_ERR_ARGUMENT, "out is NULL");
  if (n <= 0 || m <= 0 || k <= 0) return fail(OMC_ERR_ARGUMENT, "n, m and k must be positive");
  if (k > ALTMIN_KMAX) return fail(OMC_ERR_UNSUPPORTED, "omc_altmin_plan: rank k > 8 is not supported");
  const int Rmax = k * (k + 1) / 2 + 2 * k * std::max(1, max_cuts);      // as omc_altmin_batch sizes the rows of model_U
  const KernelPlan ap = altmin_plan(n, m, k, Rmax, nolds != 0);
  out[0] = altmin_variant(k); out[1] = (int64_t)ap.lds_bytes; out[2] = (int64_t)ap.slab_stride * 8; out[3] = Rmax;
  return 0;
}

int omc_altmin_master_objectives(omc_instance* h, int B, double* objective) {
  if (!h || !objective) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (B <= 0 || B != h->amobj_B) return fail(OMC_ERR_ARGUMENT, "B does not match the last omc_altmin_batch call");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(objective, h->amobj.p, 8 * (size_t)B, hipMemcpyDeviceToHost, h->stream));      // never the legacy stream: another handle may be capturing a graph
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

