// omc_api_cert.cpp -- dual certificates behind the C ABI of include/omc.h: omc_relax_keep_certificates, omc_certificate_plan,
// omc_relax_fetch_certificate and their Shor-mode forms (omc_relax_keep_shor_certificates, omc_shor_certificate_plan,
// omc_relax_fetch_shor_certificate), and the two evaluators of caller-supplied multipliers, omc_dual_bound_batch and
// omc_shor_dual_bound_batch (with omc_shor_dual_bound_plan, omc_last_shor_dual_bound_ms).  The reference driver has no counterpart: its
// bound is Mosek's (OMC.jl:1838-1877); rows and row basis are those of matrix_completion_SDP_relaxation (OMC.jl:1558-1685).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>

#include "omc_api_internal.h"

#include "omc_shor_cert.h"

// ---- best certificate per node (omc.h: "certificates") ------------------------------------------------------------------------------------
// The request applies to the stage calls that follow: they allocate the slot buffers and the arena (OmcWS::cert_flag ...), and the kernels
// that already run test the pointer.  Off: nothing is allocated and no kernel is added to a solve.
int omc_relax_keep_certificates(omc_instance* h, int on) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (h->worker.joinable() || h->worker_running.load()) return fail(OMC_ERR_ARGUMENT, "omc_relax_keep_certificates: a solve is in flight (call omc_relax_wait first)");
  h->keep_cert = on != 0;
  return 0;
}

int omc_certificate_plan(int n, int k, int nnz, int max_cuts, int nonstandard_box_rows, int64_t* out) {
  if (!out) return fail(OMC_ERR_ARGUMENT, "out is NULL");
  if (n <= 0 || k <= 0 || nnz < 0 || max_cuts < 0 || nonstandard_box_rows < 0) return fail(OMC_ERR_ARGUMENT, "omc_certificate_plan: n and k must be positive, the counts not negative");
  if (k > 8) return fail(OMC_ERR_UNSUPPORTED, "omc_certificate_plan: rank k > 8 is not supported");
  const int64_t Rmax = 1 + (int64_t)k * (k + 1) / 2 + nonstandard_box_rows + (int64_t)max_cuts * (2 * k + 1);
  const int64_t rmax = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)k + nonstandard_box_rows + max_cuts));
  out[0] = nnz; out[1] = Rmax; out[2] = (int64_t)n * rmax; out[3] = (rmax + k) * (rmax + k);
  out[4] = 8 * (1 + out[0] + out[1] + out[3]) + 4;      // what the arena holds per node: bound, Lam, lam, Psi3, the flag (Q is part of the node's descriptor)
  out[5] = rmax;
  return 0;
}

int omc_relax_fetch_certificate(omc_instance* h, int n_ids, const int* node_ids, double* Lam, double* lam, int* R, double* Q, int* r,
                                double* Psi3, double* bound) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (!h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_certificate: nothing staged");
  const OmcWS& w = h->ws;
  if (!w.cert_flag || !w.ocLam)      // a Shor-mode batch keeps certificates of its own (omc_relax_fetch_shor_certificate)
    return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_certificate: the batch was staged without omc_relax_keep_certificates(h, 1)");
  if (n_ids < 0 || (n_ids > 0 && !node_ids)) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_certificate: bad arguments");
  if (n_ids == 0) return 0;
  { int rcf = require_finished_ids(h, n_ids, node_ids, false, "omc_relax_fetch_certificate"); if (rcf) return rcf; }
  HIPCHK(hipSetDevice(h->device));
  if (!h->fetch_stream) HIPCHK(hipStreamCreateWithFlags(&h->fetch_stream, hipStreamNonBlocking));
  hipStream_t fs = h->fetch_stream;
  { int rcc = require_certificates(w, n_ids, node_ids, fs, "omc_relax_fetch_certificate"); if (rcc) return rcc; }
  const size_t nnz = (size_t)w.nnz, Rm = (size_t)w.Rmax, nq = (size_t)w.n * w.rmax, ps = (size_t)(w.rmax + w.k) * (w.rmax + w.k);
  for (int i = 0; i < n_ids; ++i) {
    const size_t nb = (size_t)node_ids[i], o = (size_t)i;
    if (Lam) HIPCHK(hipMemcpyAsync(Lam + o * nnz, w.ocLam + nb * nnz, 8 * nnz, hipMemcpyDeviceToHost, fs));
    if (lam) HIPCHK(hipMemcpyAsync(lam + o * Rm, w.oclam + nb * Rm, 8 * Rm, hipMemcpyDeviceToHost, fs));
    if (R) HIPCHK(hipMemcpyAsync(R + o, w.R + nb, sizeof(int), hipMemcpyDeviceToHost, fs));
    if (Q) HIPCHK(hipMemcpyAsync(Q + o * nq, w.Qb + nb * nq, 8 * nq, hipMemcpyDeviceToHost, fs));
    if (r) HIPCHK(hipMemcpyAsync(r + o, w.rr + nb, sizeof(int), hipMemcpyDeviceToHost, fs));
    if (Psi3) HIPCHK(hipMemcpyAsync(Psi3 + o * ps, w.ocPsi + nb * ps, 8 * ps, hipMemcpyDeviceToHost, fs));
    if (bound) HIPCHK(hipMemcpyAsync(bound + o, w.ocBound + nb, 8, hipMemcpyDeviceToHost, fs));
  }
  HIPCHK(hipStreamSynchronize(fs));
  return 0;
}

// ---- the same for Shor mode (omc.h: "Shor-mode certificates") -------------------------------------------------------------------------------
int omc_relax_keep_shor_certificates(omc_instance* h, int on) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (h->worker.joinable() || h->worker_running.load()) return fail(OMC_ERR_ARGUMENT, "omc_relax_keep_shor_certificates: a solve is in flight (call omc_relax_wait first)");
  h->keep_shor_cert = on != 0;
  return 0;
}

int omc_shor_certificate_plan(int n, int m, int k, int64_t nq_stride, int max_cuts, int nonstandard_box_rows, int64_t* out) {
  if (!out) return fail(OMC_ERR_ARGUMENT, "out is NULL");
  if (n <= 0 || m <= 0 || k <= 0 || nq_stride < 0 || max_cuts < 0 || nonstandard_box_rows < 0)
    return fail(OMC_ERR_ARGUMENT, "omc_shor_certificate_plan: n, m and k must be positive, the counts not negative");
  if (k > 1) return fail(OMC_ERR_UNSUPPORTED, "omc_shor_certificate_plan: Shor-mode certificates exist for rank 1 only");
  const int64_t Rmax = 1 + (int64_t)k * (k + 1) / 2 + nonstandard_box_rows + (int64_t)max_cuts * (2 * k + 1);
  const int64_t rmax = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)k + nonstandard_box_rows + max_cuts));
  out[0] = Rmax; out[1] = (int64_t)n * rmax; out[2] = (rmax + k) * (rmax + k); out[3] = 15 * nq_stride; out[4] = m; out[5] = (int64_t)n * m; out[6] = (int64_t)n * m;
  const int64_t per = out[0] + out[2] + out[3] + out[4] + out[5] + out[6];      // Q is part of the node's descriptor
  out[7] = 8 * (1 + per) + 8;      // arena, per node: the bound, the arrays, the flag and the minor count
  out[8] = 8 * (2 + per) + 8;      // per slot: penalty and bound of the check, the arrays, two flags
  out[9] = rmax;
  return 0;
}

int omc_relax_fetch_shor_certificate(omc_instance* h, int n_ids, const int* node_ids, double* scale, double* bound, double* lam, int* R, double* Q,
                                     int* r, double* Psi3, double* Gam, double* zeta, double* xi, double* Xbar, int* nq, int64_t* nq_stride) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (!h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_shor_certificate: nothing staged");
  const OmcWS& w = h->ws; const ShWS& sh = h->sh;
  if (!h->shor_on || !sh.cbGam || !w.cert_flag)
    return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_shor_certificate: the batch was staged without omc_relax_keep_shor_certificates(h, 1) (or is not a Shor-mode batch)");
  if (n_ids < 0 || (n_ids > 0 && !node_ids)) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_shor_certificate: bad arguments");
  if (nq_stride) *nq_stride = sh.nqmax;
  if (n_ids == 0) return 0;
  { int rcf = require_finished_ids(h, n_ids, node_ids, false, "omc_relax_fetch_shor_certificate"); if (rcf) return rcf; }
  HIPCHK(hipSetDevice(h->device));
  if (!h->fetch_stream) HIPCHK(hipStreamCreateWithFlags(&h->fetch_stream, hipStreamNonBlocking));
  hipStream_t fs = h->fetch_stream;
  { int rcc = require_certificates(w, n_ids, node_ids, fs, "omc_relax_fetch_shor_certificate"); if (rcc) return rcc; }
  const size_t Rm = (size_t)w.Rmax, nqd = (size_t)w.n * w.rmax, ps = (size_t)(w.rmax + w.k) * (w.rmax + w.k), gs = (size_t)15 * sh.nqmax, m = (size_t)sh.m, nm = (size_t)sh.n * sh.m;
  for (int i = 0; i < n_ids; ++i) {
    const size_t nb = (size_t)node_ids[i], o = (size_t)i;
    if (scale) scale[o] = sh.sc;
    if (bound) HIPCHK(hipMemcpyAsync(bound + o, w.ocBound + nb, 8, hipMemcpyDeviceToHost, fs));
    if (lam) HIPCHK(hipMemcpyAsync(lam + o * Rm, w.oclam + nb * Rm, 8 * Rm, hipMemcpyDeviceToHost, fs));
    if (R) HIPCHK(hipMemcpyAsync(R + o, w.R + nb, sizeof(int), hipMemcpyDeviceToHost, fs));
    if (Q) HIPCHK(hipMemcpyAsync(Q + o * nqd, w.Qb + nb * nqd, 8 * nqd, hipMemcpyDeviceToHost, fs));
    if (r) HIPCHK(hipMemcpyAsync(r + o, w.rr + nb, sizeof(int), hipMemcpyDeviceToHost, fs));
    if (Psi3) HIPCHK(hipMemcpyAsync(Psi3 + o * ps, w.ocPsi + nb * ps, 8 * ps, hipMemcpyDeviceToHost, fs));
    if (Gam && gs) HIPCHK(hipMemcpyAsync(Gam + o * gs, sh.ocGam + nb * gs, 8 * gs, hipMemcpyDeviceToHost, fs));
    if (zeta) HIPCHK(hipMemcpyAsync(zeta + o * m, sh.ocZeta + nb * m, 8 * m, hipMemcpyDeviceToHost, fs));
    if (xi) HIPCHK(hipMemcpyAsync(xi + o * nm, sh.ocXi + nb * nm, 8 * nm, hipMemcpyDeviceToHost, fs));
    if (Xbar) HIPCHK(hipMemcpyAsync(Xbar + o * nm, sh.ocXbar + nb * nm, 8 * nm, hipMemcpyDeviceToHost, fs));
    if (nq) HIPCHK(hipMemcpyAsync(nq + o, sh.ocNq + nb, sizeof(int), hipMemcpyDeviceToHost, fs));
  }
  HIPCHK(hipStreamSynchronize(fs));
  return 0;
}

// ---- the private eigen-kernel view of the two dual-bound evaluators ------------------------------------------------------------------------
// A workspace of their own with the dimensions of V views, through which k_dual_assemble and the eigen-kernel a check of a relaxation at this
// order would take run, cold.  No batch is staged and a staged one is not touched.
static EvalDims eval_view_dims(omc_instance* h, OmcWS& w, int V, int k, const NodePack& pk) {
  const EvalDims d = {(size_t)V, (size_t)h->n, (size_t)k, (size_t)h->nnz, (size_t)pk.Rmax, (size_t)pk.rmax, (size_t)std::max(pk.Lmax, 1)};
  memset(&w, 0, sizeof(w));
  w.nB = w.B = w.Btot = V; w.n = h->n; w.m = h->m; w.k = k; w.nnz = h->nnz; w.Rmax = (int)d.Rmax; w.Lmax = (int)d.Lmax; w.rmax = (int)d.rmax;
  w.np16 = (h->n + 15) & ~15; w.max_sweeps = MAX_SWEEPS; w.mw_budget = MAX_SWEEPS; w.gamma = h->gamma; w.clip_hi = 1.0; w.inv_s2 = 1.0;
  w.col_ptr = h->dcol_ptr.as<int>(); w.col_idx = h->dcol_idx.as<int>(); w.col_val = h->dcol_val.as<double>();
  w.geo = omc_plan_geometry(w.n, w.np16, k, w.rmax, w.Rmax, h->cmax, h->tun.global_nolds, h->tun.cone_multi_min, MW_MAX_ORDER + 1);
  return d;
}
// the flags and statistics the eigen-kernel reads, and the matrices: the zero padding of MbufC; VrowC: cold start, and 0 x garbage could be NaN.
// Both lengths come from the walks (omc_walks.h)
static int eval_view_zero(const OmcWS& w, const EvalArrays& a, hipStream_t s) {
  HIPCHK(hipMemsetAsync(w.done, 0, (size_t)((char*)a.zero_end - (char*)w.done), s));
  HIPCHK(hipMemsetAsync(w.MbufC, 0, (size_t)((char*)w.Mchk - (char*)w.MbufC), s));
  return 0;
}
// k_cone_ws LDS- or L2-resident and the multi-workgroup kernels from OMC_CONE_MULTI_MIN on, k_cone at orders 129 - 144; then everything from
// c0 to scalars_end on its way to `scal` (a scalar x of view v is scal[(w.x - w.c0) + v]): the caller synchronises
static int eval_view_solve(OmcWS& w, const EvalArrays& a, hipEvent_t after, std::vector<double>& scal, hipStream_t s) {
  if (w.geo.ws_lpp || w.geo.mw) { w.ws_mode = 1; omc_launch_cone_ws(&w, s); }
  else omc_launch_cone(&w, CONE_EVALS, s);
  if (after) HIPCHK(hipEventRecord(after, s));
  HIPCHK(hipGetLastError());
  scal.resize((size_t)(a.scalars_end - w.c0));
  HIPCHK(hipMemcpyAsync(scal.data(), w.c0, (size_t)((char*)a.scalars_end - (char*)w.c0), hipMemcpyDeviceToHost, s));
  return 0;
}

// The Lagrangian bound of caller-supplied multipliers (omc.h).  Rows and row basis on the host exactly as omc_relax_stage builds them
// (pack_nodes, put_descriptors) into buffers of its own, k_dual_assemble for the matrix and the constants, then the eigen-kernel a check of a
// relaxation at this order would take (k_cone_ws LDS- or L2-resident, k_cone at orders 129 - 144, the multi-workgroup kernels from
// OMC_CONE_MULTI_MIN on) through a private view, cold.  No batch is staged and a staged one is not touched.
int omc_dual_bound_batch(omc_instance* h, int B, int cut_type, int reference_quirk_q1, const int* L, const double* cut_x, const double* cut_Uhat,
                         const int8_t* cut_dir, const double* U_lower, const double* U_upper, const double* Lam, const double* lam,
                         const double* Psi3, double* Q_out, int* r_out, double* bound) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "omc_dual_bound_batch: handle is NULL");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "omc_dual_bound_batch: B must be positive");
  { int rcc = check_cut_type(cut_type); if (rcc) return rcc; }
  const bool query = !Lam && !lam && !Psi3 && !bound;      // rows and basis only
  if (!query && (!Lam || !lam || !bound)) return fail(OMC_ERR_ARGUMENT, "omc_dual_bound_batch: Lam, lam and bound are needed (all of Lam, lam, Psi3, bound NULL: Q_out / r_out only)");
  if (h->worker.joinable() || h->worker_running.load()) return fail(OMC_ERR_ARGUMENT, "omc_dual_bound_batch: a solve is in flight on this handle (call omc_relax_wait first)");
  omc_relax_params P = h->params; P.reference_quirk_q1 = reference_quirk_q1 ? 1 : 0;
  NodePack pk;
  { int rcp = pack_nodes(h, P, cut_type, B, L, cut_x, cut_Uhat, cut_dir, U_lower, U_upper, pk); if (rcp) return rcp; }
  const size_t sB = (size_t)B, n = h->n, m = h->m, k = h->k, nnz = h->nnz, Rmax = pk.Rmax, rmax = pk.rmax;
  if (r_out) for (int b = 0; b < B; ++b) r_out[b] = pk.rrv[b];
  if (Q_out)
    for (size_t b = 0; b < sB; ++b) {
      std::fill(Q_out + b * n * rmax, Q_out + (b + 1) * n * rmax, 0.0);
      std::copy(pk.Qn[b].begin(), pk.Qn[b].end(), Q_out + b * n * rmax);
    }
  if (query) return 0;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t ps = (rmax + k) * (rmax + k);
  OmcWS w;
  const EvalDims d = eval_view_dims(h, w, B, (int)k, pk);
  EvalArrays a{};
  ENS_CARVE(h->dbM, [&](Carve& c) { walk_dual_matrices(c, d, w); });
  if (w.geo.ws.slab_stride) BIND(h->dbS, w.cone_scratch, sB * w.geo.ws.slab_stride);
  if (n > 144) BIND(h->dbL, w.lamDX, sB * m * n, s);
  // descriptors, multipliers, scratch and the per-node scalars
  ENS_CARVE(h->dbD, [&](Carve& c) { walk_dual_doubles(c, d, w, a); });
  ENS_CARVE(h->dbI, [&](Carve& c) { walk_dual_ints(c, d, w, a); });
  { int rc = eval_view_zero(w, a, s); if (rc) return rc; }
  { int rc = put_descriptors(w, pk, B, sB, 0, L, cut_x, s); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(a.Lam, Lam, sB * nnz * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(a.lam, lam, sB * Rmax * 8, hipMemcpyHostToDevice, s));
  if (Psi3) HIPCHK(hipMemcpyAsync(a.Psi, Psi3, sB * ps * 8, hipMemcpyHostToDevice, s));
  const OmcDualIn in = {a.Lam, a.lam, Psi3 ? a.Psi : nullptr, a.T1};
  omc_launch_dual_assemble(&w, &in, s);
  std::vector<double> sc;
  { int rc = eval_view_solve(w, a, nullptr, sc, s); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  const size_t o_cpen = w.cpen - w.c0, o_cst = w.cst - w.c0, o_ev = w.evsum - w.c0;      // where the walk placed them behind c0
  for (size_t b = 0; b < sB; ++b) bound[b] = sc[b] + sc[o_ev + b] - sc[o_cpen + b] + sc[o_cst + b];      // c0 + evsum - cpen + cst, the order of k_check_final
  return 0;
}

// ---- omc_shor_dual_bound_batch: the Shor-mode bound of caller-supplied multipliers (omc.h) ---------------------------------
namespace {
// device bytes of omc_shor_dual_bound_batch (the formula of omc_shor_dual_bound_plan in omc.h): per node, per view
struct ScertBytes { size_t node, view; };
static_assert(sizeof(ShorGroupDev) == 120, "the plan of omc_shor_dual_bound_batch documents 120 bytes per list");
static ScertBytes scert_bytes(size_t n, size_t m, size_t nqs, size_t Rmax, size_t rmax, size_t Lmax, size_t slab, bool sanitise) {
  const size_t nm = n * m, NP = (n + 15) & ~(size_t)15, nn4 = (n * n + 3) & ~(size_t)3, nmb = (nqs + SCERT_T - 1) / SCERT_T, ps = (rmax + 1) * (rmax + 1);
  ScertBytes r;
  r.node = 8 * (1 + 15 * nqs + m + 2 * nm) + 8 * ((sanitise ? 15 * nqs : 0) + nmb) + 4 +
           4 * (20 * nqs + nm + m + 3) + ((nm + m + 15) & ~(size_t)15) + sizeof(ShorGroupDev);
  r.view = 8 * (12 * nqs + 2 * nmb + nm + 2 * m) + 4 * m + 8 + 8 * (2 * NP * NP + nn4 + slab) + 8 * (2 * Rmax + Lmax * n + n * rmax) +
           8 * (Rmax + ps + n * rmax + n + 5) + 4 * (4 * Rmax + 9);
  return r;
}
// eigen-decomposition of a symmetric matrix of small order on the host (cyclic Jacobi): A (N x N, overwritten) -> eigenvalues w, vectors V (columns)
static void host_jacobi(int N, std::vector<double>& A, std::vector<double>& wv, std::vector<double>& V) {
  V.assign((size_t)N * N, 0.0); wv.assign(N, 0.0);
  for (int i = 0; i < N; ++i) V[(size_t)i * N + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int r = 0; r < N; ++r) { dg += A[(size_t)r * N + r] * A[(size_t)r * N + r]; for (int c = 0; c < r; ++c) off += A[(size_t)c * N + r] * A[(size_t)c * N + r]; }
    if (!(off > 1e-34 * dg)) break;
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[(size_t)q * N + p];
        if (!(fabs(apq) > 1e-300)) continue;
        const double theta = (A[(size_t)q * N + q] - A[(size_t)p * N + p]) / (2.0 * apq), at = fabs(theta);
        double t = 1.0 / (at + sqrt(at * at + 1.0));
        t = (theta >= 0.0) ? t : -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[(size_t)p * N + p] -= t * apq; A[(size_t)q * N + q] += t * apq; A[(size_t)q * N + p] = 0.0; A[(size_t)p * N + q] = 0.0;
        for (int k = 0; k < N; ++k) {
          if (k != p && k != q) {
            const double akp = A[(size_t)p * N + k], akq = A[(size_t)q * N + k];
            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
            A[(size_t)p * N + k] = np_; A[(size_t)k * N + p] = np_; A[(size_t)q * N + k] = nq_; A[(size_t)k * N + q] = nq_;
          }
          const double vkp = V[(size_t)p * N + k], vkq = V[(size_t)q * N + k];
          V[(size_t)p * N + k] = c * vkp - s * vkq; V[(size_t)q * N + k] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < N; ++i) wv[i] = A[(size_t)i * N + i];
}
}  // namespace

int omc_shor_dual_bound_plan(int n, int m, int k, int B, int64_t nq_stride, int max_cuts, int nonstandard_box_rows, int sanitise, int64_t* out) {
  if (!out) return fail(OMC_ERR_ARGUMENT, "omc_shor_dual_bound_plan: out is NULL");
  if (n <= 0 || m <= 0 || k <= 0 || B <= 0 || nq_stride < 0 || max_cuts < 0 || nonstandard_box_rows < 0)
    return fail(OMC_ERR_ARGUMENT, "omc_shor_dual_bound_plan: n, m, k, B must be positive, the other arguments non-negative");
  if (k > 1) return fail(OMC_ERR_UNSUPPORTED, "omc_shor_dual_bound_plan: Shor-mode certificates exist for rank 1 only");
  if (nq_stride >= (1ll << 28) || (long long)n * m >= (1ll << 30)) return fail(OMC_ERR_UNSUPPORTED, "omc_shor_dual_bound_plan: beyond the size limits of omc_relax_stage_shor");
  const int Rmax = 2 + nonstandard_box_rows + 3 * max_cuts, rmax = std::max(1, std::min(n, 1 + nonstandard_box_rows + max_cuts));
  const Tuning tun;
  const OmcGeom geo = omc_plan_geometry(n, (n + 15) & ~15, 1, rmax, Rmax, n, 0, tun.cone_multi_min, MW_MAX_ORDER + 1);
  const ScertBytes sb = scert_bytes(n, m, (size_t)nq_stride, Rmax, rmax, std::max(max_cuts, 1), geo.ws.slab_stride, sanitise != 0);
  const int ways = sanitise ? 2 : 1;
  out[0] = (int64_t)(sb.node + ways * sb.view); out[1] = out[0] * B; out[2] = (int64_t)sb.node; out[3] = (int64_t)sb.view; out[4] = ways;
  out[5] = (int64_t)geo.ws.slab_stride; out[6] = Rmax; out[7] = rmax;
  return 0;
}

int omc_last_shor_dual_bound_ms(omc_instance* h, double* ms) {
  if (!h || !ms) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  *ms = h->sdb_ms;
  return 0;
}

int omc_shor_dual_bound_batch(omc_instance* h, int B, int cut_type, int reference_quirk_q1, const int* L, const double* cut_x, const double* cut_Uhat,
                              const int8_t* cut_dir, const double* U_lower, const double* U_upper, const int64_t* n_shor, const int64_t* shor_idx,
                              const int64_t* n_soc, const int64_t* soc_idx, int sanitise, int64_t nq_stride, const double* scale, const double* lam,
                              const double* Psi3, const double* Gam, const double* zeta, const double* xi, const double* Xbar, double* bound,
                              double* defects, double* terms) {
  // ---- refusals, all on the host ------------------------------------------------------------------------------------------------------
  if (!h) return fail(OMC_ERR_ARGUMENT, "omc_shor_dual_bound_batch: handle is NULL");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "omc_shor_dual_bound_batch: B must be positive");
  { int rcc = check_cut_type(cut_type); if (rcc) return rcc; }
  if (!n_shor || !n_soc || !scale || !lam || !zeta || !xi || !Xbar || !bound)
    return fail(OMC_ERR_ARGUMENT, "omc_shor_dual_bound_batch: n_shor, n_soc, scale, lam, zeta, xi, Xbar and bound are needed");
  if (h->worker.joinable() || h->worker_running.load()) return fail(OMC_ERR_ARGUMENT, "omc_shor_dual_bound_batch: a solve is in flight on this handle (call omc_relax_wait first)");
  if (h->k > 1) return fail(OMC_ERR_UNSUPPORTED, "omc_shor_dual_bound_batch: Shor-mode certificates exist for rank 1 only (quirk Q5 makes the minors vacuous for k > 1)");
  const size_t n = h->n, m = h->m, nm = n * m;
  if ((long long)n * (long long)m >= (1ll << 30)) return fail(OMC_ERR_UNSUPPORTED, "Shor mode: n * m too large for the 32-bit index structures");
  ShorGrouping grp;
  { int rc0 = shor_list_offsets(B, n_shor, shor_idx, n_soc, soc_idx, grp.so, grp.co); if (rc0) return rc0; }
  int64_t nqall = 0;
  for (int b = 0; b < B; ++b) nqall = std::max(nqall, n_shor[b]);
  if (nq_stride < nqall) return fail(OMC_ERR_ARGUMENT, "omc_shor_dual_bound_batch: nq_stride is below the longest minor list");
  if (nqall > 0 && !Gam) return fail(OMC_ERR_ARGUMENT, "omc_shor_dual_bound_batch: Gam is NULL but n_shor > 0");
  const size_t nqs = (size_t)nq_stride;
  // identical (minor list, SOC list) pairs share one index structure
  if (h->tun.shor_index_device_min > 0) {      // built on the device: ctype comes back for the defects below
    HIPCHK(hipSetDevice(h->device));
    grp.index_min = h->tun.shor_index_device_min; grp.stream = h->stream; grp.want_ctype = defects != nullptr;
  }
  { int rc0 = group_shor_lists(h, B, n_shor, shor_idx, n_soc, soc_idx, nullptr, grp); if (rc0) return rc0; }
  const std::vector<ShorGroupHost>& gh = grp.groups; const std::vector<int>& node_group = grp.node_group;
  const int NG = (int)gh.size(), nqmax = grp.nqmax, nv1max = grp.nv1max, nv2max = grp.nv2max;
  omc_relax_params P = h->params; P.reference_quirk_q1 = reference_quirk_q1 ? 1 : 0;
  NodePack pk;
  { int rcp = pack_nodes(h, P, cut_type, B, L, cut_x, cut_Uhat, cut_dir, U_lower, U_upper, pk); if (rcp) return rcp; }
  const size_t Rmax = pk.Rmax, rmax = pk.rmax, ps = (rmax + 1) * (rmax + 1);
  // ---- host part: which nodes live, lam clamped, PSD part of Psi3, the three defects that need no block --------------------------------
  const double NINF = -INFINITY;
  std::vector<uint8_t> live(B, 1);
  std::vector<double> hlam((size_t)B * Rmax, 0.0), hPsi(Psi3 ? (size_t)B * ps : 0, 0.0);
  for (int b = 0; b < B; ++b) {
    const int R = (int)pk.rk[b].size(), N3 = pk.rrv[b] + 1;
    const double* lb = lam + (size_t)b * Rmax;
    const double scb = scale[b];
    if (!(scb > 0.0 && scb - scb == 0.0)) live[b] = 0;      // not positive and finite: -inf, no device work for this node
    double min_lam = 0.0, psi_min = 0.0, min_zeta = 0.0;
    for (int r = 0; r < R; ++r) {
      if (!(lb[r] - lb[r] == 0.0)) live[b] = 0;
      min_lam = (r == 0) ? lb[r] : std::min(min_lam, lb[r]);
      hlam[(size_t)b * Rmax + r] = sanitise ? std::max(lb[r], 0.0) : lb[r];
    }
    if (Psi3) {
      const double* Pb = Psi3 + (size_t)b * ps;
      double* Ph = hPsi.data() + (size_t)b * ps;
      bool fin = true;
      for (int e = 0; e < N3 * N3; ++e) { Ph[e] = Pb[e]; fin = fin && (Pb[e] - Pb[e] == 0.0); }
      if (!fin) live[b] = 0;
      else if (sanitise || defects) {
        std::vector<double> S((size_t)N3 * N3), wv, Vv;
        for (int c = 0; c < N3; ++c) for (int r = 0; r < N3; ++r) S[(size_t)c * N3 + r] = 0.5 * (Pb[(size_t)c * N3 + r] + Pb[(size_t)r * N3 + c]);
        host_jacobi(N3, S, wv, Vv);
        psi_min = *std::min_element(wv.begin(), wv.end());
        if (sanitise)
          for (int c = 0; c < N3; ++c) for (int r = 0; r < N3; ++r) {
            double acc = 0.0;
            for (int i = 0; i < N3; ++i) acc += std::max(wv[i], 0.0) * Vv[(size_t)i * N3 + r] * Vv[(size_t)i * N3 + c];
            Ph[(size_t)c * N3 + r] = acc;
          }
      }
    }
    if (defects) {
      const std::vector<uint8_t>& ct = gh[node_group[b]].ctype;
      bool any = false;
      for (size_t j = 0; j < m; ++j) if (ct[j] != 2) { const double z = zeta[(size_t)b * m + j]; min_zeta = any ? std::min(min_zeta, z) : z; any = true; }
      double* d = defects + 5 * (size_t)b;
      d[0] = n_shor[b] > 0 ? NAN : 0.0; d[1] = n_shor[b] > 0 ? NAN : 0.0; d[2] = min_zeta; d[3] = min_lam; d[4] = psi_min;
    }
    bound[b] = NINF;
    if (terms) for (int q = 0; q < 4; ++q) terms[4 * (size_t)b + q] = NAN;
  }
  // ---- views: every live node as given (way 0); with sanitise and a non-empty list also with the negative part of its blocks removed (way 1) ----
  std::vector<int> view_node, view_way;
  for (int b = 0; b < B; ++b) {
    if (!live[b]) continue;
    view_node.push_back(b); view_way.push_back(0);
    if (sanitise && n_shor[b] > 0) { view_node.push_back(b); view_way.push_back(1); }
  }
  const int V = (int)view_node.size();
  if (V == 0) return 0;
  const size_t sV = (size_t)V, sB = (size_t)B;
  NodePack pv;
  std::vector<int> Lv(V, 0); std::vector<double> cxv;
  {
    std::vector<size_t> cutoff(B + 1, 0);
    for (int b = 0; b < B; ++b) cutoff[b + 1] = cutoff[b] + (size_t)(L ? L[b] : 0);
    pv.rk.resize(V); pv.rc.resize(V); pv.rbi.resize(V); pv.rbj.resize(V); pv.rcoef.resize(V); pv.rrhs.resize(V); pv.Qn.resize(V); pv.rrv.resize(V);
    for (int v = 0; v < V; ++v) {
      const int b = view_node[v];
      pv.rk[v] = pk.rk[b]; pv.rc[v] = pk.rc[b]; pv.rbi[v] = pk.rbi[b]; pv.rbj[v] = pk.rbj[b]; pv.rcoef[v] = pk.rcoef[b]; pv.rrhs[v] = pk.rrhs[b];
      pv.Qn[v] = pk.Qn[b]; pv.rrv[v] = pk.rrv[b];
      Lv[v] = L ? L[b] : 0;
      if (Lv[v] > 0) cxv.insert(cxv.end(), cut_x + cutoff[b] * n, cut_x + cutoff[b + 1] * n);
    }
    pv.Rmax = pk.Rmax; pv.rmax = pk.rmax; pv.Lmax = pk.Lmax;
  }
  // ---- device buffers of this call ---------------------------------------------------------------------------------------------------
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const bool want_clean = nqmax > 0 && (sanitise || defects);
  const bool store_clean = nqmax > 0 && sanitise;
  OmcWS w;
  const EvalDims d = eval_view_dims(h, w, V, 1, pk);
  ShorCertWS c;
  memset(&c, 0, sizeof(c));
  c.n = (int)n; c.m = (int)m; c.B = B; c.V = V; c.nmb = (nqmax + SCERT_T - 1) / SCERT_T; c.nv1max = nv1max; c.nv2max = nv2max; c.clamp_zeta = sanitise ? 1 : 0;
  c.nqs = (long long)nqs; c.gamma = h->gamma;
  const size_t nmb = (size_t)c.nmb;
  const ScertDims sd = {sB, nqs, nmb, (size_t)nv1max, (size_t)nv2max, m, w.geo.ws.slab_stride, store_clean};
  ScertArrays in{}; EvalArrays a{};
  int* arena_int = nullptr; uint8_t* arena_byte = nullptr; ShorGroupDev* groups_dev = nullptr;      // index structures of the call's distinct lists
  {
    size_t dbytes = 0;
    int rca = carve_ensure(h->sdD, [&](Carve& cv) { walk_scert_doubles(cv, sd, d, c, in, w, a); }, &dbytes);
    if (!rca) rca = carve_ensure(h->sdI, [&](Carve& cv) { walk_scert_ints(cv, sd, d, c, in, w, a); });
    if (!rca) rca = bind(h->sdGi, arena_int, grp.tot_int);
    if (!rca) rca = bind(h->sdGb, arena_byte, grp.tot_byte);
    if (!rca) rca = bind(h->sdGr, groups_dev, (size_t)NG);
    if (rca) {
      (void)hipGetLastError();
      return fail(OMC_ERR_ALLOC, "omc_shor_dual_bound_batch: the evaluation needs " + std::to_string(dbytes) + " bytes for " + std::to_string(V) +
                                 " views of " + std::to_string(B) + " nodes, which the device does not have (" + g_err + ")");
    }
  }
  { int rc = eval_view_zero(w, a, s); if (rc) return rc; }
  // index structures
  {
    ShorGroupImages img;
    { int rc = upload_shor_groups(h, grp, arena_int, arena_byte, groups_dev, in.node_group, s, img); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(in.view_node, view_node.data(), sizeof(int) * sV, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(in.view_way, view_way.data(), sizeof(int) * sV, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));          // the host images die with this block
  }
  c.groups = groups_dev; c.A = h->dA.as<double>(); c.mask = h->dmask.as<uint8_t>();
  { int rc = put_descriptors(w, pv, V, sV, 0, Lv.data(), cxv.empty() ? nullptr : cxv.data(), s); if (rc) return rc; }
  // multipliers: the caller's per node, lam and Psi3 (made admissible above when asked) per view
  std::vector<double> vlam(sV * Rmax, 0.0), vPsi(Psi3 ? sV * ps : 0, 0.0);
  for (int v = 0; v < V; ++v) {
    const size_t b = view_node[v];
    std::copy(hlam.begin() + b * Rmax, hlam.begin() + (b + 1) * Rmax, vlam.begin() + (size_t)v * Rmax);
    if (Psi3) std::copy(hPsi.begin() + b * ps, hPsi.begin() + (b + 1) * ps, vPsi.begin() + (size_t)v * ps);
  }
  HIPCHK(hipMemcpyAsync(in.scale, scale, sB * 8, hipMemcpyHostToDevice, s));
  if (nqmax > 0) HIPCHK(hipMemcpyAsync(in.Gam, Gam, sB * 15 * nqs * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(in.zeta, zeta, sB * m * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(in.xi, xi, sB * nm * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(in.Xbar, Xbar, sB * nm * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(a.lam, vlam.data(), sV * Rmax * 8, hipMemcpyHostToDevice, s));
  if (Psi3) HIPCHK(hipMemcpyAsync(a.Psi, vPsi.data(), sV * ps * 8, hipMemcpyHostToDevice, s));
  // ---- kernels ------------------------------------------------------------------------------------------------------------------------
  EventPair ev;
  HIPCHK(ev.create());
  HIPCHK(hipEventRecord(ev.e0, s));
  if (want_clean) omc_scert_launch_clean(&c, store_clean ? 1 : 0, s);
  if (nqmax > 0) { omc_scert_launch_keys(&c, s); omc_scert_launch_minor(&c, s); }
  omc_scert_launch_cols(&c, s);
  const OmcDualIn din = {nullptr, a.lam, Psi3 ? a.Psi : nullptr, a.T1, c.c0col, c.colbad};
  omc_launch_dual_assemble(&w, &din, s);
  std::vector<double> scl, cmu(sV * m), mpart(sV * nmb * 2 + 1), cpart(sB * nmb + 1);
  std::vector<int> cbad(sV * m);
  { int rc = eval_view_solve(w, a, ev.e1, scl, s); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(cmu.data(), c.colmu, sV * m * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(cbad.data(), c.colbad, sV * m * sizeof(int), hipMemcpyDeviceToHost, s));
  if (nmb && defects) {
    HIPCHK(hipMemcpyAsync(mpart.data(), c.minpart, sV * nmb * 2 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cpart.data(), c.cleanpart, sB * nmb * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  { float msf = 0.f; HIPCHK(hipEventElapsedTime(&msf, ev.e0, ev.e1)); h->sdb_ms = msf; }
  // ---- the host's part of the result: -inf rules, the larger of the two ways, back to the node's scale ---------------------------------
  const size_t o_cpen = w.cpen - w.c0, o_cst = w.cst - w.c0, o_ev = w.evsum - w.c0;      // where the walk placed them behind c0
  for (int v = 0; v < V; ++v) {
    const size_t b = view_node[v];
    double val = (scl[v] + scl[o_cst + v]) + scl[o_ev + v] - scl[o_cpen + v];      // (c0 + cst) + evsum - cpen
    double mumin = INFINITY;
    for (size_t j = 0; j < m; ++j) {
      if (cbad[(size_t)v * m + j]) val = NINF;
      mumin = std::min(mumin, cmu[(size_t)v * m + j]);
    }
    if (!(val - val == 0.0)) val = NINF;      // NaN or +-inf on the way
    const double out = (val == NINF) ? NINF : val / (scale[b] * scale[b]);
    const bool first = view_way[v] == 0;
    if (first || out > bound[b] || (out == bound[b] && view_way[v] == 1)) {
      bound[b] = out;
      if (terms) { double* t = terms + 4 * b; t[0] = scl[v] + scl[o_cst + v]; t[1] = scl[o_ev + v]; t[2] = scl[o_cpen + v]; t[3] = mumin; }
    }
    if (defects && first && n_shor[b] > 0) {
      const size_t nblk = ((size_t)n_shor[b] + SCERT_T - 1) / SCERT_T;
      double lo = INFINITY, res = 0.0;
      for (size_t t = 0; t < nblk; ++t) { lo = std::min(lo, cpart[b * nmb + t]); res = std::max(res, mpart[((size_t)v * nmb + t) * 2 + 1]); }
      defects[5 * b] = lo; defects[5 * b + 1] = res;
    }
  }
  return 0;
}
