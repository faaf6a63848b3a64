// omc_api.cpp -- host side of libomc_hip.so: the C ABI declared in include/omc.h, one source per area (omc_api_*.cpp; what they share:
// omc_api_internal.h).  This one: omc_last_error, the instance (omc_instance_*), the knobs (omc_tuning_*), base staging (omc_relax_stage,
// omc_relax_reserve, omc_set_node_rho_scales), the state pool (omc_state_pool_create, omc_relax_set_warm), omc_relax_append and the one append
// path, omc_relax_hold, omc_relax_submit / poll / wait, the fetches (omc_relax_fetch, omc_relax_fetch_done), omc_relax_batch and the
// omc_last_* / omc_debug_* getters of the base engine.
//
// Mirrors the call sites of the reference driver (OMC.jl = the reference driver's src/OptimalMatrixCompletion.jl):
//   omc_relax_*            <- matrix_completion_SDP_relaxation  OMC.jl:1431-1943 (called at 747-754)
// Argument checks reproduce the reference's `error(...)` conditions and return negative codes instead of
// throwing.  No torch types, no host pointer retained after return.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>
#include <algorithm>
#include <atomic>
#include <thread>
#include <mutex>
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include "omc_altmin.h"
#include "omc_api_internal.h"

thread_local std::string g_err;

static void knob_set(Tuning& t, const Knob& kb, const char* value) {      // value NULL: the default
  if (kb.flag) t.*kb.flag = value != nullptr;
  else t.*kb.num = value ? atoi(value) : Tuning{}.*kb.num;
}
// diagnostics (OMC_SEGV_TRACE=1 at instance creation): print the native frames of a crashing thread before the default action runs
static void omc_segv_trace(int sig) {
  void* fr[64];
  const int nf = backtrace(fr, 64);
  const char msg[] = "libomc_hip: fatal signal, native frames:\n";
  (void)!write(2, msg, sizeof(msg) - 1);
  backtrace_symbols_fd(fr, nf, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}
static void tuning_from_env(Tuning& t) {
  for (const Knob& kb : OMC_KNOBS) knob_set(t, kb, getenv(kb.name));
}

const char* omc_last_error(void) { return g_err.c_str(); }
int omc_version(void) { return OMC_VERSION; }
int omc_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

void omc_relax_params_default(omc_relax_params* p) {
  p->eps_gap = 1e-6; p->eps_feas = 1e-7; p->max_iters = 3000; p->check_every = 25;
  p->rho_scale = 1.0; p->rho_f_ratio = 0.1; p->relax = 1.6; p->time_limit = 3600.0;
  p->reference_quirk_q1 = 1; p->breakpoints = OMC_SMALLEST_1_EIGVEC; p->stall_checks = 8;
  p->bump_max = 2; p->bump_ratio = 4.0; p->bump_factor = 4.0; p->bump_after = 100; p->bump_window = 4; p->slots = 0;
  p->accel = 0; p->aa_mem = 10; p->aa_every = 10; p->aa_start = 50; p->aa_reg = 1e-10; p->aa_safeguard = 1.0; p->first_wins = 0;
  p->early_stop_after = 400; p->early_stop_factor = 1.5;
}

int upload(DevBuf& b, const void* src, size_t bytes, hipStream_t s) {
  int rc = b.ensure(bytes ? bytes : 8);
  if (rc) return rc;
  if (bytes) HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
  return 0;
}

// Column lists of the column prox for a value of OMC_COLPROX_BLOCK_MIN.  With the pair kernel on, a pair (2p, 2p + 1) of columns with at most
// 32 observed rows each belongs to k_colprox_pair whatever block_min says (that kernel selects its pairs itself).  Of the other non-empty
// columns, those with block_min <= c <= cp_block_cmax() are block columns (LDS list up to cp_block_lds_cmax() rows, slab list above); the rest
// go to k_colprox_wide (c <= 64) or stay with k_colprox, as before.
static int build_colprox_lists(omc_instance* h, int block_min, bool pair_on) {
  if (h->lists_valid && h->lists_block_min == block_min && h->lists_pair == pair_on) return 0;
  const int m = h->m, lds_c = cp_block_lds_cmax(), max_c = cp_block_cmax();
  std::vector<int> solo, wide, blk, slab;
  std::vector<uint8_t> isb(m, 0);
  h->cpb_cl = h->cpb_cs = h->crest_max = h->nrest = 0;
  for (int j0 = 0; j0 < m; j0 += 2) {
    const int j1 = j0 + 1;
    const int c0 = h->col_ptr[j0 + 1] - h->col_ptr[j0], c1 = (j1 < m) ? h->col_ptr[j1 + 1] - h->col_ptr[j1] : 0;
    const bool paired = j1 < m && c0 <= 32 && c1 <= 32;
    for (int j = j0; j <= j1 && j < m; ++j) {
      const int c = (j == j0) ? c0 : c1;
      if (c == 0) continue;
      if (!(paired && pair_on) && c >= block_min && c <= max_c) {
        isb[j] = 1;
        if (c <= lds_c) { blk.push_back(j); h->cpb_cl = std::max(h->cpb_cl, c); } else { slab.push_back(j); h->cpb_cs = std::max(h->cpb_cs, c); }
        continue;
      }
      ++h->nrest; h->crest_max = std::max(h->crest_max, c);
      if (paired) continue;
      if (c <= 64) wide.push_back(j); else solo.push_back(j);
    }
  }
  h->nsolo = (int)solo.size(); h->nwide = (int)wide.size(); h->nblock = (int)blk.size(); h->nslab = (int)slab.size();
  int rc = 0;
  if (h->nsolo && (rc = upload(h->dsolo, solo.data(), sizeof(int) * solo.size(), h->stream))) return rc;
  if (h->nwide && (rc = upload(h->dwide, wide.data(), sizeof(int) * wide.size(), h->stream))) return rc;
  if (h->nblock && (rc = upload(h->dblock, blk.data(), sizeof(int) * blk.size(), h->stream))) return rc;
  if (h->nslab && (rc = upload(h->dslab, slab.data(), sizeof(int) * slab.size(), h->stream))) return rc;
  if ((rc = upload(h->disblock, isb.data(), (size_t)m, h->stream))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));      // the vectors die with this call
  h->lists_valid = true; h->lists_block_min = block_min; h->lists_pair = pair_on;
  return 0;
}

int omc_instance_create(int n, int m, int k, const double* A, const uint8_t* mask, double gamma, int device,
                        omc_instance** out) {
  if (!out) return fail(OMC_ERR_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (!A || !mask) return fail(OMC_ERR_ARGUMENT, "A / mask is NULL");
  if (n <= 0 || m <= 0) return fail(OMC_ERR_DIMENSION, "Dimension mismatch: A must have size (n, m) (OMC.jl:240-246)");
  if (!(n <= m)) return fail(OMC_ERR_DIMENSION, "Input matrix A must have size (n, m) with n <= m (OMC.jl:249-254)");
  if (k < 1 || k > n) return fail(OMC_ERR_ARGUMENT, "rank k must satisfy 1 <= k <= n");
  if (k > 8) return fail(OMC_ERR_UNSUPPORTED, "k > 8 is not supported by this build");
  if (!(gamma > 0.0)) return fail(OMC_ERR_ARGUMENT, "gamma must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(OMC_ERR_NO_DEVICE, "no HIP device visible: the HIP path is the product, there is no CPU fallback");
  if (device < 0 || device >= ndev) return fail(OMC_ERR_ARGUMENT, "device index out of range");
  HIPCHK(hipSetDevice(device));
  omc_instance* h = new omc_instance();
  tuning_from_env(h->tun);
  if (h->tun.segv_trace) { signal(SIGSEGV, omc_segv_trace); signal(SIGABRT, omc_segv_trace); }
  struct Guard { omc_instance*& p; ~Guard() { if (p) omc_instance_destroy(p); } } guard{h};     // every early return below frees the handle
  h->n = n; h->m = m; h->k = k; h->gamma = gamma; h->device = device;
  { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) h->wall_khz = khz; else (void)hipGetLastError(); }
  h->A.assign(A, A + (size_t)n * m);
  h->mask.resize((size_t)n * m);
  for (size_t e = 0; e < (size_t)n * m; ++e) h->mask[e] = mask[e] ? 1 : 0;
  h->col_ptr.assign(m + 1, 0);
  for (int j = 0; j < m; ++j) {
    int c = 0;
    for (int i = 0; i < n; ++i)
      if (h->mask[(size_t)j * n + i]) { h->col_idx.push_back(i); h->col_val.push_back(A[(size_t)j * n + i]); ++c; }
    h->col_ptr[j + 1] = h->col_ptr[j] + c;
    h->cmax = std::max(h->cmax, c);
  }
  h->nnz = h->col_ptr[m];
  h->sumA2 = 0;
  for (double v : h->col_val) h->sumA2 += v * v;
  h->Ncnt.assign((size_t)n * n, 0.0);
  for (int j = 0; j < m; ++j)
    for (int p = h->col_ptr[j]; p < h->col_ptr[j + 1]; ++p)
      for (int q = h->col_ptr[j]; q < h->col_ptr[j + 1]; ++q)
        h->Ncnt[(size_t)h->col_idx[q] * n + h->col_idx[p]] += 1.0;
  // CSR copy (rows -> observed columns) for the U-step of altmin
  h->row_ptr.assign(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    int c = 0;
    for (int j = 0; j < m; ++j)
      if (h->mask[(size_t)j * n + i]) { h->row_idx.push_back(j); h->row_val.push_back(A[(size_t)j * n + i]); ++c; }
    h->row_ptr[i + 1] = h->row_ptr[i] + c;
  }
  HIPCHK(hipStreamCreate(&h->stream));
  int rc = 0;
  if ((rc = upload(h->drow_ptr, h->row_ptr.data(), sizeof(int) * (n + 1), h->stream))) return rc;
  if ((rc = upload(h->drow_idx, h->row_idx.data(), sizeof(int) * h->nnz_rows(), h->stream))) return rc;
  if ((rc = upload(h->drow_val, h->row_val.data(), sizeof(double) * h->nnz_rows(), h->stream))) return rc;
  if ((rc = upload(h->dA, h->A.data(), sizeof(double) * n * m, h->stream))) return rc;
  if ((rc = upload(h->dmask, h->mask.data(), (size_t)n * m, h->stream))) return rc;
  if ((rc = upload(h->dcol_ptr, h->col_ptr.data(), sizeof(int) * (m + 1), h->stream))) return rc;
  if ((rc = build_colprox_lists(h, h->tun.colprox_block_min, !h->tun.no_colprox_pair))) return rc;
  if ((rc = upload(h->dcol_idx, h->col_idx.data(), sizeof(int) * h->nnz, h->stream))) return rc;
  if ((rc = upload(h->dcol_val, h->col_val.data(), sizeof(double) * h->nnz, h->stream))) return rc;
  if ((rc = upload(h->dNcnt, h->Ncnt.data(), sizeof(double) * n * n, h->stream))) return rc;
  {      // objective cutoff: off.  The memory omc_relax_set_cutoff needs exists from here on, so that it never allocates.  Its stream does not:
         // a stream created here would take a hardware queue ahead of the three iteration streams (measured: -4.7 % on the default bench with
         // the cutoff never set); the first omc_relax_set_cutoff creates it, as the append and fetch streams are created by their first call
    ENS(h->bcutoff, sizeof(double));
    int prc = h->pin_cutoff.ensure(sizeof(double)); if (prc) return prc;
    *h->pin_cutoff.as<double>() = HUGE_VAL;
    HIPCHK(hipMemcpyAsync(h->bcutoff.p, h->pin_cutoff.p, sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  int lrc = omc_set_max_lds();
  if (lrc) return fail(lrc, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  { int arc = omc_altmin_set_lds(); if (arc) return fail(5000 + arc, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for the altmin kernel"); }
  omc_relax_params_default(&h->params);
  *out = h;
  h = nullptr;          // released to the caller (the guard holds a reference to this pointer)
  return 0;
}

int omc_instance_create_bits(int n, int m, int k, const double* A, const uint64_t* chunks, double gamma, int device,
                             omc_instance** out) {
  if (!chunks) return fail(OMC_ERR_ARGUMENT, "chunks is NULL");
  if (n <= 0 || m <= 0) return fail(OMC_ERR_DIMENSION, "Dimension mismatch (OMC.jl:240-246)");
  std::vector<uint8_t> mask((size_t)n * m);
  for (size_t e = 0; e < (size_t)n * m; ++e) mask[e] = (uint8_t)((chunks[e >> 6] >> (e & 63)) & 1ull);
  return omc_instance_create(n, m, k, A, mask.data(), gamma, device, out);
}

void omc_instance_destroy(omc_instance* h) {
  if (!h) return;
  if (h->worker.joinable()) h->worker.join();
  (void)hipSetDevice(h->device);
  (void)omc_comm_destroy(h);
  for (hipStream_t q : {h->stream, h->gs[0], h->gs[1], h->gs[2], h->append_stream, h->fetch_stream, h->cutoff_stream}) if (q) (void)hipStreamDestroy(q);
  for (int q = 0; q < 2; ++q) for (hipEvent_t e : h->ev_pool[q]) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->ev_up) if (e) (void)hipEventDestroy(e);
  if (h->ev_gram) (void)hipEventDestroy(h->ev_gram);
  for (int q = 0; q < 5; ++q) for (hipEvent_t e : {h->gev[q], h->gevc[q]}) if (e) (void)hipEventDestroy(e);
  if (h->ev_main) (void)hipEventDestroy(h->ev_main);
  delete h;      // the device buffers free themselves
}

// (the piece table of the disjunctive cuts, cut_piece: omc_cut_piece.h, shared with the device)

// rows (OMC.jl:1558-1685) and row subspace of a set of nodes, on the host: shared by omc_relax_stage and omc_relax_append
int pack_nodes(omc_instance* h, const omc_relax_params& P, int cut_type, int B, const int* L, const double* cut_x, const double* cut_Uhat,
                      const int8_t* cut_dir, const double* U_lower, const double* U_upper, NodePack& pk) {
  const int n = h->n, k = h->k;
  // ---- rows (host) -----------------------------------------------------------------------------------
  int Lmax = 0; long Ltot = 0;
  for (int b = 0; b < B; ++b) {
    int Lb = L ? L[b] : 0;
    if (Lb < 0) return fail(OMC_ERR_ARGUMENT, "negative cut count");
    Lmax = std::max(Lmax, Lb); Ltot += Lb;
  }
  if (Ltot > 0 && (!cut_x || !cut_Uhat || !cut_dir)) return fail(OMC_ERR_ARGUMENT, "cut arrays are NULL but L > 0");
  // box rows: entries whose bound is not implied by ||U_j|| <= 1 (OMC.jl:1561, defaults 1442-1449)
  auto& rk = pk.rk; auto& rc = pk.rc; auto& rbi = pk.rbi; auto& rbj = pk.rbj; auto& rcoef = pk.rcoef; auto& rrhs = pk.rrhs;
  rk.assign(B, {}); rc.assign(B, {}); rbi.assign(B, {}); rbj.assign(B, {}); rcoef.assign(B, {}); rrhs.assign(B, {});
  int Rmax = 0;
  long cutbase = 0;
  for (int b = 0; b < B; ++b) {
    auto add = [&](int kind, int cut, int bi, int bj, const double* coef, double rhs) {
      rk[b].push_back(kind); rc[b].push_back(cut); rbi[b].push_back(bi); rbj[b].push_back(bj);
      for (int j = 0; j < k; ++j) rcoef[b].push_back(coef ? coef[j] : 0.0);
      rrhs[b].push_back(rhs);
    };
    add(ROW_TRACE, -1, -1, -1, nullptr, (double)k);                                 // OMC.jl:1558
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < n; ++i) {
        double lo = U_lower ? U_lower[(size_t)b * n * k + (size_t)j * n + i] : ((i >= n - k + j) ? 0.0 : -1.0);
        double hi = U_upper ? U_upper[(size_t)b * n * k + (size_t)j * n + i] : 1.0;
        if (lo > hi) return fail(OMC_ERR_ARGUMENT, "U_lower > U_upper");
        double cf[8] = {0};
        if (lo > -1.0) { cf[0] = -1.0; add(ROW_BOX, -1, i, j, cf, -lo); }
        if (hi < 1.0) { cf[0] = 1.0; add(ROW_BOX, -1, i, j, cf, hi); }
      }
    const int Lb = L ? L[b] : 0;
    for (int l = 0; l < Lb; ++l) {
      const double* x = cut_x + (size_t)(cutbase + l) * n;
      const double* Uh = cut_Uhat + (size_t)(cutbase + l) * n * k;
      const int8_t* dr = cut_dir + (size_t)(cutbase + l) * k;
      double slope[8], icsum = 0.0;
      for (int j = 0; j < k; ++j) {
        double vhat = 0.0;                                                         // OMC.jl:1577
        for (int i = 0; i < n; ++i) vhat += Uh[(size_t)j * n + i] * x[i];
        double lo, hi, sl, ic;
        if (cut_piece(cut_type, dr[j], vhat, P.reference_quirk_q1, &lo, &hi, &sl, &ic))
          return fail(OMC_ERR_INVALID_ENUM, "direction code invalid for this cut type (OMC.jl:1580-1678)");
        slope[j] = -sl; icsum += ic;
        double cf[8] = {0};
        cf[j] = 1.0; add(ROW_BOUND, l, -1, j, cf, hi);                              // v_j <= hi
        cf[j] = -1.0; add(ROW_BOUND, l, -1, j, cf, -lo);                            // -v_j <= -lo
      }
      add(ROW_CUT, l, -1, -1, slope, icsum);                                        // OMC.jl:1680-1683
    }
    cutbase += Lb;
    Rmax = std::max(Rmax, (int)rk[b].size());
  }
  // ---- subspace of the U functionals: modified Gram-Schmidt (twice) over the row vectors in row order ------
  auto& Qn = pk.Qn; auto& rrv = pk.rrv;
  Qn.assign(B, {}); rrv.assign(B, 0);
  int rmax = 1;
  cutbase = 0;
  for (int b = 0; b < B; ++b) {
    std::vector<double>& Qv = Qn[b];
    int r = 0;
    std::vector<double> v(n);
    const int Lb = L ? L[b] : 0;
    for (size_t rw = 0; rw < rk[b].size(); ++rw) {
      const int kind = rk[b][rw];
      if (kind == ROW_TRACE) continue;
      for (int j = 0; j < k; ++j) {
        const double cf = rcoef[b][rw * k + j];
        bool nz = false;
        if (kind == ROW_BOX) {
          if (j != rbj[b][rw]) continue;
          std::fill(v.begin(), v.end(), 0.0); v[rbi[b][rw]] = rcoef[b][rw * k] > 0 ? 1.0 : -1.0; nz = true;
        } else if (cf != 0.0) {
          const double* x = cut_x + (size_t)(cutbase + rc[b][rw]) * n;
          double nx = 0.0;
          for (int i = 0; i < n; ++i) nx += x[i] * x[i];
          nx = sqrt(nx) * fabs(cf);
          if (nx > 0) { for (int i = 0; i < n; ++i) v[i] = cf * x[i] / nx; nz = true; }
        }
        if (!nz) continue;
        for (int pass = 0; pass < 2; ++pass)
          for (int a = 0; a < r; ++a) {
            double d = 0.0;
            for (int i = 0; i < n; ++i) d += Qv[(size_t)a * n + i] * v[i];
            for (int i = 0; i < n; ++i) v[i] -= d * Qv[(size_t)a * n + i];
          }
        double nv = 0.0;
        for (int i = 0; i < n; ++i) nv += v[i] * v[i];
        nv = sqrt(nv);
        if (nv > 1e-10 && r < n) {
          Qv.resize((size_t)(r + 1) * n);
          for (int i = 0; i < n; ++i) Qv[(size_t)r * n + i] = v[i] / nv;
          ++r;
        }
      }
    }
    rrv[b] = r; rmax = std::max(rmax, r);
    cutbase += Lb;
  }
  pk.Rmax = Rmax; pk.rmax = rmax; pk.Lmax = Lmax;
  return 0;
}

// row, cut and Q descriptors of the B nodes of `pk` (padded to the workspace's Rmax rows, Lmax cuts and rmax subspace columns) into the per-node
// arrays of the workspace from node `first` on: `rows` >= B nodes are written, those beyond B zero (omc_relax_stage writes every row up to the
// capacity, omc_relax_append its own rows only)
int put_descriptors(const OmcWS& w, const NodePack& pk, int B, size_t rows, size_t first, const int* L, const double* cut_x, hipStream_t s) {
  const size_t n = w.n, k = w.k, Rm = w.Rmax, Lm = w.Lmax, rm = w.rmax;
  std::vector<int> hR(rows, 0), hrr(rows, 0), hk(rows * Rm, 0), hc(rows * Rm, 0), hbi(rows * Rm, 0), hbj(rows * Rm, 0);
  std::vector<double> hcoef(rows * Rm * k, 0.0), hrhs(rows * Rm, 0.0), hx(rows * Lm * n, 0.0), hQ(rows * n * rm, 0.0);
  long cutbase = 0;
  for (int b = 0; b < B; ++b) {
    hR[b] = (int)pk.rk[b].size();
    for (int r = 0; r < hR[b]; ++r) {
      hk[(size_t)b * Rm + r] = pk.rk[b][r]; hc[(size_t)b * Rm + r] = pk.rc[b][r];
      hbi[(size_t)b * Rm + r] = pk.rbi[b][r]; hbj[(size_t)b * Rm + r] = pk.rbj[b][r];
      hrhs[(size_t)b * Rm + r] = pk.rrhs[b][r];
      for (size_t j = 0; j < k; ++j) hcoef[((size_t)b * Rm + r) * k + j] = pk.rcoef[b][(size_t)r * k + j];
    }
    const int Lb = L ? L[b] : 0;
    for (int l = 0; l < Lb; ++l) memcpy(&hx[((size_t)b * Lm + l) * n], cut_x + (size_t)(cutbase + l) * n, sizeof(double) * n);
    cutbase += Lb;
    memcpy(&hQ[(size_t)b * n * rm], pk.Qn[b].data(), sizeof(double) * pk.Qn[b].size());
    hrr[b] = pk.rrv[b];
  }
  HIPCHK(hipMemcpyAsync(w.R + first, hR.data(), sizeof(int) * hR.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.rkind + first * Rm, hk.data(), sizeof(int) * hk.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.rcut + first * Rm, hc.data(), sizeof(int) * hc.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.rbi + first * Rm, hbi.data(), sizeof(int) * hbi.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.rbj + first * Rm, hbj.data(), sizeof(int) * hbj.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.rcoef + first * Rm * k, hcoef.data(), 8 * hcoef.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.rrhs + first * Rm, hrhs.data(), 8 * hrhs.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.cutx + first * Lm * n, hx.data(), 8 * hx.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.Qb + first * n * rm, hQ.data(), 8 * hQ.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(w.rr + first, hrr.data(), sizeof(int) * hrr.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));          // the host arrays die with this call
  return 0;
}

// fixed parameters of the eigen-kernels and the column kernel (OmcWS fields; MAX_SWEEPS: omc_host.h)
static constexpr int CP_SERIES = 6;            // Neumann-series order of k_colprox_pair's finish
static constexpr int CP_MAXPASS = 60;          // cap on the secular passes of k_colprox_pair
static constexpr int SUB_GUARD = 2;            // Ritz values of the tracked block that must stay negative
static constexpr int SUB_CHUNK = 3;            // power steps per chunk of k_cone_sub
static constexpr double SUB_TOL = 1e-10;       // residual floor of k_cone_sub
static constexpr double SUB_ADAPT = 1e-3;      // residual target of k_cone_sub relative to the last dual residual

int check_cut_type(int cut_type) {
  if (cut_type != OMC_CUT_LINEAR && cut_type != OMC_CUT_LINEAR2 && cut_type != OMC_CUT_LINEAR3)
    return fail(OMC_ERR_INVALID_ENUM, "Invalid input for disjunctive cuts type: must be linear, linear2 or linear3 (OMC.jl:1456-1462)");
  return 0;
}

int stage_base(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L, const double* cut_x, const double* cut_Uhat,
                      const int8_t* cut_dir, const double* U_lower, const double* U_upper, const StageMode& mode) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  { int rcc = check_cut_type(cut_type); if (rcc) return rcc; }
  HIPCHK(hipSetDevice(h->device));
  h->staged = false;
  const bool shor = mode.shor;
  h->shor_on = false; h->shor_via_base = false;
  if (params) h->params = *params; else omc_relax_params_default(&h->params);
  if (shor) {      // the bound of a Shor node lags its primal value for the first ~1000 iterations: no early stop, a longer stall window, one bump
    h->params.early_stop_factor = 0.0;
    h->params.stall_checks = std::max(h->params.stall_checks, 40);
    h->params.bump_max = std::min(h->params.bump_max, 1);
    h->params.first_wins = 0; h->params.accel = 0;
  }
  const omc_relax_params& P = h->params;
  if (P.breakpoints != OMC_SMALLEST_1_EIGVEC && P.breakpoints != OMC_SMALLEST_2_EIGVEC)
    return fail(OMC_ERR_INVALID_ENUM, "Invalid input for disjunctive cuts breakpoints (OMC.jl:2440-2446)");
  const int n = h->n, m = h->m, k = h->k;
  // ---- rows and row subspaces (host) ---------------------------------------------------------------------
  NodePack pk;
  { int rcp = pack_nodes(h, P, cut_type, B, L, cut_x, cut_Uhat, cut_dir, U_lower, U_upper, pk); if (rcp) return rcp; }
  int Rmax = pk.Rmax, rmax = pk.rmax, Lmax = pk.Lmax;
  // omc_relax_reserve: room for nodes appended later (default U bounds, at most reserve_cuts cuts each)
  const int extra_nodes = h->reserve_nodes, extra_cuts = h->reserve_cuts;
  h->reserve_nodes = 0; h->reserve_cuts = 0;
  if (extra_nodes > 0) {
    Lmax = std::max(Lmax, extra_cuts);
    Rmax = std::max(Rmax, 1 + k * (k + 1) / 2 + extra_cuts * (2 * k + 1));
    rmax = std::max(rmax, std::min(n, k + extra_cuts));
  }
  // ---- workspace -------------------------------------------------------------------------------------
  OmcWS& w = h->ws;
  memset(&w, 0, sizeof(w));
  // continuous batching: S slots relax B nodes; a slot that finishes is harvested and re-used for the next pending node
  const int Bcap = B + extra_nodes;      // with omc_relax_reserve the slots are sized for the nodes that may still come
  const int S = (P.slots > 0) ? std::min(P.slots, Bcap) : std::min(Bcap, 256);
  h->Btot = B; h->Btot_live.store(B); h->node_cap = B + extra_nodes; h->staged_cut_type = cut_type; { std::lock_guard<std::mutex> lk(h->append_mu); h->append_closed = false; }
  { std::lock_guard<std::mutex> lk(h->done_mu); h->done_q.clear(); h->done_read = 0; }
  h->hold.store(0);
  w.cutoff = h->bcutoff.as<double>();      // the memset above cleared it; the value behind it is the handle's and is not touched here
  w.nB = S;
  w.B = S; w.Btot = B; w.max_iters = P.max_iters; w.n = n; w.m = m; w.k = k; w.nnz = h->nnz; w.Rmax = Rmax; w.Lmax = std::max(Lmax, 1); w.rmax = rmax;
  w.max_sweeps = MAX_SWEEPS;
  w.breakpoints = P.breakpoints; w.stall_checks = P.stall_checks > 0 ? P.stall_checks : 1000000;
  w.gamma = h->gamma; w.sumA2 = h->sumA2;
  {
    const double sh = 1.0 + h->gamma * (double)k / (double)n;
    w.rho = P.rho_scale * 0.5 * h->gamma * h->sumA2 / ((double)m * sh * sh);
  }
  if (shor) w.rho = h->shor_rho * P.rho_scale;      // penalty of the cone blocks in the scaled variables of the Shor splitting
  if (!(w.rho > 0.0)) w.rho = 1.0;
  w.clip_hi = 1.0; w.inv_s2 = 1.0; w.shor = 0;
  w.rho_f_ratio = P.rho_f_ratio;
  w.bump_max = P.bump_max; w.bump_ratio = P.bump_ratio; w.bump_factor = P.bump_factor; w.bump_after = P.bump_after;
  w.bump_gap = P.bump_window * std::max(1, P.check_every);
  w.accel = P.accel ? 1 : 0; w.aa_mem = std::max(2, std::min(P.aa_mem, AA_MAXMEM)); w.aa_every = std::max(1, P.aa_every);
  w.aa_start = std::max(2, P.aa_start); w.aa_reg = P.aa_reg; w.aa_safeguard = P.aa_safeguard;
  {
    std::vector<double> hr((size_t)B + extra_nodes, w.rho);
    if (h->rho_scale_per_node.size() == (size_t)B)
      for (int b = 0; b < B; ++b) hr[b] = w.rho / P.rho_scale * h->rho_scale_per_node[b];
    h->rho_scale_per_node.clear();
    int r0 = upload(h->brhon, hr.data(), sizeof(double) * hr.size(), h->stream); if (r0) return r0;
    HIPCHK(hipStreamSynchronize(h->stream));          // hr dies with this block: the copy must have read it
    w.rho_node = h->brhon.as<double>();
    BIND(h->brho, w.rho_b, (size_t)S);
  }
  w.relax = P.relax; w.eps_gap = P.eps_gap; w.eps_feas = P.eps_feas;
  w.check_every = std::max(1, P.check_every); w.early_stop_after = P.early_stop_after; w.early_stop_factor = (P.first_wins ? 0.0 : P.early_stop_factor);
  // what the packed buffers below are carved by (omc_walks.h): state arrays one per slot, descriptor and output arrays one per node (plus
  // the room reserved for appended nodes)
  const StageDims sd = {(size_t)S, (size_t)B + (size_t)extra_nodes, (size_t)n, (size_t)m, (size_t)k, (size_t)h->nnz, (size_t)rmax, (size_t)Rmax};
  {
    ENS_CARVE(h->bgap, [&](Carve& c) { walk_gap(c, sd, w); });
    BIND(h->bvotes, w.slow_votes, (size_t)S);
    ENS(h->bslotlist, sizeof(int) * (size_t)S);
    w.slot_list = nullptr;      // set on the per-iteration copies only (omc_relax_solve): the buffer has no pointer in the staged workspace
  }
  std::vector<double> wY((size_t)n * n);
  for (size_t e = 0; e < (size_t)n * n; ++e) wY[e] = shor ? 3.0 : P.rho_f_ratio * h->Ncnt[e] + 2.0;      // Shor mode: big cone, clip, small cone
  int rc_ = 0;
  if ((rc_ = upload(h->dwY, wY.data(), sizeof(double) * n * n, h->stream))) return rc_;
  w.col_ptr = h->dcol_ptr.as<int>(); w.col_idx = h->dcol_idx.as<int>(); w.col_val = h->dcol_val.as<double>();
  {
    const bool pair_on = !h->tun.no_colprox_pair && mode.colprox_force != 2;
    if ((rc_ = build_colprox_lists(h, mode.colprox_force == 1 ? INT_MAX : mode.colprox_force == 2 ? 1 : h->tun.colprox_block_min, pair_on))) return rc_;
    w.cp_pair = pair_on ? 1 : 0;
  }
  w.cp_nblock = h->nblock; w.cp_block = h->nblock ? h->dblock.as<int>() : nullptr;
  w.cp_nslab = h->nslab; w.cp_slab = h->nslab ? h->dslab.as<int>() : nullptr;
  w.cp_isblock = (h->nblock + h->nslab) ? h->disblock.as<unsigned char>() : nullptr; w.cp_nrest = h->nrest; w.cp_nfact = nullptr;
  w.cone_512 = h->tun.cone_512 ? 1 : 0; w.cp_series = CP_SERIES; w.cp_maxpass = CP_MAXPASS; w.cp_xcd = h->tun.colprox_no_xcd ? 0 : 1;
  w.cp_dpp = h->tun.colprox_dpp ? 1 : 0;
  w.cp_nsolo = h->nsolo; w.cp_solo = h->nsolo ? h->dsolo.as<int>() : nullptr;
  w.cp_nwide = h->nwide; w.cp_wide = h->nwide ? h->dwide.as<int>() : nullptr;
  w.Ncnt = h->dNcnt.as<double>(); w.wY1 = h->dwY.as<double>();
  w.row_ptr = h->drow_ptr.as<int>(); w.row_idx = h->drow_idx.as<int>();
  const size_t sB = (size_t)S;      // state arrays: one per slot
  const size_t sN = (size_t)B + (size_t)extra_nodes;      // descriptor and output arrays: one per node (plus the room reserved for appended nodes)
  // the arrays that own a buffer each, one statement per array: buffer, workspace pointer, elements, and the stream where it starts zeroed
  hipStream_t s0 = h->stream;
  const size_t nn = (size_t)n * n, nk = (size_t)n * k, nz = (size_t)h->nnz;
  BIND(h->bY, w.Y, sB * nn); BIND(h->bYp, w.Yp, sB * nn); BIND(h->bU, w.U, sB * nk);
  BIND(h->bD1, w.D1, sB * nn); BIND(h->bD3, w.D3, sB * nn); BIND(h->bW1, w.W1, sB * nn); BIND(h->bE3, w.E3, sB * nn);
  BIND(h->bdS, w.dS, sB * rmax * rmax);
  ENS_CARVE(h->bsm, [&](Carve& c) { walk_small_cone(c, sd, w); });
  BIND(h->balpha, w.alpha, sB * nz); BIND(h->balphaX, w.alphaX, sB * nz); BIND(h->bsval, w.sval, sB * m);
  BIND(h->bMchk, w.Mchk, sB * nn);
  size_t chk_bytes = 0;
  ENS_CARVE(h->bchk, [&](Carve& c) { walk_check(c, sd, w); }, &chk_bytes);
  BIND(h->bG, w.G, sB * Rmax * Rmax); BIND(h->blam, w.lam, sB * Rmax);
  ENS_CARVE(h->bscal, [&](Carve& c) { walk_scalars(c, sd, w); });
  BIND(h->bbx, w.bx, sB * n);
  ENS_CARVE(h->bint, [&](Carve& c) { walk_slot_ints(c, sd, w); });
  w.np16 = (n + 15) & ~15;
  const size_t pp = (size_t)w.np16 * w.np16, p16 = (size_t)w.np16 * 16;
  BIND(h->bMbuf, w.Mbuf, sB * pp); BIND(h->bVrow, w.Vrow, sB * pp);
  BIND(h->blamD, w.lamD, sB * m * n, s0);
  w.lamDX = nullptr;
  if (n > 144 || shor) BIND(h->blamDX, w.lamDX, sB * m * n, s0);      // large orders: the certificate matrix takes Lambda Lambda' from one MFMA product
  {   // tracked subspace of the cone block (k_cone_sub)
    size_t subS_bytes = 0, subI_bytes = 0;
    BIND(h->bXs, w.Xs, sB * p16, s0);
    ENS_CARVE(h->bsubS, [&](Carve& c) { walk_sub_doubles(c, sd, w); }, &subS_bytes);
    ENS_CARVE(h->bsubI, [&](Carve& c) { walk_sub_ints(c, sd, w); }, &subI_bytes);      // w1_fac (factored W1): kept or dropped below, once k_global's variant is known
    HIPCHK(hipMemsetAsync(h->bsubS.p, 0, subS_bytes, s0));
    HIPCHK(hipMemsetAsync(h->bsubI.p, 0, subI_bytes, s0));
    w.ws_phase = 0;
    w.sub_guard = SUB_GUARD; w.sub_qmax = h->tun.sub_qmax; w.sub_chunk = SUB_CHUNK;
    w.sub_tol = SUB_TOL; w.sub_adapt = SUB_ADAPT; w.sub_debug = h->tun.sub_debug;
    w.sub_enable = 0;     // decided below, once the cone kernel variant is known
    size_t subSC_bytes = 0, subIC_bytes = 0;
    BIND(h->bXsC, w.XsC, sB * p16, s0);
    ENS_CARVE(h->bsubSC, [&](Carve& c) { walk_subC_doubles(c, sd, w); }, &subSC_bytes);
    ENS_CARVE(h->bsubIC, [&](Carve& c) { walk_subC_ints(c, sd, w); }, &subIC_bytes);      // sep_done: kept or dropped below with sub_enable
    HIPCHK(hipMemsetAsync(h->bsubSC.p, 0, subSC_bytes, s0));
    HIPCHK(hipMemsetAsync(h->bsubIC.p, 0, subIC_bytes, s0));
    w.cert_enable = 0;
  }
  // warm-started eigenvalues for the certificate matrix.  VrowC: its zero padding feeds the branch-free K loop of the MFMA GEMM, 0 x garbage could be NaN
  BIND(h->bMbufC, w.MbufC, sB * pp, s0); BIND(h->bVrowC, w.VrowC, sB * pp, s0); BIND(h->bchkS, w.fro2c, sB); BIND(h->bchkI, w.vvalidC, sB, s0);
  w.Yx = nullptr;
  if (!shor && !P.accel) BIND(h->bYx, w.Yx, sB * nn);      // 2 Y - Yp for the column gathers (k_aa rewrites Y and Yp behind k_global's back)
  // with Yx the column kernels never read Yp (k_aa and the Shor kernels, its only other readers, run without Yx; k_setup rewrites it at
  // every start; the state pool does not keep it): k_global stops storing it
  w.skip_yp = (w.Yx && !h->tun.dense_proj) ? 1 : 0;
  ENS_CARVE(h->bobjcol, [&](Carve& c) { walk_objcol(c, sd, w); });
  if (w.accel) {
    w.aa_dim = 4 * n * n + 2 * rmax * k + k * k + h->nnz;
    const size_t ring = sB * (size_t)(w.aa_mem + 1) * w.aa_dim;
    size_t aaI_bytes = 0;
    BIND(h->baaF, w.aa_F, ring); BIND(h->baaG, w.aa_G, ring); BIND(h->baaZ, w.aa_zin, sB * (size_t)w.aa_dim); BIND(h->baaS, w.aa_fn, sB);
    ENS_CARVE(h->baaI, [&](Carve& c) { walk_aa_ints(c, sd, w); }, &aaI_bytes);
    HIPCHK(hipMemsetAsync(h->baaI.p, 0, aaI_bytes, s0));
  }
  HIPCHK(hipMemsetAsync(w.ws_need, 0, sizeof(int), s0));
  {
    size_t map_bytes = 0;
    ENS_CARVE(h->bslotint, [&](Carve& c) { walk_slot_map(c, sd, w.node_of, w.init, w.fin); }, &map_bytes);
    std::vector<int> hs(map_bytes / sizeof(int));      // the host image of the three arrays, laid out by the same walk
    int *h_node = nullptr, *h_init = nullptr, *h_fin = nullptr;
    { Carve hc(hs.data()); walk_slot_map(hc, sd, h_node, h_init, h_fin); }
    for (size_t b = 0; b < sB; ++b) { h_node[b] = (int)b; h_init[b] = 1; h_fin[b] = 1; }   // identity map, every slot initialises
    HIPCHK(hipMemcpyAsync(h->bslotint.p, hs.data(), map_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));          // hs dies with this block
    BIND(h->boY, w.oY, sN * nn); BIND(h->boU, w.oU, sN * nk); BIND(h->boal, w.oalphaX, sN * nz); BIND(h->bobx, w.obx, sN * n);
    ENS_CARVE(h->boscal, [&](Carve& c) { walk_out_scalars(c, sd, w); });
    ENS_CARVE(h->boint, [&](Carve& c) { walk_out_ints(c, sd, w); });
  }
  if ((h->keep_cert && !shor) || (h->keep_shor_cert && shor)) {      // best certificate per node: slot buffers and the arena of the nodes, zeroed (no slot and no node holds one)
    const size_t cnnz = shor ? 0 : (size_t)h->nnz;      // Shor mode has no alphaX: its own multipliers are kept by omc_relax_stage_shor (ShWS::cbGam ...)
    size_t cbD_bytes = 0, cbI_bytes = 0, ocD_bytes = 0;
    ENS_CARVE(h->bcbD, [&](Carve& c) { walk_cert_slot(c, sd, cnnz, w); }, &cbD_bytes);
    ENS_CARVE(h->bcbI, [&](Carve& c) { walk_cert_flags(c, sd, w); }, &cbI_bytes);
    ENS_CARVE(h->bocD, [&](Carve& c) { walk_cert_node(c, sd, cnnz, w); }, &ocD_bytes);
    BIND(h->bocI, w.ocHave, sN, s0);
    HIPCHK(hipMemsetAsync(h->bcbD.p, 0, cbD_bytes, s0)); HIPCHK(hipMemsetAsync(h->bcbI.p, 0, cbI_bytes, s0));
    HIPCHK(hipMemsetAsync(h->bocD.p, 0, ocD_bytes, s0));
    if (shor) { w.cbLam = nullptr; w.ocLam = nullptr; }
  }
  // warm-start indices of this batch (consumed: they belong to this stage call only)
  w.load_from = nullptr; w.save_to = nullptr;
  const bool warm_ok = !shor || mode.warm_filtered;
  if (h->pool_cap > 0 && warm_ok && extra_nodes > 0) {      // appended nodes may name pool entries: both index arrays exist, -1 where nothing was given
    if (h->warm_load.size() != (size_t)B) h->warm_load.assign(B, -1);
    if (h->warm_save.size() != (size_t)B) h->warm_save.assign(B, -1);
    h->warm_load.resize(sN, -1); h->warm_save.resize(sN, -1);
  } else if (extra_nodes == 0) {
    if (h->warm_load.size() != (size_t)B) h->warm_load.clear();
    if (h->warm_save.size() != (size_t)B) h->warm_save.clear();
  }
  h->save_host.assign(sN, -1);
  // cuts, rows and row-subspace columns per node on the host, and with room for appended nodes in base mode the scratch of the branch kernels
  // (omc_relax_append_children): sized here, so that an append never allocates
  h->node_L.assign(sN, 0); h->node_R.assign(sN, 0); h->node_r.assign(sN, 0);
  for (int b = 0; b < B; ++b) { h->node_L[b] = L ? L[b] : 0; h->node_R[b] = (int)pk.rk[b].size(); h->node_r[b] = pk.rrv[b]; }
  h->br_ready = false;
  if (extra_nodes > 0 && !shor) {
    BranchWS bw{};
    ENS_CARVE(h->bbrS, [&](Carve& c) { walk_branch_scratch(c, BRANCH_CHUNK, (size_t)n, (size_t)k, bw); });
    ENS_CARVE(h->bbrI, [&](Carve& c) { walk_branch_ints(c, BRANCH_CHUNK, BRANCH_CHUNK, (size_t)k, bw); });
    h->br_ready = true;
  }
  if (h->pool_cap > 0 && !shor && h->warm_load.size() == sN) {      // entries saved by a Shor solve do not hold what the base engine loads (alpha, sval)
    std::lock_guard<std::mutex> lk(h->sig_mu);
    for (int& e : h->warm_load) if (e >= 0 && (size_t)e < h->pool_sig.size() && h->pool_sig[e].kind == 2) e = -1;
  }
  if (h->pool_cap > 0 && warm_ok && (h->warm_load.size() == sN || h->warm_save.size() == sN)) {
    if (h->warm_save.size() == sN) h->save_host = h->warm_save;
    if (h->warm_load.size() == sN) { if ((rc_ = upload(h->bwarmL, h->warm_load.data(), sizeof(int) * sN, h->stream))) return rc_; w.load_from = h->bwarmL.as<int>(); }
    if (h->warm_save.size() == sN) { if ((rc_ = upload(h->bwarmS, h->warm_save.data(), sizeof(int) * sN, h->stream))) return rc_; w.save_to = h->bwarmS.as<int>(); }
    HIPCHK(hipStreamSynchronize(h->stream));
    w.pY = h->pY.as<double>(); w.pD1 = h->pD1.as<double>(); w.pD3 = h->pD3.as<double>(); w.pU = h->pU.as<double>(); w.palpha = h->palpha.as<double>();
    w.psval = h->psval.as<double>(); w.pXs = h->pXs.as<double>(); w.ptheta = h->ptheta.as<double>(); w.pscal = h->pscal.as<double>();
  }
  h->warm_load.clear(); h->warm_save.clear();
  // Q, row and cut descriptors, one row per node up to the capacity
  BIND(h->bQb, w.Qb, sN * n * rmax); BIND(h->brr, w.rr, sN); BIND(h->bR, w.R, sN);
  BIND(h->brkind, w.rkind, sN * Rmax); BIND(h->brcut, w.rcut, sN * Rmax); BIND(h->brbi, w.rbi, sN * Rmax); BIND(h->brbj, w.rbj, sN * Rmax);
  BIND(h->brcoef, w.rcoef, sN * Rmax * k); BIND(h->brrhs, w.rrhs, sN * Rmax); BIND(h->bcutx, w.cutx, sN * w.Lmax * n);
  if ((rc_ = put_descriptors(w, pk, B, sN, 0, L, cut_x, h->stream))) return rc_;
  // LDS / scratch decisions: one planner (omc_layout.h), the slabs allocated from the strides it reports
  w.geo = omc_plan_geometry(n, w.np16, k, rmax, Rmax, h->cmax, h->tun.global_nolds, h->tun.cone_multi_min, h->tun.plain_multi_min);
  BIND(h->bmwstat, w.mw_stat, sB * 4, s0);
  w.mw_budget = MAX_SWEEPS; w.ev_out = nullptr;
  w.pmw_stat = nullptr;
  if (w.geo.plain_mw) BIND(h->bpmwstat, w.pmw_stat, sB * 4, s0);
  // k_colprox_block: the dynamic LDS of its launches and the slab of the columns beyond the LDS, for those columns only.  The slab of
  // colprox_body (one block per slot and column) is sized by the longest column that still runs it
  geom_set_cpblock(w.geo, h->cpb_cl, h->cpb_cs);
  w.geo.cp_scratch_stride = h->crest_max > w.geo.cp_lds_c ? cp_body_layout(h->crest_max).doubles : 0;
  if (w.geo.cpb_slab_stride && !shor) BIND(h->bcpb, w.cp_bslab, sB * h->nslab * w.geo.cpb_slab_stride);
  if (w.geo.cp_scratch_stride) BIND(h->bcp, w.cp_scratch, sB * m * w.geo.cp_scratch_stride);
  if (w.geo.ws.slab_stride) BIND(h->bcone, w.cone_scratch, sB * w.geo.ws.slab_stride);
  if (w.geo.glob.slab_stride) BIND(h->bglob, w.glob_scratch, sB * w.geo.glob.slab_stride);
  if (w.geo.small.slab_stride) BIND(h->bsmall, w.small_scratch, sB * w.geo.small.slab_stride);
  // subspace tracking needs the warm-started kernel as its seed / fall-back and at least 3 x 16 rows
  w.sub_enable = (w.geo.ws_lpp && n >= 48 && w.geo.sub_lds <= OMC_MAX_DYN_LDS && !h->tun.no_subspace) ? 1 : 0;
  w.sub_zscratch = nullptr;
  if (w.sub_enable && w.np16 > 512) BIND(h->bsubz, w.sub_zscratch, sB * 16 * (size_t)(w.np16 + 2));
  w.cert_enable = (w.sub_enable && w.np16 > 512) ? 1 : 0;      // large orders: the certificate eigenvalues by the tracked block too (rigorous confirmation before anything is reported)
  if (!w.sub_enable) w.sep_done = nullptr;
  // factored W1 (OmcWS::w1_fac): k_global stages the accepted Ritz vectors of a slot in its NNQP scratch (LDS variant only; glob_w1_fits).
  // Off in Shor mode (its W1 views are other arrays) and with OMC_DENSE_PROJ=1.
  if (!(!shor && w.sub_enable && w.geo.glob.use_lds && glob_w1_fits(n) && !h->tun.dense_proj)) w.w1_fac = nullptr;
  HIPCHK(hipMemsetAsync(w.sweeps, 0, sizeof(int) * S, s0));
  HIPCHK(hipMemsetAsync(w.stamps, 0, (size_t)((char*)h->bchk.p + chk_bytes - (char*)w.stamps), s0));      // from stamps to the end of the walk
  HIPCHK(hipStreamSynchronize(h->stream));
  h->staged = true;
  return 0;
}

int omc_relax_stage(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L,
                    const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower,
                    const double* U_upper) {
  return stage_base(h, B, params, cut_type, L, cut_x, cut_Uhat, cut_dir, U_lower, U_upper, StageMode{});
}

int omc_set_node_rho_scales(omc_instance* h, int B, const double* rho_scale) {
  if (!h || B <= 0 || !rho_scale) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  for (int b = 0; b < B; ++b) if (!(rho_scale[b] > 0.0)) return fail(OMC_ERR_ARGUMENT, "rho_scale must be positive");
  h->rho_scale_per_node.assign(rho_scale, rho_scale + B);
  return 0;
}

// ---- warm start: a child is its parent plus one cut.  The caller keeps a pool of final states on the device and tells the
// next staged batch which entry each node starts from (its parent's) and where its own final state goes.  The reference rebuilds and cold-starts
// every model (OMC.jl:1482); this is an addition of the engine, off unless asked for.
int omc_state_pool_create(omc_instance* h, int capacity) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (capacity < 0) return fail(OMC_ERR_ARGUMENT, "capacity must be non-negative");
  HIPCHK(hipSetDevice(h->device));
  const size_t c = (size_t)capacity, n = h->n, k = h->k, np16 = (h->n + 15) & ~15;
  if (capacity > 0) {
    ENS(h->pY, c * n * n * 8); ENS(h->pD1, c * n * n * 8); ENS(h->pD3, c * n * n * 8); ENS(h->pU, c * n * k * 8); ENS(h->palpha, c * (size_t)h->nnz * 8);
    ENS(h->psval, c * (size_t)h->m * 8); ENS(h->pXs, c * np16 * 16 * 8); ENS(h->ptheta, c * 16 * 8); ENS(h->pscal, c * 4 * 8);
  }
  h->pool_cap = capacity;
  { std::lock_guard<std::mutex> lk(h->sig_mu); h->pool_sig.assign(c, omc_instance::PoolSig{}); }
  h->pool_shor = false; h->pool_nqmax = 0;      // the extension is sized per entry: reserve it again for the new capacity
  return 0;
}

int omc_relax_set_warm(omc_instance* h, int B, const int* load_from, const int* save_to) {
  if (!h || B <= 0) return fail(OMC_ERR_ARGUMENT, "omc_relax_set_warm: bad arguments");
  if (h->pool_cap <= 0) return fail(OMC_ERR_ARGUMENT, "omc_relax_set_warm: no state pool (omc_state_pool_create)");
  h->warm_load.clear(); h->warm_save.clear();
  for (int b = 0; b < B; ++b) {
    if (load_from && load_from[b] >= h->pool_cap) return fail(OMC_ERR_ARGUMENT, "load_from index beyond the pool");
    if (save_to && save_to[b] >= h->pool_cap) return fail(OMC_ERR_ARGUMENT, "save_to index beyond the pool");
  }
  if (load_from) h->warm_load.assign(load_from, load_from + B);
  if (save_to) h->warm_save.assign(save_to, save_to + B);
  return 0;
}

// ---- appending nodes to a staged / running batch ------------------------------------------------------------------------------------------
// The reference's loop pops one node at a time from a queue that children keep filling (OMC.jl:700-719, 2520-2542); a staged batch is closed.
// omc_relax_reserve(h, extra_nodes, max_cuts) makes the NEXT omc_relax_stage size its per-node arrays for extra_nodes more nodes with at most
// max_cuts cuts each (default U bounds); omc_relax_append then adds nodes -- before omc_relax_solve / omc_relax_submit or while the submitted
// solve is running (the loop hands them to slots at its next check) -- until the solve has ended, after which it is refused.
int omc_relax_reserve(omc_instance* h, int extra_nodes, int max_cuts) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (extra_nodes < 0 || max_cuts < 0) return fail(OMC_ERR_ARGUMENT, "omc_relax_reserve: negative argument");
  h->reserve_nodes = extra_nodes; h->reserve_cuts = max_cuts;
  return 0;
}

// The one append path: omc_relax_append, and with `lists` omc_relax_append_shor, whose list step (known lists share their group, new ones
// are built and may be refused) sits between the checks and the writes; with `refs` omc_relax_append_children, whose nodes are given by
// reference: branch_check stands in for pack_nodes and its stride check, branch_write (two kernels) for put_descriptors.  Lock, end-of-batch decision, capacity, rows, strides and pool
// indices first: every refusal is decided before anything is written, and a refused call leaves the batch as it was.  Then the new groups,
// the descriptors, rho_node and the warm-start indices on the append stream, and the counter last: the running kernels read the
// descriptors of nodes below Btot_live only, so these rows are not visible to them until it moves.
int append_nodes(omc_instance* h, const char* who, int B2, const int* L, const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir,
                 const int* load_from, const int* save_to, const ShorAppendLists* lists, const BranchRefs* refs) {
  const std::string pre = std::string(who) + ": ";
  HIPCHK(hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(h->append_mu);
  if (h->append_closed) return fail(OMC_ERR_ARGUMENT, pre + "the solve of this batch has ended (stage a new batch)");
  const OmcWS& w = h->ws;
  const int first = h->Btot_live.load();
  if (first + B2 > h->node_cap) return fail(OMC_ERR_ARGUMENT, pre + (lists ? "beyond the node capacity given to omc_relax_reserve" : "beyond the capacity given to omc_relax_reserve"));
  NodePack pk;      // nodes given by reference (refs) have no pack: their rows are written on the device, their strides checked from the host copies
  if (refs) { int rcb = branch_check(h, first, B2, *refs, pre); if (rcb) return rcb; }
  else {
    { int rcp = pack_nodes(h, h->params, h->staged_cut_type, B2, L, cut_x, cut_Uhat, cut_dir, nullptr, nullptr, pk); if (rcp) return rcp; }
    if (pk.Rmax > w.Rmax || pk.rmax > w.rmax || pk.Lmax > w.Lmax) return fail(OMC_ERR_ARGUMENT, pre + "a node has more cuts than omc_relax_reserve allowed for");
  }
  if ((load_from || save_to) && !(w.load_from && w.save_to))
    return fail(OMC_ERR_ARGUMENT, pre + (lists ? "warm-start indices need a state pool with its Shor extension (omc_state_pool_reserve_shor) before the batch was staged"
                                               : "warm-start indices need a state pool created before the batch was staged"));
  for (int b = 0; b < B2; ++b) {
    if (load_from && load_from[b] >= h->pool_cap) return fail(OMC_ERR_ARGUMENT, "load_from index beyond the pool");
    if (save_to && save_to[b] >= h->pool_cap) return fail(OMC_ERR_ARGUMENT, "save_to index beyond the pool");
  }
  // warm-start indices as they are written (empty: that array is not): a base append writes what was given, without the entries that a Shor
  // solve saved (as at stage time); a Shor append writes both arrays once the batch has them, -1 where nothing was given, through its filter
  std::vector<int> lfv, svv;
  ShorGrouping grouping;
  if (!h->append_stream) HIPCHK(hipStreamCreateWithFlags(&h->append_stream, hipStreamNonBlocking));
  if (lists) {
    if (w.load_from && w.save_to) {
      lfv.assign(B2, -1); svv.assign(B2, -1);
      if (load_from) lfv.assign(load_from, load_from + B2);
      if (save_to) svv.assign(save_to, save_to + B2);
    }
    int rcl = shor_append_plan(h, first, B2, *lists, lfv, svv, grouping); if (rcl) return rcl;
  } else {
    if (load_from) {
      lfv.assign(load_from, load_from + B2);
      std::lock_guard<std::mutex> lk2(h->sig_mu);
      for (int& e : lfv) if (e >= 0 && (size_t)e < h->pool_sig.size() && h->pool_sig[e].kind == 2) e = -1;
    }
    if (save_to) svv.assign(save_to, save_to + B2);
  }
  hipStream_t as = h->append_stream;
  const size_t f = (size_t)first;
  ShorGroupImages img;
  if (lists) { int rcw = shor_append_write(h, grouping, first, as, img); if (rcw) return rcw; }
  if (refs) { int rc = branch_write(h, first, B2, *refs, as); if (rc) return rc; }
  else { int rc = put_descriptors(w, pk, B2, B2, f, L, cut_x, as); if (rc) return rc; }
  std::vector<double> hrho(B2, w.rho);
  HIPCHK(hipMemcpyAsync(const_cast<double*>(w.rho_node) + f, hrho.data(), 8 * (size_t)B2, hipMemcpyHostToDevice, as));
  if (!lfv.empty()) HIPCHK(hipMemcpyAsync(const_cast<int*>(w.load_from) + f, lfv.data(), sizeof(int) * B2, hipMemcpyHostToDevice, as));
  if (!svv.empty()) {
    HIPCHK(hipMemcpyAsync(const_cast<int*>(w.save_to) + f, svv.data(), sizeof(int) * B2, hipMemcpyHostToDevice, as));
    for (int b = 0; b < B2; ++b) h->save_host[f + b] = svv[b];      // sized for node_cap at stage time; read by the solve only below Btot_live
  }
  HIPCHK(hipStreamSynchronize(as));
  if (lists) shor_append_commit(h, grouping);
  // cuts, rows and row-subspace columns of the new nodes on the host (omc_relax_append_children decides its refusals from them)
  if (refs) branch_commit(h, first, B2, *refs);
  else if (h->node_L.size() >= f + (size_t)B2)
    for (int b = 0; b < B2; ++b) { h->node_L[f + b] = L ? L[b] : 0; h->node_R[f + b] = (int)pk.rk[b].size(); h->node_r[f + b] = pk.rrv[b]; }
  h->Btot_live.store(first + B2); h->Btot = first + B2;
  if (!h->worker_running.load()) { h->ws.Btot = first + B2; if (lists) h->sh.Btot = first + B2; }      // no solve in flight: the staged batch simply grew (a running solve sets both when it ends)
  return 0;
}

int omc_relax_append(omc_instance* h, int B2, const int* L, const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir,
                     const int* load_from, const int* save_to) {
  if (!h || !h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_append: nothing staged");
  if (B2 <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  if (h->shor_on) return fail(OMC_ERR_UNSUPPORTED, "omc_relax_append: the staged batch is in Shor mode (omc_relax_append_shor)");
  return append_nodes(h, "omc_relax_append", B2, L, cut_x, cut_Uhat, cut_dir, load_from, save_to, nullptr);
}

// ---- objective cutoff (include/omc.h) --------------------------------------------------------------------------------------------------------
// The setter may run beside the worker thread of a submitted solve: it owns the host value, its page-locked image and its stream, and reads
// or writes nothing the worker uses.  An aligned 8-byte copy racing with a check is benign: k_check_final sees the old or the new value, and
// both are cutoffs the caller gave.  When the call returns the device holds the value, so every check enqueued from then on reads it.
int omc_relax_set_cutoff(omc_instance* h, double cutoff) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (cutoff != cutoff) return fail(OMC_ERR_ARGUMENT, "omc_relax_set_cutoff: the cutoff is NaN");
  HIPCHK(hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(h->cutoff_mu);
  if (!h->cutoff_stream) HIPCHK(hipStreamCreateWithFlags(&h->cutoff_stream, hipStreamNonBlocking));
  if (cutoff != HUGE_VAL) h->cutoff_armed.store(1);      // before the copy: a check that sees the value also sees the flag
  *h->pin_cutoff.as<double>() = cutoff;
  HIPCHK(hipMemcpyAsync(h->bcutoff.p, h->pin_cutoff.p, sizeof(double), hipMemcpyHostToDevice, h->cutoff_stream));
  HIPCHK(hipStreamSynchronize(h->cutoff_stream));
  h->cutoff.store(cutoff);
  if (h->solve_active.load()) h->cutoff_live.fetch_add(1);
  return 0;
}

int omc_relax_get_cutoff(omc_instance* h, double* cutoff) {
  if (!h || !cutoff) return fail(OMC_ERR_ARGUMENT, "omc_relax_get_cutoff: NULL argument");
  *cutoff = h->cutoff.load();
  return 0;
}

int omc_last_cutoff_stats(omc_instance* h, int64_t out[4]) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "omc_last_cutoff_stats: NULL argument");
  out[0] = h->cutoff_nodes.load(); out[1] = h->cutoff_iters.load(); out[2] = h->cutoff_live.load(); out[3] = 0;
  return 0;
}

void cutoff_solve_begin(omc_instance* h) {
  std::lock_guard<std::mutex> lk(h->cutoff_mu);      // not between a setter's flag and its count
  h->cutoff_nodes.store(0); h->cutoff_iters.store(0); h->cutoff_live.store(0);
  h->cutoff_armed.store(h->cutoff.load() != HUGE_VAL ? 1 : 0);
  h->solve_active.store(1);
}

// omc_relax_hold(h, 1) after staging: the submitted solve does not end when every staged node has finished but waits for omc_relax_append
// (a queue-driven host creates the next nodes from the results of the last ones); omc_relax_hold(h, 0) lets it end once it runs dry.
int omc_relax_hold(omc_instance* h, int on) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  h->hold.store(on ? 1 : 0);
  return 0;
}

// Results of the nodes harvested since the last call, in harvest order -- also while the submitted solve is still running: with omc_relax_append
// this is the other half of a queue-driven host loop (OMC.jl:700-719: pop, relax, push the children).  node_ids[i] indexes the staged + appended
// nodes; U (n*k), lambda_min (2), breakpoint_x (n) and Y (n*n) per node as in omc_relax_fetch (NULL: not copied).  *n_out = nodes returned (<= max_nodes).
int omc_relax_fetch_done(omc_instance* h, int max_nodes, int* node_ids, double* objective, double* dual_bound, int* status, int* iters,
                         double* U, double* lambda_min, double* breakpoint_x, double* Y, int* n_out) {
  if (!h || !h->staged || !node_ids || !n_out) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_done: nothing staged or NULL argument");
  if (max_nodes < 0) return fail(OMC_ERR_ARGUMENT, "max_nodes is negative");
  HIPCHK(hipSetDevice(h->device));
  std::vector<int> ids;
  {
    std::lock_guard<std::mutex> lk(h->done_mu);
    const size_t avail = h->done_q.size() - h->done_read, take = std::min(avail, (size_t)max_nodes);
    ids.assign(h->done_q.begin() + h->done_read, h->done_q.begin() + h->done_read + take);
    h->done_read += take;
  }
  *n_out = (int)ids.size();
  if (ids.empty()) return 0;
  if (!h->fetch_stream) HIPCHK(hipStreamCreateWithFlags(&h->fetch_stream, hipStreamNonBlocking));
  hipStream_t fs = h->fetch_stream;
  const OmcWS& w = h->ws;
  const size_t n = h->n, k = h->k;
  for (size_t i = 0; i < ids.size(); ++i) {
    const size_t nb = (size_t)ids[i];
    node_ids[i] = ids[i];
    if (objective) HIPCHK(hipMemcpyAsync(objective + i, w.oobj + nb, 8, hipMemcpyDeviceToHost, fs));
    if (dual_bound) HIPCHK(hipMemcpyAsync(dual_bound + i, w.olb + nb, 8, hipMemcpyDeviceToHost, fs));
    if (status) HIPCHK(hipMemcpyAsync(status + i, w.ostatus + nb, 4, hipMemcpyDeviceToHost, fs));
    if (iters) HIPCHK(hipMemcpyAsync(iters + i, w.oiters + nb, 4, hipMemcpyDeviceToHost, fs));
    if (U) HIPCHK(hipMemcpyAsync(U + i * n * k, w.oU + nb * n * k, 8 * n * k, hipMemcpyDeviceToHost, fs));
    if (lambda_min) HIPCHK(hipMemcpyAsync(lambda_min + 2 * i, w.olmin + 2 * nb, 16, hipMemcpyDeviceToHost, fs));
    if (breakpoint_x) HIPCHK(hipMemcpyAsync(breakpoint_x + i * n, w.obx + nb * n, 8 * n, hipMemcpyDeviceToHost, fs));
    if (Y) HIPCHK(hipMemcpyAsync(Y + i * n * n, w.oY + nb * n * n, 8 * n * n, hipMemcpyDeviceToHost, fs));
  }
  HIPCHK(hipStreamSynchronize(fs));
  return 0;
}

// An id is known once omc_relax_fetch_done has returned it, or (unless upto_read_only) once the solve has ended and harvested it.
int require_finished_ids(omc_instance* h, int n_ids, const int* ids, bool upto_read_only, const char* who) {
  bool ended = false;
  if (!upto_read_only) { std::lock_guard<std::mutex> lk(h->append_mu); ended = h->append_closed; }
  std::lock_guard<std::mutex> lk(h->done_mu);
  std::vector<char> seen((size_t)std::max(h->node_cap, 1), 0);
  const size_t upto = ended ? h->done_q.size() : h->done_read;
  for (size_t i = 0; i < upto; ++i) if ((size_t)h->done_q[i] < seen.size()) seen[h->done_q[i]] = 1;
  for (int i = 0; i < n_ids; ++i)
    if (ids[i] < 0 || (size_t)ids[i] >= seen.size() || !seen[ids[i]])
      return fail(OMC_ERR_ARGUMENT, std::string(who) + ": node " + std::to_string(ids[i]) +
                                        (upto_read_only ? " is out of range or has not been returned by omc_relax_fetch_done"
                                                        : " is out of range or has not finished (omc_relax_fetch_done has not returned it)"));
  return 0;
}

int require_certificates(const OmcWS& w, int n_ids, const int* ids, hipStream_t fs, const char* who) {
  std::vector<int> have(n_ids, 0);
  for (int i = 0; i < n_ids; ++i) HIPCHK(hipMemcpyAsync(&have[i], w.ocHave + ids[i], sizeof(int), hipMemcpyDeviceToHost, fs));
  HIPCHK(hipStreamSynchronize(fs));
  for (int i = 0; i < n_ids; ++i)
    if (!have[i]) return fail(OMC_ERR_ARGUMENT, std::string(who) + ": node " + std::to_string(ids[i]) + " never reached a rigorous check (no certificate)");
  return 0;
}

// ---- asynchronous boundary: the solve runs on a worker thread of the library, the caller (the Julia task that owns the queue) keeps
// working -- popping, pruning, building the next batch -- and polls.  One solve in flight per handle; no other call on the handle
// except omc_relax_poll until omc_relax_wait has returned.
int omc_relax_submit(omc_instance* h) {
  if (!h || !h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_submit: nothing staged");
  if (h->worker.joinable()) return fail(OMC_ERR_ARGUMENT, "omc_relax_submit: a solve is already in flight (call omc_relax_wait first)");
  h->nodes_done.store(0); h->worker_running.store(1); h->worker_rc = 0; h->worker_err.clear();
  cutoff_solve_begin(h);      // here, not on the worker: an omc_relax_set_cutoff that follows this call is counted as taken while the solve ran
  h->worker = std::thread([h]() {
    const int rc = omc_relax_solve(h);
    h->worker_rc = rc;
    if (rc) h->worker_err = g_err;        // g_err is thread-local: hand the message to the thread that will call omc_relax_wait
    h->worker_running.store(0);
  });
  return 0;
}

int omc_relax_poll(omc_instance* h, int* running, int* nodes_done, int* nodes_total) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (running) *running = h->worker_running.load();
  if (nodes_done) *nodes_done = h->nodes_done.load();
  if (nodes_total) *nodes_total = h->Btot_live.load();
  return 0;
}

int omc_relax_wait(omc_instance* h) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (!h->worker.joinable()) return fail(OMC_ERR_ARGUMENT, "omc_relax_wait: no solve in flight");
  h->worker.join();
  if (h->worker_rc) g_err = h->worker_err;
  return h->worker_rc;
}

int omc_relax_fetch(omc_instance* h, double* objective, double* dual_bound, int* status, int* iters, double* Y,
                    double* U, double* X, double* Theta, double* lambda_min, double* breakpoint_x, double* solve_time) {
  if (!h || !h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch: nothing staged");
  HIPCHK(hipSetDevice(h->device));
  const OmcWS& w = h->ws;
  const size_t B = w.Btot, n = w.n, m = w.m, k = w.k;
  hipStream_t s = h->stream;
  if (objective) HIPCHK(hipMemcpyAsync(objective, w.oobj, 8 * B, hipMemcpyDeviceToHost, s));
  if (dual_bound) HIPCHK(hipMemcpyAsync(dual_bound, w.olb, 8 * B, hipMemcpyDeviceToHost, s));
  if (status) HIPCHK(hipMemcpyAsync(status, w.ostatus, 4 * B, hipMemcpyDeviceToHost, s));
  if (iters) HIPCHK(hipMemcpyAsync(iters, w.oiters, 4 * B, hipMemcpyDeviceToHost, s));
  if (Y) HIPCHK(hipMemcpyAsync(Y, w.oY, 8 * B * n * n, hipMemcpyDeviceToHost, s));
  if (U) HIPCHK(hipMemcpyAsync(U, w.oU, 8 * B * n * k, hipMemcpyDeviceToHost, s));
  if (lambda_min) HIPCHK(hipMemcpyAsync(lambda_min, w.olmin, 8 * 2 * B, hipMemcpyDeviceToHost, s));
  if (breakpoint_x) HIPCHK(hipMemcpyAsync(breakpoint_x, w.obx, 8 * B * n, hipMemcpyDeviceToHost, s));
  if (h->shor_on) {
    if (X) HIPCHK(hipMemcpyAsync(X, h->sh.oX, 8 * B * n * m, hipMemcpyDeviceToHost, s));
    if (Theta) HIPCHK(hipMemcpyAsync(Theta, h->sh.oTh, 8 * B * m * m, hipMemcpyDeviceToHost, s));
  } else if (X || Theta) {
    double *dX = nullptr, *dTh = nullptr;
    BIND(h->bXout, dX, B * n * m);
    omc_launch_make_X(&w, dX, s);
    if (X) HIPCHK(hipMemcpyAsync(X, dX, 8 * B * n * m, hipMemcpyDeviceToHost, s));
    if (Theta) {
      BIND(h->bThout, dTh, B * m * m);
      omc_launch_make_Theta(&w, dX, dTh, s);
      HIPCHK(hipMemcpyAsync(Theta, dTh, 8 * B * m * m, hipMemcpyDeviceToHost, s));
    }
  }
  HIPCHK(hipStreamSynchronize(s));
  if (solve_time) for (size_t b = 0; b < B; ++b) solve_time[b] = h->last_solve_seconds;
  // a status still SLOW/TIME here has values (OMC.jl:1871-1877): feasible = true for every node
  return 0;
}

int omc_relax_batch(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L,
                    const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower,
                    const double* U_upper, double* objective, double* dual_bound, int* status, int* iters, double* Y,
                    double* U, double* X, double* Theta, double* lambda_min, double* breakpoint_x, double* solve_time) {
  int rc = omc_relax_stage(h, B, params, cut_type, L, cut_x, cut_Uhat, cut_dir, U_lower, U_upper);
  if (rc) return rc;
  rc = omc_relax_solve(h);
  if (rc) return rc;
  return omc_relax_fetch(h, objective, dual_bound, status, iters, Y, U, X, Theta, lambda_min, breakpoint_x, solve_time);
}

int omc_debug_residuals(omc_instance* h, double* rp, double* rd) {
  if (!h || !rp || !rd || !h->ws.rp) return fail(OMC_ERR_ARGUMENT, "nothing staged");
  HIPCHK(hipMemcpy(rp, h->ws.rp, 8 * (size_t)h->ws.B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rd, h->ws.rd, 8 * (size_t)h->ws.B, hipMemcpyDeviceToHost));
  return 0;
}

int omc_tuning_set(omc_instance* h, const char* name, const char* value) {
  if (!h || !name) return fail(OMC_ERR_ARGUMENT, "omc_tuning_set: handle or name is NULL");
  for (const Knob& kb : OMC_KNOBS) if (!strcmp(kb.name, name)) { knob_set(h->tun, kb, value); return 0; }
  return fail(OMC_ERR_ARGUMENT, "omc_tuning_set: unknown knob");
}

int omc_tuning_reload_env(omc_instance* h) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  tuning_from_env(h->tun);
  return 0;
}

int omc_debug_stamps(omc_instance* h, double* out32) {
  if (!h || !out32 || !h->ws.stamps) return fail(OMC_ERR_ARGUMENT, "no stamps");
  if (h->tun.sub_debug == 3 && h->ws.B >= 8) {      // diagnostics: three histograms (tools/diagnostics/gpu_nkeep_hist.py passes 96 doubles)
    HIPCHK(hipMemcpy(out32, h->ws.stamps, 96 * 8, hipMemcpyDeviceToHost));
    return 0;
  }
  HIPCHK(hipMemcpy(out32, h->ws.stamps, 32 * 8, hipMemcpyDeviceToHost));
  return 0;
}

int omc_debug_aa(omc_instance* h, int* accepted, int* rejected) {
  if (!h || !accepted || !rejected || !h->ws.accel || !h->ws.aa_nacc) return fail(OMC_ERR_ARGUMENT, "acceleration is off or nothing staged");
  HIPCHK(hipMemcpy(accepted, h->ws.aa_nacc, 4 * (size_t)h->ws.B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rejected, h->ws.aa_nrej, 4 * (size_t)h->ws.B, hipMemcpyDeviceToHost));
  return 0;
}

int omc_debug_diag(omc_instance* h, double* out /* 8 * slots */) {
  if (!h || !out || !h->ws.stamps) return fail(OMC_ERR_ARGUMENT, "no diagnostics");
  HIPCHK(hipMemcpy(out, h->ws.stamps + 32, 8 * 8 * (size_t)h->ws.B, hipMemcpyDeviceToHost));
  return 0;
}

int omc_last_host_phases(omc_instance* h, double* ms, int64_t* count) {
  if (!h || !ms || !count) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  for (int q = 0; q < OMC_HOST_NPHASE; ++q) { ms[q] = h->host_ms[q]; count[q] = h->host_cnt[q]; }
  return 0;
}

int omc_last_solver_info(omc_instance* h, double* info) {
  if (!h || !info) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  info[0] = h->last_solve_seconds; info[1] = (double)h->total_sweeps; info[2] = h->ws.rho; info[3] = (double)h->ws.rmax;
  info[4] = (double)h->ws.geo.cone.use_lds; info[5] = (double)h->ws.geo.glob.use_lds; info[6] = (double)h->ws.geo.small.use_lds; info[7] = (double)h->ws.Rmax;
  return 0;
}

int omc_last_subspace_stats(omc_instance* h, int64_t* out) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  for (int q = 0; q < 8; ++q) out[q] = h->sub_tot[q];
  return 0;
}

int omc_kernel_residency(omc_instance* h, int* out) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (!h->ws.geo.sub_lds) return fail(OMC_ERR_ARGUMENT, "omc_kernel_residency: nothing staged yet (the geometry is planned by omc_relax_stage)");
  HIPCHK(hipSetDevice(h->device));
  omc_query_residency(&h->ws, out);
  return 0;
}

int omc_last_kernel_stats(omc_instance* h, int64_t* launches, double* ms, int64_t* units) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  for (int c = 0; c < OMC_KERNEL_NCLASS; ++c) {
    if (launches) launches[c] = h->launches[c];
    if (ms) ms[c] = h->ms[c];
    if (units) units[c] = h->units[c];
  }
  return 0;
}
