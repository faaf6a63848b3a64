// omc_api.cpp -- host side of libomc_hip.so: the C ABI declared in include/omc.h.
//
// Mirrors the call sites of the reference driver (OMC.jl = /root/reference/src/OptimalMatrixCompletion.jl):
//   omc_relax_*            <- matrix_completion_SDP_relaxation  OMC.jl:1431-1943 (called at 747-754)
//   omc_separation_batch   <- eigs(U U' - Y) at OMC.jl:1274 and 2466-2477
//   omc_evaluate_objective <- evaluate_objective OMC.jl:2330-2359
//   omc_altmin_batch       <- alternating_minimization OMC.jl:1979-2279
// Argument checks reproduce the reference's `error(...)` conditions and return negative codes instead of
// throwing.  No torch types, no host pointer retained after return.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <chrono>
#include <string>
#include <vector>
#include <algorithm>
#include <atomic>
#include <thread>
#include <mutex>

#include "omc.h"
#include "omc_device.h"
#include "omc_altmin.h"
#include "omc_shor.h"
#include "omc_shor_relax.h"
#include "omc_shor_cert.h"
#include <unordered_map>
#include <dlfcn.h>
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#include <rccl/rccl.h>   // types only: the library is loaded with dlopen on first use, so that libomc_hip.so has no hard dependency on it

#include "omc_host.h"
#include "omc_walks.h"

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


extern "C" {

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

static int upload(DevBuf& b, const void* src, size_t bytes, hipStream_t s) {
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
  for (hipStream_t q : {h->stream, h->gs[0], h->gs[1], h->gs[2], h->append_stream, h->fetch_stream}) if (q) (void)hipStreamDestroy(q);
  for (int q = 0; q < 2; ++q) for (hipEvent_t e : h->ev_pool[q]) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->ev_up) if (e) (void)hipEventDestroy(e);
  if (h->ev_gram) (void)hipEventDestroy(h->ev_gram);
  for (int q = 0; q < 5; ++q) for (hipEvent_t e : {h->gev[q], h->gevc[q]}) if (e) (void)hipEventDestroy(e);
  if (h->ev_main) (void)hipEventDestroy(h->ev_main);
  delete h;      // the device buffers free themselves
}

// piece table of the disjunctive cuts (OMC.jl:1580-1678): lo <= v <= hi, g(v) = slope*v + icpt
static int cut_piece(int cut_type, int dir, double vhat, int q1, double* lo, double* hi, double* slope, double* icpt) {
  const double a = fabs(vhat);
  if (cut_type == OMC_CUT_LINEAR) {
    if (dir == OMC_DIR_LEFT) { *lo = -1; *hi = vhat; *slope = vhat - 1; *icpt = vhat; return 0; }      // 1582-1591
    if (dir == OMC_DIR_RIGHT) { *lo = vhat; *hi = 1; *slope = vhat + 1; *icpt = -vhat; return 0; }     // 1592-1601
  } else if (cut_type == OMC_CUT_LINEAR2) {
    if (dir == OMC_DIR_LEFT) { *lo = -1; *hi = -a; *slope = -(1 + a); *icpt = -a; return 0; }          // 1604-1613
    if (dir == OMC_DIR_MIDDLE) { *lo = -a; *hi = a; *slope = 0; *icpt = vhat * vhat; return 0; }       // 1614-1623
    if (dir == OMC_DIR_RIGHT) { *lo = a; *hi = 1; *slope = 1 + a; *icpt = -a; return 0; }              // 1624-1633
  } else if (cut_type == OMC_CUT_LINEAR3) {
    if (dir == OMC_DIR_LEFT) { *lo = -1; *hi = -a; *slope = -(1 + a); *icpt = -a; return 0; }          // 1636-1645
    if (dir == OMC_DIR_INNER_LEFT) { *lo = -a; *hi = 0; *slope = -a; *icpt = 0; return 0; }            // 1646-1655
    if (dir == OMC_DIR_INNER_RIGHT) { *lo = 0; *hi = a; *slope = a; *icpt = 0; return 0; }             // 1656-1665
    if (dir == OMC_DIR_RIGHT) {                                                                        // 1666-1675
      *lo = a; *hi = 1;
      if (q1) { *slope = a; *icpt = 0; } else { *slope = 1 + a; *icpt = -a; }
      return 0;
    }
  }
  return -1;
}


// rows (OMC.jl:1558-1685) and row subspace of a set of nodes, on the host: shared by omc_relax_stage and omc_relax_append
struct NodePack {
  std::vector<std::vector<int>> rk, rc, rbi, rbj;
  std::vector<std::vector<double>> rcoef, rrhs, Qn;
  std::vector<int> rrv;
  int Rmax = 0, rmax = 1, Lmax = 0;
};
static int pack_nodes(omc_instance* h, const omc_relax_params& P, int cut_type, int B, const int* L, const double* cut_x, const double* cut_Uhat,
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
static int put_descriptors(const OmcWS& w, const NodePack& pk, int B, size_t rows, size_t first, const int* L, const double* cut_x, hipStream_t s) {
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

// What the callers of the one staging routine ask of it beyond omc_relax_stage's arguments.  It travels with the call: nothing is left on
// the instance when a stage call returns early.
struct StageMode {
  bool shor = false;            // omc_relax_stage_shor: the base workspace of a Shor-mode batch
  bool warm_filtered = false;   // omc_relax_stage_shor: the warm-start indices have passed its filter
  int colprox_force = 0;        // omc_column_prox_batch: 1 = no block kernel, 2 = the block kernel for every non-empty column
};
static int check_cut_type(int cut_type) {
  if (cut_type != OMC_CUT_LINEAR && cut_type != OMC_CUT_LINEAR2 && cut_type != OMC_CUT_LINEAR3)
    return fail(OMC_ERR_INVALID_ENUM, "Invalid input for disjunctive cuts type: must be linear, linear2 or linear3 (OMC.jl:1456-1462)");
  return 0;
}

static int stage_base(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L, const double* cut_x, const double* cut_Uhat,
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
    r0 = h->brho.ensure(sizeof(double) * (size_t)S); if (r0) return r0;
    w.rho_b = h->brho.as<double>();
  }
  w.relax = P.relax; w.eps_gap = P.eps_gap; w.eps_feas = P.eps_feas;
  w.check_every = std::max(1, P.check_every); w.early_stop_after = P.early_stop_after; w.early_stop_factor = (P.first_wins ? 0.0 : P.early_stop_factor);
  // what the packed buffers below are carved by (omc_walks.h): state arrays one per slot, descriptor and output arrays one per node (plus
  // the room reserved for appended nodes)
  const StageDims sd = {(size_t)S, (size_t)B + (size_t)extra_nodes, (size_t)n, (size_t)m, (size_t)k, (size_t)h->nnz, (size_t)rmax, (size_t)Rmax};
  {
    ENS_CARVE(h->bgap, [&](Carve& c) { walk_gap(c, sd, w); });
    int r0 = h->bvotes.ensure(sizeof(int) * (size_t)S); if (r0) return r0;
    r0 = h->bslotlist.ensure(sizeof(int) * (size_t)S); if (r0) return r0;
    w.slow_votes = h->bvotes.as<int>();
    w.slot_list = nullptr;      // set on the per-iteration copies only (omc_relax_solve)
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
  w.cp_nsolo = h->nsolo; w.cp_solo = h->nsolo ? h->dsolo.as<int>() : nullptr;
  w.cp_nwide = h->nwide; w.cp_wide = h->nwide ? h->dwide.as<int>() : nullptr;
  w.Ncnt = h->dNcnt.as<double>(); w.wY1 = h->dwY.as<double>();
  w.row_ptr = h->drow_ptr.as<int>(); w.row_idx = h->drow_idx.as<int>();
  const size_t sB = (size_t)S;      // state arrays: one per slot
  const size_t sN = (size_t)B + (size_t)extra_nodes;      // descriptor and output arrays: one per node (plus the room reserved for appended nodes)
  ENS(h->bY, sB * n * n * 8); ENS(h->bYp, sB * n * n * 8); ENS(h->bU, sB * n * k * 8);
  ENS(h->bD1, sB * n * n * 8); ENS(h->bD3, sB * n * n * 8); ENS(h->bW1, sB * n * n * 8); ENS(h->bE3, sB * n * n * 8);
  ENS(h->bdS, sB * rmax * rmax * 8);
  ENS_CARVE(h->bsm, [&](Carve& c) { walk_small_cone(c, sd, w); });
  ENS(h->balpha, sB * h->nnz * 8); ENS(h->balphaX, sB * h->nnz * 8); ENS(h->bsval, sB * m * 8);
  ENS(h->bMchk, sB * n * n * 8);
  size_t chk_bytes = 0;
  ENS_CARVE(h->bchk, [&](Carve& c) { walk_check(c, sd, w); }, &chk_bytes);
  ENS(h->bG, sB * Rmax * Rmax * 8); ENS(h->blam, sB * Rmax * 8);
  ENS_CARVE(h->bscal, [&](Carve& c) { walk_scalars(c, sd, w); });
  ENS(h->bbx, sB * n * 8);
  ENS_CARVE(h->bint, [&](Carve& c) { walk_slot_ints(c, sd, w); });
  w.np16 = (n + 15) & ~15;
  ENS(h->bMbuf, sB * w.np16 * w.np16 * 8); ENS(h->bVrow, sB * w.np16 * w.np16 * 8);
  ENS(h->blamD, sB * m * n * 8);
  HIPCHK(hipMemsetAsync(h->blamD.p, 0, sB * m * n * 8, h->stream));
  w.lamD = h->blamD.as<double>();
  w.lamDX = nullptr;
  if (n > 144 || shor) {      // large orders: the certificate matrix takes Lambda Lambda' from one MFMA product
    ENS(h->blamDX, sB * m * n * 8);
    HIPCHK(hipMemsetAsync(h->blamDX.p, 0, sB * m * n * 8, h->stream));
    w.lamDX = h->blamDX.as<double>();
  }
  w.Mbuf = h->bMbuf.as<double>(); w.Vrow = h->bVrow.as<double>();
  {   // tracked subspace of the cone block (k_cone_sub)
    size_t subS_bytes = 0, subI_bytes = 0;
    ENS(h->bXs, sB * w.np16 * 16 * 8);
    ENS_CARVE(h->bsubS, [&](Carve& c) { walk_sub_doubles(c, sd, w); }, &subS_bytes);
    ENS_CARVE(h->bsubI, [&](Carve& c) { walk_sub_ints(c, sd, w); }, &subI_bytes);      // w1_fac (factored W1): kept or dropped below, once k_global's variant is known
    HIPCHK(hipMemsetAsync(h->bXs.p, 0, sB * w.np16 * 16 * 8, h->stream));
    HIPCHK(hipMemsetAsync(h->bsubS.p, 0, subS_bytes, h->stream));
    HIPCHK(hipMemsetAsync(h->bsubI.p, 0, subI_bytes, h->stream));
    w.Xs = h->bXs.as<double>(); w.ws_phase = 0;
    w.sub_guard = SUB_GUARD; w.sub_qmax = h->tun.sub_qmax; w.sub_chunk = SUB_CHUNK;
    w.sub_tol = SUB_TOL; w.sub_adapt = SUB_ADAPT; w.sub_debug = h->tun.sub_debug;
    w.sub_enable = 0;     // decided below, once the cone kernel variant is known
    size_t subSC_bytes = 0, subIC_bytes = 0;
    ENS(h->bXsC, sB * w.np16 * 16 * 8);
    ENS_CARVE(h->bsubSC, [&](Carve& c) { walk_subC_doubles(c, sd, w); }, &subSC_bytes);
    ENS_CARVE(h->bsubIC, [&](Carve& c) { walk_subC_ints(c, sd, w); }, &subIC_bytes);      // sep_done: kept or dropped below with sub_enable
    HIPCHK(hipMemsetAsync(h->bXsC.p, 0, sB * w.np16 * 16 * 8, h->stream));
    HIPCHK(hipMemsetAsync(h->bsubSC.p, 0, subSC_bytes, h->stream));
    HIPCHK(hipMemsetAsync(h->bsubIC.p, 0, subIC_bytes, h->stream));
    w.XsC = h->bXsC.as<double>();
    w.cert_enable = 0;
  }
  {   // warm-started eigenvalues for the certificate matrix
    ENS(h->bMbufC, sB * w.np16 * w.np16 * 8); ENS(h->bVrowC, sB * w.np16 * w.np16 * 8); ENS(h->bchkS, sB * 8); ENS(h->bchkI, sB * sizeof(int));
    HIPCHK(hipMemsetAsync(h->bMbufC.p, 0, sB * w.np16 * w.np16 * 8, h->stream));
    HIPCHK(hipMemsetAsync(h->bVrowC.p, 0, sB * w.np16 * w.np16 * 8, h->stream));   // its zero padding feeds the branch-free K loop of the MFMA GEMM: 0 x garbage could be NaN
    HIPCHK(hipMemsetAsync(h->bchkI.p, 0, sB * sizeof(int), h->stream));
    w.MbufC = h->bMbufC.as<double>(); w.VrowC = h->bVrowC.as<double>(); w.fro2c = h->bchkS.as<double>(); w.vvalidC = h->bchkI.as<int>();
  }
  w.Y = h->bY.as<double>(); w.Yp = h->bYp.as<double>(); w.U = h->bU.as<double>();
  w.Yx = nullptr;
  if (!shor && !P.accel) { ENS(h->bYx, sB * n * n * 8); w.Yx = h->bYx.as<double>(); }      // 2 Y - Yp for the column gathers (k_aa rewrites Y and Yp behind k_global's back)
  // with Yx the column kernels never read Yp (k_aa and the Shor kernels, its only other readers, run without Yx; k_setup rewrites it at
  // every start; the state pool does not keep it): k_global stops storing it
  w.skip_yp = (w.Yx && !h->tun.dense_proj) ? 1 : 0;
  w.D1 = h->bD1.as<double>(); w.D3 = h->bD3.as<double>(); w.W1 = h->bW1.as<double>(); w.E3 = h->bE3.as<double>();
  w.dS = h->bdS.as<double>();
  w.alpha = h->balpha.as<double>(); w.alphaX = h->balphaX.as<double>(); w.sval = h->bsval.as<double>();
  ENS_CARVE(h->bobjcol, [&](Carve& c) { walk_objcol(c, sd, w); });
  w.Mchk = h->bMchk.as<double>(); w.G = h->bG.as<double>(); w.lam = h->blam.as<double>();
  w.bx = h->bbx.as<double>();
  if (w.accel) {
    w.aa_dim = 4 * n * n + 2 * rmax * k + k * k + h->nnz;
    const size_t ring = sB * (size_t)(w.aa_mem + 1) * w.aa_dim * 8;
    size_t aaI_bytes = 0;
    ENS(h->baaF, ring); ENS(h->baaG, ring); ENS(h->baaZ, sB * (size_t)w.aa_dim * 8); ENS(h->baaS, sB * 8);
    ENS_CARVE(h->baaI, [&](Carve& c) { walk_aa_ints(c, sd, w); }, &aaI_bytes);
    w.aa_F = h->baaF.as<double>(); w.aa_G = h->baaG.as<double>(); w.aa_zin = h->baaZ.as<double>(); w.aa_fn = h->baaS.as<double>();
    HIPCHK(hipMemsetAsync(h->baaI.p, 0, aaI_bytes, h->stream));
  }
  HIPCHK(hipMemsetAsync(w.ws_need, 0, sizeof(int), h->stream));
  {
    size_t map_bytes = 0;
    ENS_CARVE(h->bslotint, [&](Carve& c) { walk_slot_map(c, sd, w.node_of, w.init, w.fin); }, &map_bytes);
    std::vector<int> hs(map_bytes / sizeof(int));      // the host image of the three arrays, laid out by the same walk
    int *h_node = nullptr, *h_init = nullptr, *h_fin = nullptr;
    { Carve hc(hs.data()); walk_slot_map(hc, sd, h_node, h_init, h_fin); }
    for (size_t b = 0; b < sB; ++b) { h_node[b] = (int)b; h_init[b] = 1; h_fin[b] = 1; }   // identity map, every slot initialises
    HIPCHK(hipMemcpyAsync(h->bslotint.p, hs.data(), map_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));          // hs dies with this block
    ENS(h->boY, sN * n * n * 8); ENS(h->boU, sN * n * k * 8); ENS(h->boal, sN * h->nnz * 8); ENS(h->bobx, sN * n * 8);
    ENS_CARVE(h->boscal, [&](Carve& c) { walk_out_scalars(c, sd, w); });
    ENS_CARVE(h->boint, [&](Carve& c) { walk_out_ints(c, sd, w); });
    w.oY = h->boY.as<double>(); w.oU = h->boU.as<double>(); w.oalphaX = h->boal.as<double>(); w.obx = h->bobx.as<double>();
  }
  if ((h->keep_cert && !shor) || (h->keep_shor_cert && shor)) {      // best certificate per node: slot buffers and the arena of the nodes, zeroed (no slot and no node holds one)
    const size_t cnnz = shor ? 0 : (size_t)h->nnz;      // Shor mode has no alphaX: its own multipliers are kept by omc_relax_stage_shor (ShWS::cbGam ...)
    size_t cbD_bytes = 0, cbI_bytes = 0, ocD_bytes = 0;
    ENS_CARVE(h->bcbD, [&](Carve& c) { walk_cert_slot(c, sd, cnnz, w); }, &cbD_bytes);
    ENS_CARVE(h->bcbI, [&](Carve& c) { walk_cert_flags(c, sd, w); }, &cbI_bytes);
    ENS_CARVE(h->bocD, [&](Carve& c) { walk_cert_node(c, sd, cnnz, w); }, &ocD_bytes);
    ENS(h->bocI, sN * sizeof(int));
    HIPCHK(hipMemsetAsync(h->bcbD.p, 0, cbD_bytes, h->stream)); HIPCHK(hipMemsetAsync(h->bcbI.p, 0, cbI_bytes, h->stream));
    HIPCHK(hipMemsetAsync(h->bocD.p, 0, ocD_bytes, h->stream)); HIPCHK(hipMemsetAsync(h->bocI.p, 0, sN * sizeof(int), h->stream));
    if (shor) { w.cbLam = nullptr; w.ocLam = nullptr; }
    w.ocHave = h->bocI.as<int>();
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
  ENS(h->bQb, sN * n * rmax * 8); ENS(h->brr, sN * sizeof(int)); ENS(h->bR, sN * sizeof(int));
  ENS(h->brkind, sN * Rmax * sizeof(int)); ENS(h->brcut, sN * Rmax * sizeof(int)); ENS(h->brbi, sN * Rmax * sizeof(int)); ENS(h->brbj, sN * Rmax * sizeof(int));
  ENS(h->brcoef, sN * Rmax * k * 8); ENS(h->brrhs, sN * Rmax * 8); ENS(h->bcutx, sN * w.Lmax * n * 8);
  w.Qb = h->bQb.as<double>(); w.rr = h->brr.as<int>(); w.R = h->bR.as<int>(); w.rkind = h->brkind.as<int>(); w.rcut = h->brcut.as<int>();
  w.rbi = h->brbi.as<int>(); w.rbj = h->brbj.as<int>(); w.rcoef = h->brcoef.as<double>(); w.rrhs = h->brrhs.as<double>(); w.cutx = h->bcutx.as<double>();
  if ((rc_ = put_descriptors(w, pk, B, sN, 0, L, cut_x, h->stream))) return rc_;
  // LDS / scratch decisions: one planner (omc_layout.h), the slabs allocated from the strides it reports
  w.geo = omc_plan_geometry(n, w.np16, k, rmax, Rmax, h->cmax, h->tun.global_nolds, h->tun.cone_multi_min, h->tun.plain_multi_min);
  ENS(h->bmwstat, sB * 4 * sizeof(int)); HIPCHK(hipMemsetAsync(h->bmwstat.p, 0, sB * 4 * sizeof(int), h->stream));
  w.mw_stat = h->bmwstat.as<int>(); w.mw_budget = MAX_SWEEPS; w.ev_out = nullptr;
  w.pmw_stat = nullptr;
  if (w.geo.plain_mw) { ENS(h->bpmwstat, sB * 4 * sizeof(int)); HIPCHK(hipMemsetAsync(h->bpmwstat.p, 0, sB * 4 * sizeof(int), h->stream)); w.pmw_stat = h->bpmwstat.as<int>(); }
  // k_colprox_block: the dynamic LDS of its launches and the slab of the columns beyond the LDS, for those columns only.  The slab of
  // colprox_body (one block per slot and column) is sized by the longest column that still runs it
  geom_set_cpblock(w.geo, h->cpb_cl, h->cpb_cs);
  w.geo.cp_scratch_stride = h->crest_max > w.geo.cp_lds_c ? cp_body_layout(h->crest_max).doubles : 0;
  if (w.geo.cpb_slab_stride && !shor) { ENS(h->bcpb, sB * h->nslab * w.geo.cpb_slab_stride * 8); w.cp_bslab = h->bcpb.as<double>(); }
  if (w.geo.cp_scratch_stride) { ENS(h->bcp, sB * m * w.geo.cp_scratch_stride * 8); w.cp_scratch = h->bcp.as<double>(); }
  if (w.geo.ws.slab_stride) { ENS(h->bcone, sB * w.geo.ws.slab_stride * 8); w.cone_scratch = h->bcone.as<double>(); }
  if (w.geo.glob.slab_stride) { ENS(h->bglob, sB * w.geo.glob.slab_stride * 8); w.glob_scratch = h->bglob.as<double>(); }
  if (w.geo.small.slab_stride) { ENS(h->bsmall, sB * w.geo.small.slab_stride * 8); w.small_scratch = h->bsmall.as<double>(); }
  // subspace tracking needs the warm-started kernel as its seed / fall-back and at least 3 x 16 rows
  w.sub_enable = (w.geo.ws_lpp && n >= 48 && w.geo.sub_lds <= OMC_MAX_DYN_LDS && !h->tun.no_subspace) ? 1 : 0;
  w.sub_zscratch = nullptr;
  if (w.sub_enable && w.np16 > 512) { ENS(h->bsubz, sB * 16 * (size_t)(w.np16 + 2) * 8); w.sub_zscratch = h->bsubz.as<double>(); }
  w.cert_enable = (w.sub_enable && w.np16 > 512) ? 1 : 0;      // large orders: the certificate eigenvalues by the tracked block too (rigorous confirmation before anything is reported)
  if (!w.sub_enable) w.sep_done = nullptr;
  // factored W1 (OmcWS::w1_fac): k_global stages the accepted Ritz vectors of a slot in its NNQP scratch (LDS variant only; glob_w1_fits).
  // Off in Shor mode (its W1 views are other arrays) and with OMC_DENSE_PROJ=1.
  if (!(!shor && w.sub_enable && w.geo.glob.use_lds && glob_w1_fits(n) && !h->tun.dense_proj)) w.w1_fac = nullptr;
  HIPCHK(hipMemsetAsync(w.sweeps, 0, sizeof(int) * S, h->stream));
  HIPCHK(hipMemsetAsync(w.stamps, 0, (size_t)((char*)h->bchk.p + chk_bytes - (char*)w.stamps), h->stream));      // from stamps to the end of the walk
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

static uint64_t fnv1a(const void* p, size_t bytes, uint64_t hsh) {
  const uint8_t* c = (const uint8_t*)p;
  for (size_t e = 0; e < bytes; ++e) { hsh ^= c[e]; hsh *= 1099511628211ull; }
  return hsh;
}
static constexpr uint64_t FNV_SEED = 1469598103934665603ull;

// The one rule for starting a Shor node from a saved Shor state: 1 = identical (minor list, SOC list) pairs, 2 = the parent's minor list is a
// strict prefix of the child's and both SOC lists are the complement shorthand, 0 = no transfer.  same_head: the child's first n_parent tuples
// are the parent's list; same_soc: the SOC lists are equal (only asked when the lengths agree).
static int shor_warm_rule(int64_t n_parent, int64_t n_soc_parent, int64_t n_child, int64_t n_soc_child, bool same_head, bool same_soc) {
  if (n_parent < 0 || n_child < 0 || n_parent > n_child || !same_head) return 0;
  if (n_parent == n_child) return (n_soc_parent == n_soc_child && same_soc) ? 1 : 0;
  return (n_soc_parent == -1 && n_soc_child == -1) ? 2 : 0;
}

int omc_shor_warm_compat(int64_t n_parent, const int64_t* parent_idx, int64_t n_soc_parent, const int64_t* parent_soc, int64_t n_child,
                         const int64_t* child_idx, int64_t n_soc_child, const int64_t* child_soc) {
  if (n_parent < 0 || n_child < 0 || n_parent > n_child) return 0;
  if ((n_parent > 0 && !parent_idx) || (n_child > 0 && !child_idx)) return 0;
  if ((n_soc_parent > 0 && !parent_soc) || (n_soc_child > 0 && !child_soc)) return 0;
  const bool same_head = n_parent == 0 || memcmp(parent_idx, child_idx, 32 * (size_t)n_parent) == 0;
  const bool same_soc = n_soc_parent == n_soc_child && (n_soc_parent <= 0 || memcmp(parent_soc, child_soc, 16 * (size_t)n_soc_parent) == 0);
  return shor_warm_rule(n_parent, n_soc_parent, n_child, n_soc_child, same_head, same_soc);
}

int omc_state_pool_reserve_shor(omc_instance* h, int64_t nq_max) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (h->pool_cap <= 0) return fail(OMC_ERR_ARGUMENT, "omc_state_pool_reserve_shor: no state pool (omc_state_pool_create)");
  if (nq_max < 0 || nq_max >= (1ll << 28)) return fail(OMC_ERR_ARGUMENT, "omc_state_pool_reserve_shor: nq_max out of range");
  if (h->worker_running.load()) return fail(OMC_ERR_ARGUMENT, "omc_state_pool_reserve_shor: a solve is running");
  HIPCHK(hipSetDevice(h->device));
  const ShorPoolLayout L = shor_pool_layout(h->n, h->m, (int)nq_max);
  DevBuf nb, nh;      // allocated beside the old buffers: a failure leaves the pool as it was
  { int r_ = nb.ensure((size_t)h->pool_cap * L.stride * 8); if (r_) return r_; }
  { int r_ = nh.ensure((size_t)h->pool_cap * 4 * sizeof(long long)); if (r_) return r_; }
  HIPCHK(hipMemsetAsync(nh.p, 0, (size_t)h->pool_cap * 4 * sizeof(long long), h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::swap(h->pShor.p, nb.p); std::swap(h->pShor.cap, nb.cap);
  std::swap(h->pShorHdr.p, nh.p); std::swap(h->pShorHdr.cap, nh.cap);
  { std::lock_guard<std::mutex> lk(h->sig_mu); h->pool_sig.assign((size_t)h->pool_cap, omc_instance::PoolSig{}); }      // every entry is invalid now
  h->pool_shor = true; h->pool_nqmax = nq_max;
  return 0;
}

int omc_last_shor_warm_stats(omc_instance* h, int64_t out[4]) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  for (int q = 0; q < 4; ++q) out[q] = h->shor_warm_stats[q];
  return 0;
}

// scale of the Shor splitting: the program is homogeneous of degree 2 in A (oracle: shor_scale)
static double shor_scale(const omc_instance* h) {
  return sqrt(((double)h->nnz / ((double)h->n * h->m)) * (double)std::min(h->n, h->m) / std::max(h->sumA2, 1e-300));
}

int omc_state_pool_fetch_shor(omc_instance* h, int entry, int64_t* nq, double* X, double* Theta, double* V) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (!h->pool_shor || entry < 0 || entry >= h->pool_cap) return fail(OMC_ERR_ARGUMENT, "omc_state_pool_fetch_shor: no such entry (omc_state_pool_reserve_shor)");
  if (h->worker_running.load()) return fail(OMC_ERR_ARGUMENT, "omc_state_pool_fetch_shor: a solve is running");
  { std::lock_guard<std::mutex> lk(h->sig_mu);
    if (h->pool_sig[entry].kind != 2) return fail(OMC_ERR_ARGUMENT, "omc_state_pool_fetch_shor: the entry is empty or was saved by a base-mode solve"); }
  HIPCHK(hipSetDevice(h->device));
  const size_t n = h->n, m = h->m, pnq = (size_t)h->pool_nqmax;
  const ShorPoolLayout L = shor_pool_layout(h->n, h->m, (int)pnq);
  const double* E = h->pShor.as<double>() + (size_t)entry * L.stride;
  long long hd[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(hd, h->pShorHdr.as<long long>() + (size_t)entry * 4, sizeof(hd), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t q = (size_t)std::max<long long>(0, std::min<long long>(hd[0], (long long)pnq));
  if (nq) *nq = (int64_t)q;
  const double isc = 1.0 / shor_scale(h), is2 = isc * isc;
  if (X) { HIPCHK(hipMemcpyAsync(X, E + L.X, 8 * n * m, hipMemcpyDeviceToHost, h->stream)); }
  if (Theta) { HIPCHK(hipMemcpyAsync(Theta, E + L.Th, 8 * m * m, hipMemcpyDeviceToHost, h->stream)); }
  std::vector<double> Vs;
  if (V && q) { Vs.resize(5 * q); for (int c = 0; c < 5; ++c) HIPCHK(hipMemcpyAsync(Vs.data() + c * q, E + L.V + c * pnq, 8 * q, hipMemcpyDeviceToHost, h->stream)); }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (X) for (size_t e = 0; e < n * m; ++e) X[e] *= isc;
  if (Theta) for (size_t e = 0; e < m * m; ++e) Theta[e] *= is2;
  if (V) for (size_t t = 0; t < q; ++t) for (int c = 0; c < 5; ++c) V[t * 5 + c] = Vs[c * q + t] * is2;
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

// The one append path, defined below behind the Shor list helpers it uses.  `lists`: the lists of the nodes of an omc_relax_append_shor call, NULL in base mode
struct ShorAppendLists { const int64_t *n_shor, *shor_idx, *n_soc, *soc_idx; };
static int append_nodes(omc_instance* h, const char* who, int B2, const int* L, const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir,
                        const int* load_from, const int* save_to, const ShorAppendLists* lists);
int omc_relax_append(omc_instance* h, int B2, const int* L, const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir,
                     const int* load_from, const int* save_to) {
  if (!h || !h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_append: nothing staged");
  if (B2 <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  if (h->shor_on) return fail(OMC_ERR_UNSUPPORTED, "omc_relax_append: the staged batch is in Shor mode (omc_relax_append_shor)");
  return append_nodes(h, "omc_relax_append", B2, L, cut_x, cut_Uhat, cut_dir, load_from, save_to, nullptr);
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
static int require_finished_ids(omc_instance* h, int n_ids, const int* ids, bool upto_read_only, const char* who) {
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

static int require_certificates(const OmcWS& w, int n_ids, const int* ids, hipStream_t fs, const char* who) {
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
    int r_ = h->bXout.ensure(8 * B * n * m); if (r_) return r_;
    omc_launch_make_X(&w, h->bXout.as<double>(), s);
    if (X) HIPCHK(hipMemcpyAsync(X, h->bXout.p, 8 * B * n * m, hipMemcpyDeviceToHost, s));
    if (Theta) {
      r_ = h->bThout.ensure(8 * B * m * m); if (r_) return r_;
      omc_launch_make_Theta(&w, h->bXout.as<double>(), h->bThout.as<double>(), s);
      HIPCHK(hipMemcpyAsync(Theta, h->bThout.p, 8 * B * m * m, hipMemcpyDeviceToHost, s));
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


// ---- Shor mode (rank 1): matrix_completion_SDP_relaxation with add_Shor_valid_inequalities = true ---------------------------------------
// OMC.jl:1503-1525, 1755-1779, 1838-1846; node.Shor_info lists OMC.jl:37-40.  Formulation: oracle/omc_oracle_shor.py, DESIGN.md 3.7.
int omc_set_shor_penalties(omc_instance* h, double rho, double r4, double r5) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (!(rho > 0.0) || !(r4 >= 0.0) || !(r5 > 0.0)) return fail(OMC_ERR_ARGUMENT, "rho and r5 must be positive, r4 non-negative (0 = automatic)");
  h->shor_rho = rho; h->shor_r4 = r4; h->shor_r5 = r5;
  return 0;
}

namespace {
struct ShorGroupHost {
  int nq = 0, nv1 = 0, nv2 = 0;
  uint64_t hash = 0; double r4 = 0.0;      // FNV-1a of the list's tuples ; penalty of its order-5 blocks relative to rho
  std::vector<int> mi, kid, cptr, cent, v1ptr, v1ent, v2ptr, v2ent, slackrow;
  std::vector<uint8_t> eclass, ctype;
  size_t off_int = 0, off_byte = 0;       // offsets into the concatenated device buffers
  // built on the device (omc_shor_index.hip): the arrays wait in the staging room at st_int / st_byte, each at its capacity; the vectors stay
  // empty (ctype is copied back where a caller reads it on the host).  The packed lengths follow from the counts.
  bool dev = false; size_t st_int = 0, st_byte = 0, nm = 0, m = 0;
  size_t ints() const {
    if (dev) return (size_t)16 * nq + nm + m + 3 + (size_t)nv1 + (size_t)nv2;
    return mi.size() + kid.size() + cptr.size() + cent.size() + v1ptr.size() + v1ent.size() + v2ptr.size() + v2ent.size() + slackrow.size();
  }
  size_t bytes() const { return ((dev ? nm + m : eclass.size() + ctype.size()) + 15) & ~(size_t)15; }
};
// keys sorted, ids assigned in sorted order (as numpy.unique does in the oracle); members in increasing (minor, position) order
static void build_keys(const std::vector<uint64_t>& keyA, const std::vector<uint64_t>& keyB, int nq, int& nkeys, int* kidA, int* kidB,
                       std::vector<int>& ptr, std::vector<int>& ent) {
  std::vector<std::pair<uint64_t, int>> all((size_t)2 * nq);
  for (int q = 0; q < nq; ++q) { all[(size_t)2 * q] = {keyA[q], 2 * q}; all[(size_t)2 * q + 1] = {keyB[q], 2 * q + 1}; }
  std::sort(all.begin(), all.end());
  ptr.clear(); ent.resize((size_t)2 * nq);
  nkeys = 0;
  for (size_t e = 0; e < all.size(); ++e) {
    if (e == 0 || all[e].first != all[e - 1].first) { ptr.push_back((int)e); ++nkeys; }
    ent[e] = all[e].second;
    const int q = all[e].second >> 1;
    if (all[e].second & 1) kidB[q] = nkeys - 1; else kidA[q] = nkeys - 1;
  }
  ptr.push_back((int)all.size());
}

// wire format of a batch of Shor lists: lengths checked, offsets of every node's tuples / pairs in the concatenated arrays
static int shor_list_offsets(int B, const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx,
                             std::vector<size_t>& so, std::vector<size_t>& co) {
  so.assign(B + 1, 0); co.assign(B + 1, 0);
  for (int b = 0; b < B; ++b) {
    if (n_shor[b] < 0 || n_soc[b] < -1) return fail(OMC_ERR_ARGUMENT, "negative list length");
    if (n_shor[b] >= (1ll << 28)) return fail(OMC_ERR_UNSUPPORTED, "Shor mode: more than 2^28 minors in one node");
    so[b + 1] = so[b] + (size_t)n_shor[b]; co[b + 1] = co[b] + (size_t)(n_soc[b] > 0 ? n_soc[b] : 0);
  }
  if (so[B] > 0 && !shor_idx) return fail(OMC_ERR_ARGUMENT, "shor_idx is NULL but n_shor > 0");
  if (co[B] > 0 && !soc_idx) return fail(OMC_ERR_ARGUMENT, "soc_idx is NULL but n_soc > 0");
  return 0;
}

// identity of a (minor list, SOC list) pair among the lists a batch knows: hash of both lists, then the lists themselves
using ShorListKey = omc_instance::ShorListKey;
static uint64_t shor_pair_hash(int64_t nq, const int64_t* idx, int64_t nsoc, const int64_t* soc) {
  uint64_t hv = FNV_SEED;
  hv = fnv1a(&nq, 8, hv); hv = fnv1a(&nsoc, 8, hv);
  hv = fnv1a(idx, 32 * (size_t)nq, hv);
  if (nsoc > 0) hv = fnv1a(soc, 16 * (size_t)nsoc, hv);
  return hv;
}
static int find_shor_list(const std::unordered_map<uint64_t, std::vector<int>>& byhash, const std::vector<ShorListKey>& lists, uint64_t hv,
                          int64_t nq, const int64_t* idx, int64_t nsoc, const int64_t* soc) {
  auto it = byhash.find(hv);
  if (it == byhash.end()) return -1;
  for (int g : it->second) {
    const ShorListKey& K = lists[g];
    if (K.nq == nq && K.nsoc == nsoc && (nq == 0 || memcmp(K.idx.data(), idx, 32 * (size_t)nq) == 0) &&
        (nsoc <= 0 || memcmp(K.soc.data(), soc, 16 * (size_t)nsoc) == 0)) return g;
  }
  return -1;
}
static void add_shor_list(std::unordered_map<uint64_t, std::vector<int>>& byhash, std::vector<ShorListKey>& lists, uint64_t hv,
                          int64_t nq, const int64_t* idx, int64_t nsoc, const int64_t* soc) {
  ShorListKey K;
  K.nq = nq; K.nsoc = nsoc; K.hlist = fnv1a(idx, 32 * (size_t)nq, FNV_SEED);
  if (nq > 0) K.idx.assign(idx, idx + 4 * (size_t)nq);
  if (nsoc > 0) K.soc.assign(soc, soc + 2 * (size_t)nsoc);
  byhash[hv].push_back((int)lists.size());
  lists.push_back(std::move(K));
}

// the weight of the order-5 blocks on an entry of X / W is r4 x (blocks that hold it): r4 follows the mean multiplicity 4 nq / (n m)
// (measured: 20 at 12 x 14 with 152 minors, 5 at 100 x 100 with 38 813, 1.2 at 200 x 200 with 632 732 certify fastest)
static double shor_auto_r4(const omc_instance* h, int nq) {
  return (h->shor_r4 > 0.0) ? h->shor_r4 : std::min(40.0, std::max(0.25, 75.0 * (double)h->n * (double)h->m / (4.0 * (double)std::max(nq, 1))));
}
static const char* const SHOR_MSG_RANGE = "Shor minors must satisfy 1 <= i1 < i2 <= n, 1 <= j1 < j2 <= m (OMC.jl:2556-2603)";
static const char* const SHOR_MSG_DUP = "duplicate Shor minor in a node's list";
static const char* const SHOR_MSG_SOC = "SOC coordinate out of range";

// One (minor list, SOC list) pair -> the index structure its nodes share (validation, keys, coordinate CSR, entry classes, column types, slack
// rows, block penalty, list hash).  The one builder: every caller comes through group_shor_lists.
static int build_shor_group(const omc_instance* h, int64_t nq64, const int64_t* idx, int64_t nsoc, const int64_t* soc, ShorGroupHost& G) {
  const int n = h->n, m = h->m;
  const int nq = (int)nq64;
  G.nq = nq;
  G.hash = fnv1a(idx, 32 * (size_t)nq, FNV_SEED);
  G.mi.resize((size_t)4 * nq); G.kid.resize((size_t)4 * nq);
  std::vector<uint64_t> enc(nq), k1a(nq), k1b(nq), k2a(nq), k2b(nq);
  std::vector<int> cnt((size_t)n * m + 1, 0);
  for (int q = 0; q < nq; ++q) {
    const int64_t* t = idx + 4 * (size_t)q;
    const int64_t i1 = t[0] - 1, i2 = t[1] - 1, j1 = t[2] - 1, j2 = t[3] - 1;
    if (!(0 <= i1 && i1 < i2 && i2 < n && 0 <= j1 && j1 < j2 && j2 < m))
      return fail(OMC_ERR_ARGUMENT, SHOR_MSG_RANGE);
    G.mi[q] = (int)i1; G.mi[(size_t)nq + q] = (int)i2; G.mi[(size_t)2 * nq + q] = (int)j1; G.mi[(size_t)3 * nq + q] = (int)j2;
    enc[q] = (((uint64_t)i1 * n + (uint64_t)i2) * m + (uint64_t)j1) * m + (uint64_t)j2;
    k1a[q] = ((uint64_t)i1 * m + j1) * m + j2; k1b[q] = ((uint64_t)i2 * m + j1) * m + j2;      // V1[i,(j1,j2)]
    k2a[q] = ((uint64_t)i1 * n + i2) * m + j1; k2b[q] = ((uint64_t)i1 * n + i2) * m + j2;      // V2[(i1,i2),j]
    ++cnt[(size_t)j1 * n + i1]; ++cnt[(size_t)j2 * n + i1]; ++cnt[(size_t)j1 * n + i2]; ++cnt[(size_t)j2 * n + i2];
  }
  { std::vector<uint64_t> se = enc; std::sort(se.begin(), se.end()); if (std::adjacent_find(se.begin(), se.end()) != se.end()) return fail(OMC_ERR_ARGUMENT, SHOR_MSG_DUP); }
  build_keys(k1a, k1b, nq, G.nv1, G.kid.data(), G.kid.data() + nq, G.v1ptr, G.v1ent);
  build_keys(k2a, k2b, nq, G.nv2, G.kid.data() + (size_t)2 * nq, G.kid.data() + (size_t)3 * nq, G.v2ptr, G.v2ent);
  // coordinate CSR: members in increasing (minor, position) order
  G.cptr.assign((size_t)n * m + 1, 0);
  for (size_t e = 0; e < (size_t)n * m; ++e) G.cptr[e + 1] = G.cptr[e] + cnt[e];
  G.cent.resize((size_t)4 * nq);
  { std::vector<int> fill(G.cptr.begin(), G.cptr.end() - 1);
    for (int q = 0; q < nq; ++q) {
      const int i1 = G.mi[q], i2 = G.mi[(size_t)nq + q], j1 = G.mi[(size_t)2 * nq + q], j2 = G.mi[(size_t)3 * nq + q];
      const size_t ce[4] = {(size_t)j1 * n + i1, (size_t)j2 * n + i1, (size_t)j1 * n + i2, (size_t)j2 * n + i2};
      for (int p = 0; p < 4; ++p) G.cent[fill[ce[p]]++] = 4 * q + p;
    } }
  // entry classes, column types, slack rows
  G.eclass.assign((size_t)n * m, 0);
  if (nsoc < 0) { for (size_t e = 0; e < (size_t)n * m; ++e) G.eclass[e] = 1; }
  else for (int64_t c = 0; c < nsoc; ++c) {
    const int64_t i = soc[2 * c] - 1, j = soc[2 * c + 1] - 1;
    if (!(0 <= i && i < n && 0 <= j && j < m)) return fail(OMC_ERR_ARGUMENT, SHOR_MSG_SOC);
    G.eclass[(size_t)j * n + i] = 1;
  }
  for (size_t e = 0; e < (size_t)n * m; ++e) if (cnt[e] > 0) G.eclass[e] = 2;      // W >= X^2 is implied by the order-5 block there
  G.ctype.assign(m, 2); G.slackrow.assign(m, -1);
  for (int j = 0; j < m; ++j) {
    int first_nonC = -1, first_unobs = -1;
    for (int i = 0; i < n; ++i) {
      if (G.eclass[(size_t)j * n + i] == 2) continue;
      if (first_nonC < 0) first_nonC = i;
      if (first_unobs < 0 && !h->mask[(size_t)j * n + i]) first_unobs = i;
    }
    if (first_unobs >= 0) { G.ctype[j] = 0; G.slackrow[j] = first_unobs; }
    else if (first_nonC >= 0) { G.ctype[j] = 1; G.slackrow[j] = first_nonC; }
  }
  if (h->k > 1) {
    // Reference quirk Q5 (oracle/omc_oracle_shor.py header): in the rank k > 1 form (OMC.jl:1526-1551, 1780-1827) the slack that H
    // cancels in W = sum Wt + 2 sum H makes every per-layer order-5 block satisfiable, so the minors do not constrain (X, W); what remains of them
    // is W >= X^2 on their coordinates (implied by the order-(k+1) block).  The program solved is therefore the one without order-5 blocks and
    // with those coordinates on the SOC list; the lifted variables Xt, Wt, H, V of the result are an explicit extension (host side: api.py).
    for (size_t e = 0; e < (size_t)n * m; ++e) if (G.eclass[e] == 2) G.eclass[e] = 1;
    for (int j = 0; j < m; ++j) {
      int first_unobs = -1;
      for (int i = 0; i < n; ++i) if (!h->mask[(size_t)j * n + i]) { first_unobs = i; break; }
      if (first_unobs >= 0) { G.ctype[j] = 0; G.slackrow[j] = first_unobs; } else { G.ctype[j] = 1; G.slackrow[j] = 0; }
    }
    G.nq = 0; G.nv1 = 0; G.nv2 = 0;
    G.mi.clear(); G.kid.clear(); G.cent.clear(); G.v1ent.clear(); G.v2ent.clear();
    G.cptr.assign((size_t)n * m + 1, 0); G.v1ptr.assign(1, 0); G.v2ptr.assign(1, 0);
  }
  G.r4 = shor_auto_r4(h, G.nq);
  return 0;
}

// ---- the same structure built on the device (omc_shor_index.hip) ---------------------------------------------------------------
// Scratch for lists of up to nq minors and a staging room of the given size.  The buffer only grows, and only with `grow` (no solve runs:
// stage time, the dual-bound evaluator, omc_shor_index_build); an append finds the room its stage call made.
static int shor_index_room(omc_instance* h, size_t nq, size_t stage_ints, size_t stage_bytes, bool grow) {
  const ShorIndexDims& have = h->sx_dims;
  const size_t soc_cap = std::max<size_t>((size_t)h->n * h->m, 1024);
  if (h->sxD.p && nq <= have.nq && stage_ints <= have.stage_ints && stage_bytes <= have.stage_bytes && soc_cap <= have.soc_cap) return 0;
  if (!grow) return fail(OMC_ERR_ALLOC, "Shor index structures on the device: the room made at stage time does not hold this list");
  ShorIndexDims d;
  d.nq = std::max(nq, have.nq); d.soc_cap = std::max(soc_cap, have.soc_cap);
  d.stage_ints = std::max(stage_ints, have.stage_ints); d.stage_bytes = std::max(stage_bytes, have.stage_bytes);
  size_t bytes = 0;
  if (carve_ensure(h->sxD, [&](Carve& c) { walk_shor_index(c, d, h->sx, h->sx_stage_int, h->sx_stage_byte); }, &bytes)) {
    (void)hipGetLastError();
    h->sx_dims = ShorIndexDims{};
    return fail(OMC_ERR_ALLOC, "Shor index structures on the device: " + std::to_string(bytes) + " bytes of scratch and staging room, which the device does not have (" + g_err + ")");
  }
  h->sx_dims = d;
  return 0;
}
static size_t shor_stage_ints(size_t nq, size_t nm, size_t m) { return 20 * nq + nm + m + 3; }
static size_t shor_stage_bytes(size_t nm, size_t m) { return (nm + m + 15) & ~(size_t)15; }
// the descriptor of one list whose arrays sit in the staging room at (st_int, st_byte)
static ShorIndexWS shor_index_view(omc_instance* h, int nq, int64_t nsoc, size_t st_int, size_t st_byte) {
  ShorIndexWS w = h->sx;
  const size_t nm = (size_t)h->n * h->m;
  w.n = h->n; w.m = h->m; w.nq = nq; w.soc_fill = nsoc < 0 ? 1 : 0; w.mask = h->dmask.as<uint8_t>();
  Carve c(h->sx_stage_int + st_int);
  walk_shor_index_list(c, (size_t)nq, nm, (size_t)h->m, w);
  w.eclass = h->sx_stage_byte + st_byte; w.ctype = w.eclass + nm;
  return w;
}
// Builds one list on stream s into the staging room and waits for its result word.  The refusals are the host builder's, in its order.
static int build_shor_group_device(omc_instance* h, hipStream_t s, int64_t nq64, const int64_t* idx, int64_t nsoc, const int64_t* soc,
                                   size_t st_int, size_t st_byte, bool want_ctype, ShorGroupHost& G) {
  const int nq = (int)nq64;
  const ShorIndexWS w = shor_index_view(h, nq, nsoc, st_int, st_byte);
  if (nq > 0) HIPCHK(hipMemcpyAsync(const_cast<long long*>(w.idx), idx, 32 * (size_t)nq, hipMemcpyHostToDevice, s));
  int launches = omc_shidx_launch_sort(&w, s);
  for (int64_t c0 = 0; c0 < nsoc; c0 += (int64_t)h->sx_dims.soc_cap) {
    const int64_t cnt = std::min<int64_t>(nsoc - c0, (int64_t)h->sx_dims.soc_cap);
    HIPCHK(hipMemcpyAsync(const_cast<long long*>(w.soc), soc + 2 * c0, 16 * (size_t)cnt, hipMemcpyHostToDevice, s));
    omc_shidx_launch_soc(&w, cnt, s);
  }
  launches += omc_shidx_launch_finish(&w, s);
  int meta[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(meta, w.meta, sizeof(meta), hipMemcpyDeviceToHost, s));
  if (want_ctype) { G.ctype.resize(h->m); HIPCHK(hipMemcpyAsync(G.ctype.data(), w.ctype, (size_t)h->m, hipMemcpyDeviceToHost, s)); }
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  h->shidx_stats[4] = launches;
  if (meta[0] & SHIDX_ERR_RANGE) return fail(OMC_ERR_ARGUMENT, SHOR_MSG_RANGE);
  if (meta[0] & SHIDX_ERR_DUP) return fail(OMC_ERR_ARGUMENT, SHOR_MSG_DUP);
  if (meta[0] & SHIDX_ERR_SOC) return fail(OMC_ERR_ARGUMENT, SHOR_MSG_SOC);
  G.dev = true; G.st_int = st_int; G.st_byte = st_byte; G.nm = (size_t)h->n * h->m; G.m = (size_t)h->m;
  G.nq = nq; G.nv1 = meta[1]; G.nv2 = meta[2];
  G.hash = fnv1a(idx, 32 * (size_t)nq, FNV_SEED);
  G.r4 = shor_auto_r4(h, nq);
  return 0;
}

// image of a group in the two index arenas: hi / hb are host images whose element 0 lands at dev_int / dev_byte on the device; the group's
// own offsets (off_int, off_byte) are relative to them
static void pack_shor_group(const ShorGroupHost& G, int* hi, uint8_t* hb, const int* dev_int, const uint8_t* dev_byte, ShorGroupDev& d) {
  size_t o = G.off_int;
  auto put = [&](const std::vector<int>& v) { const int* dp = dev_int + o; if (!v.empty()) memcpy(hi + o, v.data(), v.size() * sizeof(int)); o += v.size(); return dp; };
  d.nq = G.nq; d.nv1 = G.nv1; d.nv2 = G.nv2; d.pad = 0; d.hash = G.hash; d.r4 = G.r4;
  d.mi = put(G.mi); d.kid = put(G.kid); d.cptr = put(G.cptr); d.cent = put(G.cent);
  d.v1ptr = put(G.v1ptr); d.v1ent = put(G.v1ent); d.v2ptr = put(G.v2ptr); d.v2ent = put(G.v2ent); d.slackrow = put(G.slackrow);
  memcpy(hb + G.off_byte, G.eclass.data(), G.eclass.size());
  memcpy(hb + G.off_byte + G.eclass.size(), G.ctype.data(), G.ctype.size());
  d.eclass = dev_byte + G.off_byte; d.ctype = d.eclass + G.eclass.size();
}
// The same for a group built on the device: its arrays move from the staging room to the place the host image would have put them (the
// packed order and lengths of pack_shor_group; the padding behind the bytes is zeroed as the host image has it), on stream s.
static int place_shor_group_device(omc_instance* h, const ShorGroupHost& G, int* dev_int, uint8_t* dev_byte, ShorGroupDev& d, hipStream_t s) {
  const ShorIndexWS src = shor_index_view(h, G.nq, 0, G.st_int, G.st_byte);
  const size_t nq = (size_t)G.nq;
  int* o = dev_int + G.off_int;
  auto put = [&](const int* from, size_t count) { const int* dp = o; if (count && hipMemcpyAsync(o, from, count * sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess) return (const int*)nullptr; o += count; return dp; };
  d.nq = G.nq; d.nv1 = G.nv1; d.nv2 = G.nv2; d.pad = 0; d.hash = G.hash; d.r4 = G.r4;
  d.mi = put(src.mi, 12 * nq + G.nm + 1);      // mi, kid, cptr, cent: adjacent in both layouts (walk_shor_index_list)
  d.kid = d.mi + 4 * nq; d.cptr = d.kid + 4 * nq; d.cent = d.cptr + G.nm + 1;
  d.v1ptr = put(src.v1ptr, (size_t)G.nv1 + 1); d.v1ent = put(src.v1ent, 2 * nq);
  d.v2ptr = put(src.v2ptr, (size_t)G.nv2 + 1); d.v2ent = put(src.v2ent, 2 * nq);
  d.slackrow = put(src.slackrow, G.m);
  if (!d.mi || !d.v1ptr || !d.v2ptr || !d.slackrow || (nq && (!d.v1ent || !d.v2ent))) return fail(999, "hipMemcpyAsync (Shor index structures, staging room to arena) failed");
  uint8_t* b = dev_byte + G.off_byte;
  HIPCHK(hipMemcpyAsync(b, src.eclass, G.nm + G.m, hipMemcpyDeviceToDevice, s));
  if (G.bytes() > G.nm + G.m) HIPCHK(hipMemsetAsync(b + G.nm + G.m, 0, G.bytes() - (G.nm + G.m), s));
  d.eclass = b; d.ctype = b + G.nm;
  return 0;
}

// The host's filter of one node's warm-start indices (omc_relax_stage_shor and omc_relax_append_shor; the caller holds sig_mu): a load index that
// may not be used -- empty entry, saved by the base engine, larger than the reservation, not related by shor_warm_rule -- becomes -1 and is
// counted as refused; a save index of a list the reservation has no room for becomes -1.
static void shor_warm_filter(omc_instance* h, const omc_instance::PoolSig& sg, const int64_t* idx, int* load, int* save) {
  if (load && *load >= 0) {
    const omc_instance::PoolSig& pe = h->pool_sig[*load];
    int how = 0;
    if (pe.kind == 2 && pe.nq <= h->pool_nqmax && pe.nq <= sg.nq) {
      const bool same_head = pe.hlist == (pe.nq == sg.nq ? sg.hlist : fnv1a(idx, 32 * (size_t)pe.nq, FNV_SEED));
      how = shor_warm_rule(pe.nq, pe.nsoc, sg.nq, sg.nsoc, same_head, pe.nsoc == sg.nsoc && pe.hsoc == sg.hsoc);
    }
    if (how == 0) { *load = -1; ++h->shor_warm_stats[2]; } else ++h->shor_warm_stats[how - 1];
  }
  if (save && *save >= 0 && sg.nq > h->pool_nqmax) *save = -1;
}
// The lists a staged batch already knows and the room it has left for new ones (omc_relax_append_shor)
struct ShorKnownLists {
  const std::unordered_map<uint64_t, std::vector<int>>* byhash; const std::vector<ShorListKey>* lists;
  int group_cap; size_t int_room, byte_room; int nqmax, nv1max, nv2max;
};
// The nodes of a call grouped by identical (minor list, SOC list) pairs.  Group ids: the known lists first (their ids in the batch), the
// lists new with this call behind them in order of first appearance; `groups`, `lists`, `hashes` hold the new ones only, with arena
// offsets relative to the first of them.
struct ShorGrouping {
  std::vector<size_t> so, co;      // offsets of every node's tuples / pairs in the concatenated arrays (B + 1 each)
  std::vector<int> node_group;
  std::vector<ShorGroupHost> groups;
  std::unordered_map<uint64_t, std::vector<int>> byhash; std::vector<ShorListKey> lists; std::vector<uint64_t> hashes;
  size_t tot_int = 0, tot_byte = 0;
  int nqmax = 0, nv1max = 0, nv2max = 0;
  // set by the caller: lists with at least index_min minors (0: none) are built on the device on `stream`, whose scratch and staging room may
  // grow (never during an append) and are made to hold at least the room_* figures ; ctype of such a list is wanted on the host
  int index_min = 0; hipStream_t stream = nullptr; bool grow = true, want_ctype = false;
  size_t room_nq = 0, room_ints = 0, room_bytes = 0;
};
// Groups the nodes (out.so / out.co: from shor_list_offsets) and builds the index structure of every new list.  With `known`, a new list
// that the batch has no room for is refused (messages of omc_relax_append_shor); nothing is written anywhere but `out`.
static int group_shor_lists(omc_instance* h, int B, const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx,
                            const ShorKnownLists* known, ShorGrouping& out) {
  const int NG0 = known ? (int)known->lists->size() : 0;
  const size_t nm = (size_t)h->n * h->m, m = (size_t)h->m;
  const int index_min = h->k == 1 ? out.index_min : 0;      // rank k > 1: the host builder (its structure has no minors, quirk Q5)
  out.node_group.assign(B, 0);
  // which nodes bring a list new with this call, and which earlier node of the call has the same one: nothing is built or refused here
  std::vector<uint64_t> hv(B); std::vector<int> first_of(B, -1);
  {
    std::unordered_map<uint64_t, std::vector<int>> firsts;
    size_t dev_nq = out.room_nq, dev_ints = 0, dev_bytes = 0; bool any_dev = false;
    for (int b = 0; b < B; ++b) {
      const int64_t* ib = shor_idx + 4 * out.so[b]; const int64_t* sb = soc_idx + 2 * out.co[b];
      hv[b] = shor_pair_hash(n_shor[b], ib, n_soc[b], sb);
      const int gid = known ? find_shor_list(*known->byhash, *known->lists, hv[b], n_shor[b], ib, n_soc[b], sb) : -1;
      if (gid >= 0) { out.node_group[b] = gid; continue; }
      std::vector<int>& cand = firsts[hv[b]];
      int f = b;
      for (int c : cand)
        if (n_shor[c] == n_shor[b] && n_soc[c] == n_soc[b] && (n_shor[b] == 0 || memcmp(shor_idx + 4 * out.so[c], ib, 32 * (size_t)n_shor[b]) == 0) &&
            (n_soc[b] <= 0 || memcmp(soc_idx + 2 * out.co[c], sb, 16 * (size_t)n_soc[b]) == 0)) { f = c; break; }
      if (f == b) {
        cand.push_back(b);
        if (index_min > 0 && n_shor[b] >= index_min) {
          any_dev = true; dev_nq = std::max(dev_nq, (size_t)n_shor[b]);
          dev_ints += shor_stage_ints((size_t)n_shor[b], nm, m); dev_bytes += shor_stage_bytes(nm, m);
        }
      }
      first_of[b] = f;
    }
    if (any_dev && out.grow) {
      int rcr = shor_index_room(h, dev_nq, std::max(dev_ints, out.room_ints), std::max(dev_bytes, out.room_bytes), true);
      if (rcr) return rcr;
    }
  }
  size_t st_int = 0, st_byte = 0;      // staging room used by the lists built on the device so far
  for (int b = 0; b < B; ++b) {
    if (first_of[b] < 0) continue;      // a list the batch knows
    if (first_of[b] != b) { out.node_group[b] = out.node_group[first_of[b]]; continue; }
    const int64_t* ib = shor_idx + 4 * out.so[b]; const int64_t* sb = soc_idx + 2 * out.co[b];
    {      // a list new with this call: built here, so that the first refusal in node order is the one reported
      if (known && n_shor[b] > known->nqmax)
        return fail(OMC_ERR_ARGUMENT, "omc_relax_append_shor: a list has " + std::to_string(n_shor[b]) + " minors, the batch has room for " + std::to_string(known->nqmax) + " per node (nq_max of omc_relax_reserve_shor)");
      if (known && NG0 + (int)out.lists.size() >= known->group_cap)
        return fail(OMC_ERR_ARGUMENT, "omc_relax_append_shor: a new list, and the list capacity of the batch (" + std::to_string(known->group_cap) + " lists: staged + extra_lists of omc_relax_reserve_shor) is used up");
      out.groups.emplace_back();
      ShorGroupHost& G = out.groups.back();
      const auto t0 = std::chrono::steady_clock::now();
      const bool dev = index_min > 0 && n_shor[b] >= index_min;
      if (dev) {
        const size_t need_i = shor_stage_ints((size_t)n_shor[b], nm, m), need_b = shor_stage_bytes(nm, m);
        { int rcr = shor_index_room(h, (size_t)n_shor[b], st_int + need_i, st_byte + need_b, false); if (rcr) return rcr; }
        int rc0 = build_shor_group_device(h, out.stream, n_shor[b], ib, n_soc[b], sb, st_int, st_byte, out.want_ctype, G);
        if (rc0) return rc0;
        st_int += need_i; st_byte += need_b;
      } else {
        int rc0 = build_shor_group(h, n_shor[b], ib, n_soc[b], sb, G); if (rc0) return rc0;
      }
      h->shidx_stats[dev ? 1 : 0] += 1.0;
      h->shidx_stats[dev ? 3 : 2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      out.nqmax = std::max(out.nqmax, G.nq); out.nv1max = std::max(out.nv1max, G.nv1); out.nv2max = std::max(out.nv2max, G.nv2);
      G.off_int = out.tot_int; out.tot_int += G.ints();
      G.off_byte = out.tot_byte; out.tot_byte += G.bytes();
      if (known && (G.nv1 > known->nv1max || G.nv2 > known->nv2max || out.tot_int > known->int_room || out.tot_byte > known->byte_room))
        return fail(OMC_ERR_ARGUMENT, "omc_relax_append_shor: a new list does not fit the index room reserved by omc_relax_reserve_shor (list capacity used up)");
      out.node_group[b] = NG0 + (int)out.lists.size();
      add_shor_list(out.byhash, out.lists, hv[b], n_shor[b], ib, n_soc[b], sb);
      out.hashes.push_back(hv[b]);
    }
  }
  return 0;
}

// Host images of the new groups of `g` and their copies to the given arena positions, the group table and the nodes' group ids, enqueued on s.
// The images must live until the caller has synchronised s.
struct ShorGroupImages { std::vector<int> hi; std::vector<uint8_t> hb; std::vector<ShorGroupDev> gd; };
static int upload_shor_groups(omc_instance* h, const ShorGrouping& g, int* dev_int, uint8_t* dev_byte, ShorGroupDev* dev_groups, int* dev_node_group, hipStream_t s,
                              ShorGroupImages& img) {
  if (!g.groups.empty()) {
    bool any_dev = false;
    for (const ShorGroupHost& G : g.groups) any_dev = any_dev || G.dev;
    img.hi.assign(g.tot_int, 0); img.hb.assign(g.tot_byte, 0); img.gd.resize(g.groups.size());
    for (size_t q = 0; q < g.groups.size(); ++q) if (!g.groups[q].dev) pack_shor_group(g.groups[q], img.hi.data(), img.hb.data(), dev_int, dev_byte, img.gd[q]);
    if (!any_dev) {
      HIPCHK(hipMemcpyAsync(dev_int, img.hi.data(), g.tot_int * sizeof(int), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(dev_byte, img.hb.data(), g.tot_byte, hipMemcpyHostToDevice, s));
    } else {      // group by group: the host's part of the images, and the staging room's lists (s is the stream they were built on)
      for (size_t q = 0; q < g.groups.size(); ++q) {
        const ShorGroupHost& G = g.groups[q];
        if (G.dev) { int rcp = place_shor_group_device(h, G, dev_int, dev_byte, img.gd[q], s); if (rcp) return rcp; continue; }
        HIPCHK(hipMemcpyAsync(dev_int + G.off_int, img.hi.data() + G.off_int, G.ints() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dev_byte + G.off_byte, img.hb.data() + G.off_byte, G.bytes(), hipMemcpyHostToDevice, s));
      }
    }
    HIPCHK(hipMemcpyAsync(dev_groups, img.gd.data(), sizeof(ShorGroupDev) * img.gd.size(), hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemcpyAsync(dev_node_group, g.node_group.data(), sizeof(int) * g.node_group.size(), hipMemcpyHostToDevice, s));
  return 0;
}

}  // namespace

int omc_relax_reserve_shor(omc_instance* h, int64_t nq_max, int extra_lists) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (nq_max < 0 || extra_lists < 0) return fail(OMC_ERR_ARGUMENT, "omc_relax_reserve_shor: negative argument");
  if (nq_max >= (1ll << 28)) return fail(OMC_ERR_ARGUMENT, "omc_relax_reserve_shor: nq_max out of range");
  h->reserve_shor_nq = nq_max; h->reserve_shor_lists = extra_lists; h->reserve_shor_set = true;
  return 0;
}

// ---- one list's index structure, returned to the caller (omc.h) ---------------------------------------------------------------------------------
int omc_shor_index_plan(int n, int m, int64_t nq, int64_t* out) {
  if (!out) return fail(OMC_ERR_ARGUMENT, "omc_shor_index_plan: out is NULL");
  if (n <= 0 || m <= 0 || nq < 0) return fail(OMC_ERR_ARGUMENT, "omc_shor_index_plan: n and m must be positive, nq not negative");
  if (nq >= (1ll << 28) || (long long)n * m >= (1ll << 30)) return fail(OMC_ERR_UNSUPPORTED, "omc_shor_index_plan: beyond the size limits of omc_relax_stage_shor");
  const ShorIndexPlan P = shor_index_plan(n, m, nq);
  ShorIndexDims d;
  d.nq = (size_t)nq; d.soc_cap = std::max<size_t>((size_t)n * m, 1024);
  ShorIndexWS w{}; int* si = nullptr; uint8_t* sb = nullptr;
  Carve measure;
  walk_shor_index(measure, d, w, si, sb);
  out[0] = P.p_v1; out[1] = P.p_v2; out[2] = P.p_co; out[3] = P.p_dup;
  out[4] = (int64_t)measure.bytes();
  out[5] = (int64_t)shor_stage_ints((size_t)nq, (size_t)n * m, (size_t)m); out[6] = (int64_t)shor_stage_bytes((size_t)n * m, (size_t)m);
  out[7] = P.launches; out[8] = SHIDX_TILE;
  return 0;
}

int omc_last_shor_index_stats(omc_instance* h, double* out) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  for (int q = 0; q < 5; ++q) out[q] = h->shidx_stats[q];
  return 0;
}

int omc_shor_index_build(omc_instance* h, int where, int64_t nq, const int64_t* shor_idx, int64_t n_soc, const int64_t* soc_idx, int64_t* counts,
                         double* r4, uint64_t* hash, int* mi, int* kid, int* cptr, int* cent, int* v1ptr, int* v1ent, int* v2ptr, int* v2ent,
                         int* slackrow, uint8_t* eclass, uint8_t* ctype) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "omc_shor_index_build: handle is NULL");
  if (where != 0 && where != 1) return fail(OMC_ERR_ARGUMENT, "omc_shor_index_build: where is 0 (host) or 1 (device)");
  if (h->worker.joinable() || h->worker_running.load()) return fail(OMC_ERR_ARGUMENT, "omc_shor_index_build: a solve is in flight on this handle (call omc_relax_wait first)");
  if (where == 1 && h->k > 1) return fail(OMC_ERR_UNSUPPORTED, "omc_shor_index_build: rank k > 1 has no device builder (its structure has no minors, quirk Q5)");
  const size_t n = h->n, m = h->m, nm = n * m;
  if ((long long)n * (long long)m >= (1ll << 30)) return fail(OMC_ERR_UNSUPPORTED, "Shor mode: n * m too large for the 32-bit index structures");
  { std::vector<size_t> so, co; int rc0 = shor_list_offsets(1, &nq, shor_idx, &n_soc, soc_idx, so, co); if (rc0) return rc0; }
  ShorGroupHost G;
  if (where == 0) {
    { int rc0 = build_shor_group(h, nq, shor_idx, n_soc, soc_idx, G); if (rc0) return rc0; }
    auto give = [](auto* dst, const auto& v) { if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    give(mi, G.mi); give(kid, G.kid); give(cptr, G.cptr); give(cent, G.cent); give(v1ptr, G.v1ptr); give(v1ent, G.v1ent);
    give(v2ptr, G.v2ptr); give(v2ent, G.v2ent); give(slackrow, G.slackrow); give(eclass, G.eclass); give(ctype, G.ctype);
  } else {
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    { int rcr = shor_index_room(h, (size_t)nq, shor_stage_ints((size_t)nq, nm, m), shor_stage_bytes(nm, m), true); if (rcr) return rcr; }
    { int rc0 = build_shor_group_device(h, s, nq, shor_idx, n_soc, soc_idx, 0, 0, false, G); if (rc0) return rc0; }
    const ShorIndexWS w = shor_index_view(h, G.nq, 0, 0, 0);
    const size_t q = (size_t)G.nq;
    auto back = [&](void* dst, const void* src, size_t bytes) { return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess; };
    HIPCHK(back(mi, w.mi, 16 * q)); HIPCHK(back(kid, w.kid, 16 * q)); HIPCHK(back(cptr, w.cptr, 4 * (nm + 1))); HIPCHK(back(cent, w.cent, 16 * q));
    HIPCHK(back(v1ptr, w.v1ptr, 4 * ((size_t)G.nv1 + 1))); HIPCHK(back(v1ent, w.v1ent, 8 * q));
    HIPCHK(back(v2ptr, w.v2ptr, 4 * ((size_t)G.nv2 + 1))); HIPCHK(back(v2ent, w.v2ent, 8 * q));
    HIPCHK(back(slackrow, w.slackrow, 4 * m)); HIPCHK(back(eclass, w.eclass, nm)); HIPCHK(back(ctype, w.ctype, m));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (counts) { counts[0] = G.nq; counts[1] = G.nv1; counts[2] = G.nv2; counts[3] = where == 1 ? (int64_t)h->shidx_stats[4] : 0; }
  if (r4) *r4 = G.r4;
  if (hash) *hash = G.hash;
  return 0;
}

int omc_relax_stage_shor(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L, const double* cut_x,
                         const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower, const double* U_upper,
                         const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  if (!n_shor || !n_soc) return fail(OMC_ERR_ARGUMENT, "n_shor / n_soc is NULL");
  if (h->keep_shor_cert && h->k > 1)
    return fail(OMC_ERR_UNSUPPORTED, "omc_relax_stage_shor: Shor-mode certificates are kept (omc_relax_keep_shor_certificates) and rank k > 1 has no certificate layout (its minors are vacuous, quirk Q5)");
  if (h->keep_cert && !h->keep_shor_cert) return fail(OMC_ERR_UNSUPPORTED, "omc_relax_stage_shor: certificates are kept (omc_relax_keep_certificates) and the Shor-mode bound has multipliers the certificate layout does not hold");
  const int n = h->n, m = h->m;
  if ((long long)n * m >= (1ll << 30)) return fail(OMC_ERR_UNSUPPORTED, "Shor mode: n * m too large for the 32-bit index structures");
  // ---- group the nodes by identical lists ------------------------------------------------------------------------------------------
  ShorGrouping grp;      // its lists are kept in the handle for the life of the batch
  { int rc0 = shor_list_offsets(B, n_shor, shor_idx, n_soc, soc_idx, grp.so, grp.co); if (rc0) return rc0; }
  for (int q = 0; q < 5; ++q) h->shidx_stats[q] = 0.0;
  h->sh_index_min = h->k == 1 ? std::max(h->tun.shor_index_device_min, 0) : 0;      // the staged batch keeps the knob's value: its appends follow it
  if (h->sh_index_min > 0) {
    // lists built on the device: on the instance's stream ; the scratch and the staging room also hold what an append may bring (a call's new
    // lists: at most extra_lists of them, none longer than the batch's stride), so that an append allocates nothing
    HIPCHK(hipSetDevice(h->device));
    grp.index_min = h->sh_index_min; grp.stream = h->stream;
    if (h->reserve_shor_set) {
      int64_t nq_all = h->reserve_shor_nq;
      for (int b = 0; b < B; ++b) nq_all = std::max(nq_all, n_shor[b]);
      grp.room_nq = (size_t)nq_all;
      grp.room_ints = (size_t)h->reserve_shor_lists * shor_stage_ints((size_t)nq_all, (size_t)n * m, (size_t)m);
      grp.room_bytes = (size_t)h->reserve_shor_lists * shor_stage_bytes((size_t)n * m, (size_t)m);
      if (grp.room_ints) { int rcr = shor_index_room(h, grp.room_nq, grp.room_ints, grp.room_bytes, true); if (rcr) return rcr; }
    }
  }
  { int rc0 = group_shor_lists(h, B, n_shor, shor_idx, n_soc, soc_idx, nullptr, grp); if (rc0) return rc0; }
  const std::vector<size_t>& so = grp.so; const std::vector<size_t>& co = grp.co;
  const std::vector<ShorGroupHost>& gh = grp.groups; const std::vector<int>& node_group = grp.node_group;
  const int NG = (int)gh.size();
  int nqmax = grp.nqmax, nv1max = grp.nv1max, nv2max = grp.nv2max;
  const size_t tot_int = grp.tot_int, tot_byte = grp.tot_byte;
  // omc_relax_reserve_shor: consumed by this call
  const bool res_set = h->reserve_shor_set; const int64_t res_nq = res_set ? h->reserve_shor_nq : 0; const int res_lists = res_set ? h->reserve_shor_lists : 0;
  h->reserve_shor_set = false; h->reserve_shor_nq = 0; h->reserve_shor_lists = 0;
  // ---- rank k > 1 with an unobserved entry in every column: the program without order-5 blocks IS the base relaxation (theta_j >= x_j' Y^+ x_j
  // implies theta_j >= ||x_j||^2 because Y <= I, and the slack of Theta_jj = sum_i W_ij sits on an unobserved entry at no cost): the base engine
  // solves it (no order-(n+m) cone), omc_relax_fetch_shor completes W = X^2 + slack from its (X, Theta).
  if (h->k > 1) {
    bool all_free = true;
    for (int g = 0; g < NG && all_free; ++g) for (int j = 0; j < m; ++j) if (gh[g].ctype[j] != 0) { all_free = false; break; }
    if (all_free && !h->tun.shor_explicit) {
      h->warm_load.clear(); h->warm_save.clear();      // warm-start indices are not honoured on this path (include/omc.h)
      int rc0 = omc_relax_stage(h, B, params, cut_type, L, cut_x, cut_Uhat, cut_dir, U_lower, U_upper);
      if (rc0) return rc0;
      h->shor_via_base = true;
      h->shor_slackrow = gh[0].slackrow;      // first unobserved row of every column (a property of the mask: the same for every list)
      return 0;
    }
  }
  // ---- warm start: the indices of omc_relax_set_warm pass the host's filter, so that the kernels see a plain "warm or cold" per node ------
  // With omc_relax_reserve and a pool both index arrays exist (omc_relax_stage fills what was not given with -1): appended nodes may name entries.
  for (int q = 0; q < 4; ++q) h->shor_warm_stats[q] = 0;
  StageMode mode;
  mode.shor = true;
  const int extra_nodes = h->reserve_nodes;      // consumed by omc_relax_stage below
  if (h->pool_cap > 0 && h->pool_shor && h->k == 1 && (h->warm_load.size() == (size_t)B || h->warm_save.size() == (size_t)B || extra_nodes > 0)) {
    std::lock_guard<std::mutex> lk(h->sig_mu);
    h->node_sig.assign((size_t)B + (size_t)extra_nodes, omc_instance::PoolSig{});
    for (int b = 0; b < B; ++b) {
      omc_instance::PoolSig& sg = h->node_sig[b];
      sg.kind = 2; sg.nq = n_shor[b]; sg.nsoc = n_soc[b]; sg.hlist = gh[node_group[b]].hash;
      sg.hsoc = n_soc[b] > 0 ? fnv1a(soc_idx + 2 * co[b], 16 * (size_t)n_soc[b], FNV_SEED) : 0;
      shor_warm_filter(h, sg, shor_idx + 4 * so[b], h->warm_load.size() == (size_t)B ? &h->warm_load[b] : nullptr,
                       h->warm_save.size() == (size_t)B ? &h->warm_save[b] : nullptr);
    }
    mode.warm_filtered = true;
  } else {
    h->warm_load.clear(); h->warm_save.clear();      // no reservation (or rank k > 1): ignored
  }
  // ---- base staging (rows, small cone, clip, certificate machinery) with the Shor flag ----------------------------------------------
  int rc = stage_base(h, B, params, cut_type, L, cut_x, cut_Uhat, cut_dir, U_lower, U_upper, mode);
  if (rc) return rc;
  h->staged = false;
  OmcWS& w = h->ws;
  const int S = w.B, N = n + m;
  hipStream_t s = h->stream;
  // ---- strides and capacities: the staged lists, or what omc_relax_reserve_shor asked for (a minor has two V1 and two V2 keys: nv <= 2 nq) ----
  if (res_set) {
    nqmax = (int)std::max<int64_t>(nqmax, res_nq);
    nv1max = std::max(nv1max, 2 * nqmax); nv2max = std::max(nv2max, 2 * nqmax);
  }
  const size_t int_cap = tot_int + (size_t)res_lists * ((size_t)20 * (size_t)res_nq + (size_t)n * m + (size_t)m + 3);
  const size_t byte_cap = tot_byte + (size_t)res_lists * ((((size_t)n * m + (size_t)m) + 15) & ~(size_t)15);
  // ---- upload the index structures ------------------------------------------------------------------------------------------------
  {
    if ((rc = h->sgInts.ensure(int_cap * sizeof(int)))) return rc;
    if ((rc = h->sgBytes.ensure(byte_cap))) return rc;
    if ((rc = h->sgGroups.ensure(sizeof(ShorGroupDev) * ((size_t)NG + (size_t)res_lists)))) return rc;
    if ((rc = h->sgNodeGroup.ensure(sizeof(int) * (size_t)h->node_cap))) return rc;
    ShorGroupImages img;
    if ((rc = upload_shor_groups(h, grp, h->sgInts.as<int>(), h->sgBytes.as<uint8_t>(), h->sgGroups.as<ShorGroupDev>(), h->sgNodeGroup.as<int>(), s, img))) return rc;
    HIPCHK(hipStreamSynchronize(s));          // the host images die with this block
  }
  h->sh_byhash = std::move(grp.byhash); h->sh_lists = std::move(grp.lists);
  h->sh_group_cap = NG + res_lists; h->sh_int_used = tot_int; h->sh_int_cap = int_cap; h->sh_byte_used = tot_byte; h->sh_byte_cap = byte_cap;
  // ---- scaling: the program is homogeneous of degree 2 in A (oracle: shor_scale) -------------------------------------------------------
  const double sc = shor_scale(h);
  {
    std::vector<double> Ah((size_t)n * m);
    for (size_t e = 0; e < Ah.size(); ++e) Ah[e] = h->A[e] * sc;
    if ((rc = upload(h->sAh, Ah.data(), 8 * Ah.size(), s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
  }
  // ---- state ---------------------------------------------------------------------------------------------------------------------------
  ShWS& sh = h->sh;
  memset(&sh, 0, sizeof(sh));
  const size_t sB = (size_t)S, sN = (size_t)h->node_cap, nm = (size_t)n * m;      // per-node outputs: room for the appended nodes too
  const int NPb = (N + 15) & ~15;
  const int nmb = std::max(1, (nqmax + 255) / 256);
  const size_t nq1 = (size_t)std::max(nqmax, 1), nv11 = (size_t)std::max(nv1max, 1), nv21 = (size_t)std::max(nv2max, 1);
  ENS(h->sX, sB * nm * 8); ENS(h->sW, sB * nm * 8); ENS(h->sTh, sB * m * m * 8);
  ENS(h->sV1, sB * nv11 * 8); ENS(h->sV2, sB * nv21 * 8); ENS(h->sV3, sB * nq1 * 8);
  ENS(h->sD0, sB * N * N * 8); ENS(h->sP0, sB * N * N * 8); ENS(h->sMbufB, sB * NPb * NPb * 8); ENS(h->sVrowB, sB * NPb * NPb * 8);
  ENS(h->sTq, sB * 15 * nq1 * 8); ENS(h->sPq, sB * 15 * nq1 * 8); ENS(h->sNq, sB * 15 * nq1 * 8);
  ENS(h->sD5x, sB * nm * 8); ENS(h->sD5t, sB * m * 8); ENS(h->snu5, sB * m * 8); ENS(h->sP5x, sB * nm * 8);
  ENS(h->scolpart, sB * m * 4 * 8); ENS(h->sminpart, sB * nmb * 8); ENS(h->sminpart2, sB * nmb * 8);
  ENS_CARVE(h->sfroB, [&](Carve& c) { walk_shor_fro(c, sB, sh); }); ENS(h->svvB, sB * sizeof(int)); ENS(h->se1, sB * nv11 * 8); ENS(h->se2, sB * nv21 * 8);
  ENS(h->soX, sN * nm * 8); ENS(h->soW, sN * nm * 8); ENS(h->soTh, sN * m * m * 8);
  HIPCHK(hipMemsetAsync(h->sMbufB.p, 0, sB * NPb * NPb * 8, s));
  HIPCHK(hipMemsetAsync(h->sVrowB.p, 0, sB * NPb * NPb * 8, s));
  HIPCHK(hipMemsetAsync(h->sminpart.p, 0, sB * nmb * 8, s));
  HIPCHK(hipMemsetAsync(h->sminpart2.p, 0, sB * nmb * 8, s));
  HIPCHK(hipMemsetAsync(h->soX.p, 0, sN * nm * 8, s)); HIPCHK(hipMemsetAsync(h->soW.p, 0, sN * nm * 8, s)); HIPCHK(hipMemsetAsync(h->soTh.p, 0, sN * m * m * 8, s));
  sh.n = n; sh.m = m; sh.k = h->k; sh.N = N; sh.NPb = NPb; sh.S = S; sh.Btot = B; sh.nqmax = nqmax; sh.nv1max = nv1max; sh.nv2max = nv2max; sh.nmb = nmb;
  sh.rx = w.relax; sh.r4 = h->shor_r4; sh.r5 = h->shor_r5; sh.gamma = h->gamma; sh.sc = sc;
  sh.groups = h->sgGroups.as<ShorGroupDev>(); sh.node_group = h->sgNodeGroup.as<int>();
  sh.node_of = w.node_of; sh.done = w.done; sh.init = w.init; sh.fin = w.fin; sh.rho_b = w.rho_b; sh.bfac = w.bfac;
  sh.Ah = h->sAh.as<double>(); sh.mask = h->dmask.as<uint8_t>();
  sh.X = h->sX.as<double>(); sh.W = h->sW.as<double>(); sh.Th = h->sTh.as<double>();
  sh.V1 = h->sV1.as<double>(); sh.V2 = h->sV2.as<double>(); sh.V3 = h->sV3.as<double>();
  sh.D0 = h->sD0.as<double>(); sh.P0 = h->sP0.as<double>(); sh.MbufB = h->sMbufB.as<double>(); sh.VrowB = h->sVrowB.as<double>();
  sh.Tq = h->sTq.as<double>(); sh.Pq = h->sPq.as<double>(); sh.Nq = h->sNq.as<double>();
  sh.D5x = h->sD5x.as<double>(); sh.D5t = h->sD5t.as<double>(); sh.nu5 = h->snu5.as<double>(); sh.P5x = h->sP5x.as<double>();
  sh.colpart = h->scolpart.as<double>(); sh.minpart = h->sminpart.as<double>(); sh.minpart2 = h->sminpart2.as<double>();
  sh.vvalidB = h->svvB.as<int>();
  sh.Y = w.Y; sh.Yp = w.Yp; sh.rp = w.rp; sh.rd = w.rd;
  sh.e1 = h->se1.as<double>(); sh.e2 = h->se2.as<double>();
  sh.objcol = w.objcol; sh.c0col = w.c0col; sh.lamDX = w.lamDX;
  sh.oX = h->soX.as<double>(); sh.oW = h->soW.as<double>(); sh.oTh = h->soTh.as<double>();
  sh.oV = nullptr;
  if (w.load_from || w.save_to) {      // indices that passed the filter above: the Shor extension of the pool beside the base entries
    const ShorPoolLayout PL = shor_pool_layout(n, m, (int)h->pool_nqmax);
    sh.load_from = w.load_from; sh.save_to = w.save_to; sh.pscal = w.pscal; sh.pY = w.pY; sh.rho_node = w.rho_node;
    sh.pS = h->pShor.as<double>(); sh.pShdr = h->pShorHdr.as<long long>(); sh.pstride = PL.stride; sh.pnq = (int)h->pool_nqmax;
    ENS(h->sloadpart, sB * NPb * 2 * 8); sh.loadpart = h->sloadpart.as<double>();
  }
  if (h->keep_shor_cert) {      // best certificate per node, Shor part: blocks, paraboloid multipliers and points, per slot and per node of the capacity; zeroed
    size_t cb_bytes = 0, oc_bytes = 0;
    if (carve_ensure(h->scbD, [&](Carve& c) { walk_shor_cert(c, sB, nq1, m, nm, sh.cbGam, sh.cbZeta, sh.cbXi, sh.cbXbar); }, &cb_bytes) ||
        carve_ensure(h->socD, [&](Carve& c) { walk_shor_cert(c, sN, nq1, m, nm, sh.ocGam, sh.ocZeta, sh.ocXi, sh.ocXbar); }, &oc_bytes) ||
        h->socNq.ensure(sN * sizeof(int))) {
      (void)hipGetLastError();
      return fail(OMC_ERR_ALLOC, "omc_relax_stage_shor: the Shor-mode certificates need " + std::to_string(cb_bytes / sB) + " bytes per slot (" + std::to_string(S) +
                                 ") and per node of the capacity (" + std::to_string(h->node_cap) + "), which the device does not have (" + g_err + ")");
    }
    HIPCHK(hipMemsetAsync(h->scbD.p, 0, cb_bytes, s)); HIPCHK(hipMemsetAsync(h->socD.p, 0, oc_bytes, s)); HIPCHK(hipMemsetAsync(h->socNq.p, 0, sN * sizeof(int), s));
    sh.ocNq = h->socNq.as<int>(); sh.cert_flag = w.cert_flag; sh.cb_rho = w.cb_rho;
  }
  if (h->shor_keep_V) { ENS(h->soV, sN * 5 * nq1 * 8); HIPCHK(hipMemsetAsync(h->soV.p, 0, sN * 5 * nq1 * 8, s)); sh.oV = h->soV.as<double>(); }
  // ---- base workspace in Shor mode, and the view through which its eigen-kernels project the order-(n+m) cone -------------------------
  w.shor = 1; w.shN = N; w.shP0 = sh.P0; w.shD0 = sh.D0; w.inv_s2 = 1.0 / (sc * sc);
  OmcWS& wb = h->wbig;
  wb = w;
  wb.n = N; wb.np16 = NPb; wb.Mbuf = sh.MbufB; wb.Vrow = sh.VrowB; wb.vvalid = sh.vvalidB; wb.fro2 = sh.fro2B; wb.W1 = sh.P0;
  wb.sub_enable = 0; wb.cert_enable = 0; wb.ws_mode = 0; wb.clip_hi = 1e300; wb.sub_debug = 0; wb.ws_first = nullptr; wb.ws_need = nullptr; wb.ws_phase = 0;
  // the view's own geometry (only the eigen-kernels are launched through it)
  wb.geo = omc_plan_geometry(N, NPb, wb.k, wb.rmax, wb.Rmax, h->cmax, h->tun.global_nolds, h->tun.cone_multi_min, MW_MAX_ORDER + 1);
  ENS(h->sbigmw, sB * 4 * sizeof(int)); HIPCHK(hipMemsetAsync(h->sbigmw.p, 0, sB * 4 * sizeof(int), s));
  wb.mw_stat = h->sbigmw.as<int>();
  if (wb.geo.ws.slab_stride) { ENS(h->sbigscr, sB * wb.geo.ws.slab_stride * 8); wb.cone_scratch = h->sbigscr.as<double>(); }
  // the big cone's input has a handful of positive eigenvalues once the iterate has settled (measured: 2 - 5 of n + m): the tracked-subspace
  // kernel of the base engine follows them; the warm-started full kernel seeds the block and is the fall-back
  wb.trM = sh.trB;
  if (wb.geo.ws_lpp && N >= 48 && wb.geo.sub_lds <= OMC_MAX_DYN_LDS && !h->tun.no_subspace && !h->tun.shor_no_subspace) {
    size_t subI_bytes = 0;
    ENS(h->sXsB, sB * NPb * 16 * 8); ENS(h->ssubSB, sB * 16 * 8);
    ENS_CARVE(h->ssubIB, [&](Carve& c) { walk_shor_sub_ints(c, sB, sh, wb); }, &subI_bytes);
    HIPCHK(hipMemsetAsync(h->sXsB.p, 0, sB * NPb * 16 * 8, s));
    HIPCHK(hipMemsetAsync(h->ssubSB.p, 0, sB * 16 * 8, s));
    HIPCHK(hipMemsetAsync(h->ssubIB.p, 0, subI_bytes, s));
    wb.sub_enable = 1; wb.Xs = h->sXsB.as<double>(); wb.sub_theta = h->ssubSB.as<double>();
    wb.sub_zscratch = nullptr;
    if (NPb > 512) { ENS(h->bsubz, sB * 16 * (size_t)(NPb + 2) * 8); wb.sub_zscratch = h->bsubz.as<double>(); }
    wb.ws_first = nullptr; wb.ws_need = nullptr; wb.ws_phase = 0; wb.sub_on = sh.sub_onB; wb.cone_done = sh.cone_doneB; wb.sub_wait = sh.sub_waitB; wb.sub_nfail = sh.sub_nfailB;
    wb.sep_done = nullptr;
  }
  HIPCHK(hipStreamSynchronize(s));
  h->shor_on = true;
  h->staged = true;
  return 0;
}

int omc_set_shor_keep_V(omc_instance* h, int keep) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  h->shor_keep_V = keep != 0;
  return 0;
}

int omc_relax_fetch_shor_V(omc_instance* h, double* V) {
  if (!h || !h->staged || !h->shor_on) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_shor_V: no Shor-mode batch staged");
  if (!h->sh.oV) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_shor_V: V was not kept (call omc_set_shor_keep_V(h, 1) before staging)");
  if (!V) return fail(OMC_ERR_ARGUMENT, "V is NULL");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(V, h->sh.oV, 8 * (size_t)h->sh.Btot * 5 * (size_t)std::max(h->sh.nqmax, 1), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int omc_last_shor_subspace_stats(omc_instance* h, int64_t* out) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  for (int q = 0; q < 8; ++q) out[q] = h->big_sub_tot[q];
  return 0;
}

int omc_relax_fetch_shor(omc_instance* h, double* W) {
  if (h && h->staged && h->shor_via_base) {      // rank k > 1 served by the base engine: W = X^2, the slack Theta_jj - ||x_j||^2 on the column's first unobserved row
    if (!W) return 0;
    const size_t B = h->ws.Btot, n = h->n, m = h->m;
    std::vector<double> X(B * n * m), Th(B * m * m);
    int rc = omc_relax_fetch(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, X.data(), Th.data(), nullptr, nullptr, nullptr);
    if (rc) return rc;
    for (size_t b = 0; b < B; ++b)
      for (size_t j = 0; j < m; ++j) {
        double s2 = 0.0;
        for (size_t i = 0; i < n; ++i) { const double x = X[(b * m + j) * n + i]; W[(b * m + j) * n + i] = x * x; s2 += x * x; }
        W[(b * m + j) * n + h->shor_slackrow[j]] += Th[(b * m + j) * m + j] - s2;
      }
    return 0;
  }
  if (!h || !h->staged || !h->shor_on) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_shor: no Shor-mode batch staged");
  HIPCHK(hipSetDevice(h->device));
  if (W) HIPCHK(hipMemcpyAsync(W, h->sh.oW, 8 * (size_t)h->sh.Btot * h->n * h->m, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int omc_relax_batch_shor(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L, const double* cut_x,
                         const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower, const double* U_upper,
                         const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx, double* objective,
                         double* dual_bound, int* status, int* iters, double* Y, double* U, double* X, double* Theta, double* W,
                         double* lambda_min, double* breakpoint_x, double* solve_time) {
  int rc = omc_relax_stage_shor(h, B, params, cut_type, L, cut_x, cut_Uhat, cut_dir, U_lower, U_upper, n_shor, shor_idx, n_soc, soc_idx);
  if (rc) return rc;
  rc = omc_relax_solve(h);
  if (rc) return rc;
  rc = omc_relax_fetch(h, objective, dual_bound, status, iters, Y, U, X, Theta, lambda_min, breakpoint_x, solve_time);
  if (rc) return rc;
  return omc_relax_fetch_shor(h, W);
}

// ---- appending Shor nodes to a staged / running Shor batch (rank 1) ---------------------------------------------------------------------
// The Shor form of omc_relax_append: same lock, same end-of-batch decision, descriptors first and the counter last.  A node whose lists the
// batch already knows (staged or appended) shares that group; a new list is built by build_shor_group and written into the room that
// omc_relax_reserve_shor reserved in the index arenas and the group table, behind everything the running kernels can reach (they find a list
// through node_group of a node below Btot_live).  Every refusal is decided before anything is written: a refused call leaves the batch as it was.
int omc_relax_append_shor(omc_instance* h, int B2, const int* L, const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir,
                          const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx,
                          const int* load_from, const int* save_to) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (h->k > 1) return fail(OMC_ERR_UNSUPPORTED, "omc_relax_append_shor: rank k > 1 is not supported (a batch served by the base engine takes omc_relax_append)");
  if (!h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_append_shor: nothing staged");
  if (!h->shor_on) return fail(OMC_ERR_ARGUMENT, "omc_relax_append_shor: the staged batch is not in Shor mode (omc_relax_append)");
  if (B2 <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  if (!n_shor || !n_soc) return fail(OMC_ERR_ARGUMENT, "n_shor / n_soc is NULL");
  const ShorAppendLists lists = {n_shor, shor_idx, n_soc, soc_idx};
  return append_nodes(h, "omc_relax_append_shor", B2, L, cut_x, cut_Uhat, cut_dir, load_from, save_to, &lists);
}

// lists: known ones share their group, new ones are built (and may still be refused); then the warm-start filter of stage time, where
// node_sig lets the harvest sign the entry an appended node saves to
static int shor_append_plan(omc_instance* h, int first, int B2, const ShorAppendLists& l, std::vector<int>& load, std::vector<int>& save, ShorGrouping& g) {
  const ShWS& sh = h->sh;
  const ShorKnownLists known = {&h->sh_byhash, &h->sh_lists, h->sh_group_cap, h->sh_int_cap - h->sh_int_used, h->sh_byte_cap - h->sh_byte_used,
                                sh.nqmax, sh.nv1max, sh.nv2max};
  { int rc0 = shor_list_offsets(B2, l.n_shor, l.shor_idx, l.n_soc, l.soc_idx, g.so, g.co); if (rc0) return rc0; }
  g.index_min = h->sh_index_min; g.stream = h->append_stream; g.grow = false;      // device builds: on the append stream, in the room of stage time
  { int rc0 = group_shor_lists(h, B2, l.n_shor, l.shor_idx, l.n_soc, l.soc_idx, &known, g); if (rc0) return rc0; }
  if (load.empty()) return 0;      // the batch has no warm-start arrays
  const int NG0 = (int)h->sh_lists.size();
  std::lock_guard<std::mutex> lk2(h->sig_mu);
  for (int b = 0; b < B2; ++b) {
    omc_instance::PoolSig sg;
    sg.kind = 2; sg.nq = l.n_shor[b]; sg.nsoc = l.n_soc[b];
    sg.hlist = g.node_group[b] < NG0 ? h->sh_lists[g.node_group[b]].hlist : g.lists[g.node_group[b] - NG0].hlist;
    sg.hsoc = l.n_soc[b] > 0 ? fnv1a(l.soc_idx + 2 * g.co[b], 16 * (size_t)l.n_soc[b], FNV_SEED) : 0;
    shor_warm_filter(h, sg, l.shor_idx + 4 * g.so[b], &load[b], &save[b]);
    h->node_sig[(size_t)first + b] = sg;      // sized for node_cap at stage time; read by the solve only below Btot_live
  }
  return 0;
}

// the new groups go into the room that omc_relax_reserve_shor reserved in the index arenas and the group table, behind everything the
// running kernels can reach (they find a list through node_group of a node below Btot_live)
static int shor_append_write(omc_instance* h, const ShorGrouping& g, int first, hipStream_t s, ShorGroupImages& img) {
  return upload_shor_groups(h, g, h->sgInts.as<int>() + h->sh_int_used, h->sgBytes.as<uint8_t>() + h->sh_byte_used,
                            h->sgGroups.as<ShorGroupDev>() + h->sh_lists.size(), h->sgNodeGroup.as<int>() + first, s, img);
}

static void shor_append_commit(omc_instance* h, ShorGrouping& g) {
  for (size_t q = 0; q < g.lists.size(); ++q) {
    h->sh_byhash[g.hashes[q]].push_back((int)h->sh_lists.size());
    h->sh_lists.push_back(std::move(g.lists[q]));
  }
  h->sh_int_used += g.tot_int; h->sh_byte_used += g.tot_byte;
}

// The one append path: omc_relax_append, and with `lists` omc_relax_append_shor, whose list step (known lists share their group, new ones
// are built and may be refused) sits between the checks and the writes.  Lock, end-of-batch decision, capacity, rows, strides and pool
// indices first: every refusal is decided before anything is written, and a refused call leaves the batch as it was.  Then the new groups,
// the descriptors, rho_node and the warm-start indices on the append stream, and the counter last: the running kernels read the
// descriptors of nodes below Btot_live only, so these rows are not visible to them until it moves.
static int append_nodes(omc_instance* h, const char* who, int B2, const int* L, const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir,
                        const int* load_from, const int* save_to, const ShorAppendLists* lists) {
  const std::string pre = std::string(who) + ": ";
  HIPCHK(hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(h->append_mu);
  if (h->append_closed) return fail(OMC_ERR_ARGUMENT, pre + "the solve of this batch has ended (stage a new batch)");
  const OmcWS& w = h->ws;
  const int first = h->Btot_live.load();
  if (first + B2 > h->node_cap) return fail(OMC_ERR_ARGUMENT, pre + (lists ? "beyond the node capacity given to omc_relax_reserve" : "beyond the capacity given to omc_relax_reserve"));
  NodePack pk;
  { int rcp = pack_nodes(h, h->params, h->staged_cut_type, B2, L, cut_x, cut_Uhat, cut_dir, nullptr, nullptr, pk); if (rcp) return rcp; }
  if (pk.Rmax > w.Rmax || pk.rmax > w.rmax || pk.Lmax > w.Lmax) return fail(OMC_ERR_ARGUMENT, pre + "a node has more cuts than omc_relax_reserve allowed for");
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
  { int rc = put_descriptors(w, pk, B2, B2, f, L, cut_x, as); if (rc) return rc; }
  std::vector<double> hrho(B2, w.rho);
  HIPCHK(hipMemcpyAsync(const_cast<double*>(w.rho_node) + f, hrho.data(), 8 * (size_t)B2, hipMemcpyHostToDevice, as));
  if (!lfv.empty()) HIPCHK(hipMemcpyAsync(const_cast<int*>(w.load_from) + f, lfv.data(), sizeof(int) * B2, hipMemcpyHostToDevice, as));
  if (!svv.empty()) {
    HIPCHK(hipMemcpyAsync(const_cast<int*>(w.save_to) + f, svv.data(), sizeof(int) * B2, hipMemcpyHostToDevice, as));
    for (int b = 0; b < B2; ++b) h->save_host[f + b] = svv[b];      // sized for node_cap at stage time; read by the solve only below Btot_live
  }
  HIPCHK(hipStreamSynchronize(as));
  if (lists) shor_append_commit(h, grouping);
  h->Btot_live.store(first + B2); h->Btot = first + B2;
  if (!h->worker_running.load()) { h->ws.Btot = first + B2; if (lists) h->sh.Btot = first + B2; }      // no solve in flight: the staged batch simply grew (a running solve sets both when it ends)
  return 0;
}

// X, W, Theta of nodes that omc_relax_fetch_done has already returned, copied from the per-node outputs on the fetch stream while the solve
// runs (the harvest wrote them before the id was queued).  The values omc_relax_fetch / omc_relax_fetch_shor give after the solve.
int omc_relax_fetch_done_shor(omc_instance* h, int n_ids, const int* node_ids, double* X, double* W, double* Theta) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (!h->staged || !h->shor_on) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_done_shor: no Shor-mode batch staged");
  if (n_ids < 0 || (n_ids > 0 && !node_ids)) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_done_shor: bad arguments");
  if (n_ids == 0) return 0;
  { int rcf = require_finished_ids(h, n_ids, node_ids, true, "omc_relax_fetch_done_shor"); if (rcf) return rcf; }
  HIPCHK(hipSetDevice(h->device));
  if (!h->fetch_stream) HIPCHK(hipStreamCreateWithFlags(&h->fetch_stream, hipStreamNonBlocking));
  hipStream_t fs = h->fetch_stream;
  const size_t nm = (size_t)h->n * h->m, mm = (size_t)h->m * h->m;
  for (int i = 0; i < n_ids; ++i) {
    const size_t nb = (size_t)node_ids[i];
    if (X) HIPCHK(hipMemcpyAsync(X + i * nm, h->sh.oX + nb * nm, 8 * nm, hipMemcpyDeviceToHost, fs));
    if (W) HIPCHK(hipMemcpyAsync(W + i * nm, h->sh.oW + nb * nm, 8 * nm, hipMemcpyDeviceToHost, fs));
    if (Theta) HIPCHK(hipMemcpyAsync(Theta + i * mm, h->sh.oTh + nb * mm, 8 * mm, hipMemcpyDeviceToHost, fs));
  }
  HIPCHK(hipStreamSynchronize(fs));
  return 0;
}

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
  if (w.geo.ws.slab_stride) { ENS(h->dbS, sB * w.geo.ws.slab_stride * 8); w.cone_scratch = h->dbS.as<double>(); }
  if (n > 144) { ENS(h->dbL, sB * m * n * 8); HIPCHK(hipMemsetAsync(h->dbL.p, 0, sB * m * n * 8, s)); w.lamDX = h->dbL.as<double>(); }
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
  {
    size_t dbytes = 0;
    int rca = carve_ensure(h->sdD, [&](Carve& cv) { walk_scert_doubles(cv, sd, d, c, in, w, a); }, &dbytes);
    if (!rca) rca = carve_ensure(h->sdI, [&](Carve& cv) { walk_scert_ints(cv, sd, d, c, in, w, a); });
    if (!rca) rca = h->sdGi.ensure(grp.tot_int * sizeof(int));
    if (!rca) rca = h->sdGb.ensure(grp.tot_byte);
    if (!rca) rca = h->sdGr.ensure(sizeof(ShorGroupDev) * (size_t)NG);
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
    { int rc = upload_shor_groups(h, grp, h->sdGi.as<int>(), h->sdGb.as<uint8_t>(), h->sdGr.as<ShorGroupDev>(), in.node_group, s, img); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(in.view_node, view_node.data(), sizeof(int) * sV, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(in.view_way, view_way.data(), sizeof(int) * sV, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));          // the host images die with this block
  }
  c.groups = (const ShorGroupDev*)h->sdGr.p; c.A = h->dA.as<double>(); c.mask = h->dmask.as<uint8_t>();
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
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  HIPCHK(hipEventCreate(&ev0)); HIPCHK(hipEventCreate(&ev1));
  HIPCHK(hipEventRecord(ev0, s));
  if (want_clean) omc_scert_launch_clean(&c, store_clean ? 1 : 0, s);
  if (nqmax > 0) { omc_scert_launch_keys(&c, s); omc_scert_launch_minor(&c, s); }
  omc_scert_launch_cols(&c, s);
  const OmcDualIn din = {nullptr, a.lam, Psi3 ? a.Psi : nullptr, a.T1, c.c0col, c.colbad};
  omc_launch_dual_assemble(&w, &din, s);
  std::vector<double> scl, cmu(sV * m), mpart(sV * nmb * 2 + 1), cpart(sB * nmb + 1);
  std::vector<int> cbad(sV * m);
  { int rc = eval_view_solve(w, a, ev1, scl, s); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(cmu.data(), c.colmu, sV * m * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(cbad.data(), c.colbad, sV * m * sizeof(int), hipMemcpyDeviceToHost, s));
  if (nmb && defects) {
    HIPCHK(hipMemcpyAsync(mpart.data(), c.minpart, sV * nmb * 2 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cpart.data(), c.cleanpart, sB * nmb * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  { float msf = 0.f; HIPCHK(hipEventElapsedTime(&msf, ev0, ev1)); h->sdb_ms = msf; }
  (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
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

int omc_evaluate_objective(omc_instance* h, int B, const double* X, double* objective) {
  if (!h || !X || !objective) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (B <= 0) return fail(OMC_ERR_ARGUMENT, "B must be positive");
  HIPCHK(hipSetDevice(h->device));
  const size_t n = h->n, m = h->m;
  int r_ = h->bXin.ensure(8 * (size_t)B * n * m + 8 * (size_t)B + 64); if (r_) return r_;
  double* dX = h->bXin.as<double>();
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
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~PlainCall() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  int launch(omc_instance* h, const OmcWS& w, int mode) {
    if (w.geo.plain_mw) { HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); HIPCHK(hipEventRecord(e0, h->stream)); }
    omc_launch_cone(&w, mode, h->stream);
    if (w.geo.plain_mw) HIPCHK(hipEventRecord(e1, h->stream));
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
    float msv = 0.f; HIPCHK(hipEventElapsedTime(&msv, e0, e1));
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
  ENS(h->bXin, (size_t)B * n * m * 8);
  HIPCHK(hipMemcpyAsync(h->bXin.p, X, 8 * (size_t)B * n * m, hipMemcpyHostToDevice, h->stream));
  omc_launch_gram_XXt(&w, h->bXin.as<double>(), B, h->stream);
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
  ENS(h->pjM, sB * NP * NP * 8); ENS(h->pjV, sB * NP * NP * 8); ENS(h->pjW, sB * N * N * 8);
  int* ints_end = nullptr;
  ENS_CARVE(h->pjD, [&](Carve& c) { walk_project_doubles(c, sB, NP, w); });
  ENS_CARVE(h->pjI, [&](Carve& c) { walk_project_ints(c, sB, w, ints_end); });
  if (w.geo.ws.slab_stride) { ENS(h->pjS, sB * w.geo.ws.slab_stride * 8); w.cone_scratch = h->pjS.as<double>(); }
  w.Mbuf = h->pjM.as<double>(); w.Vrow = h->pjV.as<double>(); w.W1 = h->pjW.as<double>();
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
  else HIPCHK(hipMemsetAsync(w.Vrow, 0, sB * NP * NP * 8, s));
  HIPCHK(hipMemcpyAsync(w.fro2, hf.data(), sB * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(ip, hi_.data(), hi_.size() * sizeof(int), hipMemcpyHostToDevice, s));
  hipEvent_t e0 = nullptr, e1 = nullptr;      // device time of the projection alone (uploads and downloads outside)
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  struct EvGuard { hipEvent_t &a, &b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evg{e0, e1};
  HIPCHK(hipEventRecord(e0, s));
  if (cold) omc_launch_cone(&w, CONE_BIG, s); else omc_launch_cone_ws(&w, s);
  HIPCHK(hipEventRecord(e1, s));
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
  { float msv = 0.f; HIPCHK(hipEventElapsedTime(&msv, e0, e1)); h->mw_tot[4] = (long long)(1000.0 * msv); }
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
  ENS(h->bnfact, sB * m * sizeof(int));
  w.cp_nfact = h->bnfact.as<int>();
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
  if ((rc_ = h->aU.ensure(8 * sB * n * k))) return rc_;
  if ((rc_ = h->aV.ensure(8 * sB * m * k))) return rc_;
  if ((rc_ = h->aobj.ensure(8 * sB * max_iters))) return rc_;
  if ((rc_ = h->aint.ensure(4 * sB * 2))) return rc_;
  if ((rc_ = h->amobj.ensure(8 * sB))) return rc_;
  h->amobj_B = B;
  if ((rc_ = h->aG.ensure(8 * sB * Rmax * Rmax))) return rc_;
  AltminWS w{};
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
  w.U0 = h->aU0.as<double>(); w.U = h->aU.as<double>(); w.V = h->aV.as<double>(); w.objectives = h->aobj.as<double>();
  w.converged = h->aint.as<int>(); w.n_iters = h->aint.as<int>() + B; w.G = h->aG.as<double>(); w.mobj = h->amobj.as<double>();
  // a problem that does not fit the LDS (config 5: 1000 x 1000, k = 2 needs 144 KB) runs the same kernel on a per-problem global slab
  const KernelPlan ap = altmin_plan(n, m, k, Rmax, h->tun.altmin_nolds);
  w.scratch = nullptr; w.scratch_stride = ap.slab_stride; w.lds_bytes = ap.lds_bytes;
  if (ap.slab_stride) { ENS(h->aG2, (size_t)B * ap.slab_stride * 8); w.scratch = h->aG2.as<double>(); }
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

// ---------------------------------------------------------------------------------------------------------------------
// Shor minors: generate_rank1_matrix_completion_Shor_constraints_indexes (OMC.jl:2545-2612) and
// generate_violated_Shor_minors (OMC.jl:2614-2640).  Kernels in omc_shor.hip; the host only sequences the segments.
// ---------------------------------------------------------------------------------------------------------------------
struct ShorSeg { int kind, la, lb; };
// two timing events that are destroyed on every exit path
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int create() { if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 1; return 0; }
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
static void shor_segments(int n_classes, const int* classes, bool dedup, std::vector<ShorSeg>& segs) {
  bool seen[5] = {false, false, false, false, false};
  for (int c = 0; c < n_classes; ++c) {
    const int p = classes[c];
    if (p < 0 || p > 4) continue;                 // the reference's if/elseif chain has no branch for other values
    if (dedup) { if (seen[p]) continue; seen[p] = true; }
    if (p == 4) segs.push_back({SH_COMBO, SH_BOTH, 0});                                       // OMC.jl:2556-2561
    else if (p == 3) segs.push_back({SH_PRODUCT, SH_BOTH, SH_XOR});                           // 2562-2569
    else if (p == 2) { segs.push_back({SH_PRODUCT, SH_BOTH, SH_NONE}); segs.push_back({SH_COMBO, SH_XOR, 0}); }  // 2570-2584
    else if (p == 1) segs.push_back({SH_PRODUCT, SH_XOR, SH_NONE});                           // 2585-2596
    else segs.push_back({SH_COMBO, SH_NONE, 0});                                              // 2597-2608
  }
}
static int shor_prepare(omc_instance* h) {
  if (h->shor_ready) return 0;
  const int n = h->n, m = h->m;
  if (m > 8192) return fail(OMC_ERR_UNSUPPORTED, "Shor enumeration supports m <= 8192 in this build");
  HIPCHK(hipSetDevice(h->device));
  const int W = (m + 63) / 64;
  std::vector<uint64_t> bits((size_t)n * W, 0);
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < n; ++i)
      if (h->mask[(size_t)j * n + i]) bits[(size_t)i * W + (j >> 6)] |= (1ULL << (j & 63));
  const long long np = (long long)n * (n - 1) / 2;
  int rc;
  if ((rc = upload(h->sbits, bits.data(), bits.size() * 8, h->stream))) return rc;
  if ((rc = h->scb.ensure((size_t)std::max(np, 1LL) * 4)) || (rc = h->scx.ensure((size_t)std::max(np, 1LL) * 4)) ||
      (rc = h->scz.ensure((size_t)std::max(np, 1LL) * 4)) || (rc = h->soff.ensure((size_t)std::max(np, 1LL) * 8)) ||
      (rc = h->stot.ensure(64)) || (rc = h->shist.ensure(256 * 8)) || (rc = h->scnt.ensure(64)))
    return rc;
  omc_shor_launch_pair_counts(n, m, W, h->sbits.as<uint64_t>(), np, h->scb.as<int>(), h->scx.as<int>(), h->scz.as<int>(), h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));   // `bits` is a host temporary
  h->shor_W = W; h->shor_pairs = np; h->shor_ready = true;
  return 0;
}
// scan segment `sg` with offsets starting at `base`; returns its total
static int shor_scan(omc_instance* h, const ShorSeg& sg, long long base, long long* total) {
  omc_shor_launch_seg_scan(sg.kind, sg.la, sg.lb, h->scb.as<int>(), h->scx.as<int>(), h->scz.as<int>(), h->shor_pairs, base,
                           h->soff.as<long long>(), h->stot.as<long long>(), h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(total, h->stot.p, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int omc_shor_count(omc_instance* h, int n_classes, const int* num_entries_present, int64_t* count_per_class) {
  if (!h || (n_classes > 0 && !num_entries_present) || !count_per_class) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  int rc = shor_prepare(h);
  if (rc) return rc;
  for (int c = 0; c < n_classes; ++c) {
    std::vector<ShorSeg> segs;
    shor_segments(1, num_entries_present + c, false, segs);
    long long tot = 0;
    for (const ShorSeg& sg : segs) { long long t = 0; if ((rc = shor_scan(h, sg, 0, &t))) return rc; tot += t; }
    count_per_class[c] = tot;
  }
  return 0;
}

int omc_shor_indexes(omc_instance* h, int n_classes, const int* num_entries_present, int64_t capacity, int64_t* out, int64_t* count) {
  if (!h || (n_classes > 0 && !num_entries_present) || !count) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  int rc = shor_prepare(h);
  if (rc) return rc;
  std::vector<ShorSeg> segs;
  shor_segments(n_classes, num_entries_present, false, segs);
  std::vector<long long> tot(segs.size(), 0);
  long long total = 0;
  for (size_t q = 0; q < segs.size(); ++q) { if ((rc = shor_scan(h, segs[q], 0, &tot[q]))) return rc; total += tot[q]; }
  *count = total;
  if (!out || capacity < total || total == 0) return 0;      // size query (or nothing to write)
  if ((rc = h->sout.ensure((size_t)total * 32))) return rc;
  EventPair ev;
  if (ev.create()) return fail(999, "hipEventCreate failed");
  hipEvent_t e0 = ev.e0, e1 = ev.e1;
  HIPCHK(hipEventRecord(e0, h->stream));
  long long base = 0;
  for (size_t q = 0; q < segs.size(); ++q) {
    long long t = 0;
    if ((rc = shor_scan(h, segs[q], base, &t))) return rc;
    omc_shor_launch_enum_tuples(h->n, h->m, h->shor_W, h->sbits.as<uint64_t>(), segs[q].kind, segs[q].la, segs[q].lb,
                                h->soff.as<long long>(), h->shor_pairs, h->sout.as<long long>(), h->stream);
    HIPCHK(hipGetLastError());
    base += t;
  }
  HIPCHK(hipEventRecord(e1, h->stream));
  HIPCHK(hipMemcpyAsync(out, h->sout.p, (size_t)total * 32, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  h->shor_last_ms = ms; h->shor_last_candidates = total;
  return 0;
}

// MSD radix select of the K largest of the N 128-bit keys (hi, lo), 1 <= K <= N: finds a digit prefix (*bhi, *blo) such that the keys >= it are
// the K largest and at most SHOR_SEL_CAP more, and emits those to sohi / solo (*got of them, in no particular order)
static const long long SHOR_SEL_CAP = 8192;
static int shor_select_emit(omc_instance* h, long long N, long long K, uint64_t* bhi, uint64_t* blo, unsigned long long* got) {
  uint64_t phi = 0, plo = 0; long long need = K; unsigned long long bin = 0;
  for (int level = 0; level < 16; ++level) {
    HIPCHK(hipMemsetAsync(h->shist.p, 0, 256 * 8, h->stream));
    omc_shor_launch_hist(N, h->shi.as<uint64_t>(), h->slo.as<uint64_t>(), phi, plo, level, h->shist.as<unsigned long long>(), h->stream);
    HIPCHK(hipGetLastError());
    unsigned long long hist[256];
    HIPCHK(hipMemcpyAsync(hist, h->shist.p, sizeof(hist), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    long long cum = 0; int d = 255;
    for (; d > 0; --d) { if (cum + (long long)hist[d] >= need) break; cum += (long long)hist[d]; }
    need -= cum; bin = hist[d];
    if (level < 8) phi |= (uint64_t)d << (56 - 8 * level); else plo |= (uint64_t)d << (56 - 8 * (level - 8));
    if ((long long)bin - need <= SHOR_SEL_CAP) break;
  }
  const unsigned long long cap = (unsigned long long)(K + SHOR_SEL_CAP + 16);
  int rc;
  if ((rc = h->sohi.ensure(cap * 8)) || (rc = h->solo.ensure(cap * 8))) return rc;
  HIPCHK(hipMemsetAsync((char*)h->scnt.p + 8, 0, 8, h->stream));
  omc_shor_launch_emit(N, h->shi.as<uint64_t>(), h->slo.as<uint64_t>(), phi, plo, h->sohi.as<uint64_t>(), h->solo.as<uint64_t>(),
                       h->scnt.as<unsigned long long>() + 1, cap, h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(got, (char*)h->scnt.p + 8, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (*got > cap || (long long)*got < K) return fail(OMC_ERR_ARGUMENT, "internal: radix select emitted an unexpected number of keys");
  *bhi = phi; *blo = plo;
  return 0;
}

// Streaming selection: the K largest keys without the key of every candidate in memory.  The segments are walked in tiles of
// consecutive row pairs; the enumerator keeps the candidates at or above the threshold in a buffer of `capacity` keys (shi / slo), and
// whenever enough new keys have arrived the radix select above reduces it to the K largest (+ at most SHOR_SEL_CAP) and its boundary becomes the
// threshold.  Keys are unique, so the K largest are a unique set whatever the tiles and the order of the appends; on return they are in
// sohi / solo (*got of them) exactly as the materialised path leaves them.
//   capacity = max(budget / 16, K + SHOR_SEL_CAP + largest candidate count of one row pair in one segment): after a compaction at most
//   K + SHOR_SEL_CAP keys remain, so a tile of one pair always fits and the walk terminates for any budget.
static int shor_stream_select(omc_instance* h, const std::vector<ShorSeg>& segs, long long n_existing_keys, long long K, long long budget_bytes,
                              unsigned long long* got) {
  const int n = h->n, m = h->m, k = h->k;
  const long long np = h->shor_pairs;
  int rc;
  // per-pair offsets of every segment on the host (off[np] = the segment's total)
  std::vector<std::vector<long long>> hoff(segs.size());
  long long maxpair = 0;
  for (size_t q = 0; q < segs.size(); ++q) {
    hoff[q].resize((size_t)np + 1);
    if ((rc = shor_scan(h, segs[q], 0, &hoff[q][(size_t)np]))) return rc;
    HIPCHK(hipMemcpyAsync(hoff[q].data(), h->soff.p, (size_t)np * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (long long t = 0; t < np; ++t) maxpair = std::max(maxpair, hoff[q][(size_t)t + 1] - hoff[q][(size_t)t]);
  }
  const long long nominal = std::max<long long>(budget_bytes / 16, 1);      // the buffer the budget asks for; tiles and compactions are paced by it
  const long long capacity = std::max(nominal, K + SHOR_SEL_CAP + maxpair);
  if ((rc = h->shi.ensure((size_t)capacity * 8)) || (rc = h->slo.ensure((size_t)capacity * 8))) return rc;
  h->shor_sel[3] = 16 * capacity;
  unsigned long long* d_count = h->scnt.as<unsigned long long>() + 2;       // survivor counter; the overflow flag is the word after it
  unsigned int* d_flag = (unsigned int*)(h->scnt.as<unsigned long long>() + 3);
  uint64_t thi = 0, tlo = 0;                                                 // every key is >= (0, 1): the first tiles keep every candidate
  long long count = 0, compacted_at = 0;
  auto set_count = [&](long long c) -> int {
    const unsigned long long w[2] = {(unsigned long long)c, 0ULL};
    HIPCHK(hipMemcpyAsync(d_count, w, 16, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                                 // `w` is a stack temporary
    return 0;
  };
  auto compact = [&]() -> int {                                              // count > K
    unsigned long long g = 0;
    int r = shor_select_emit(h, count, K, &thi, &tlo, &g);
    if (r) return r;
    HIPCHK(hipMemcpyAsync(h->shi.p, h->sohi.p, g * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->slo.p, h->solo.p, g * 8, hipMemcpyDeviceToDevice, h->stream));
    count = compacted_at = (long long)g;
    ++h->shor_sel[2];
    return set_count(count);
  };
  if ((rc = set_count(0))) return rc;
  const long long TILE_MAX = 1LL << 32;      // candidates: ~0.1 s of the scorer, so the host looks at the counter often enough
  double gain = 1.0;                         // candidates per free slot that the last tile's survival rate allows (half the free space filled)
  // while most candidates survive (no threshold yet, or scores that grow along the enumeration) a tile can only fill the buffer: such tiles start
  // at 1/64 of the budget, so that the first threshold costs a small select, and double as long as that goes on
  long long probe = std::min(nominal, std::max(nominal / 64, 65536LL));
  for (size_t q = 0; q < segs.size(); ++q) {
    const long long* off = hoff[q].data();
    long long p = 0, forced = 0;             // forced > 0: candidate limit of a tile that is being run again after an overflow
    bool compacted_for_tile = false;
    while (p < np) {
      if (off[np] == off[p]) break;          // nothing left in this segment
      if (off[p + 1] - off[p] > capacity - count) { if ((rc = compact())) return rc; }      // count > K + SHOR_SEL_CAP here, so this frees the room
      const long long free_ = capacity - count, base = std::min(free_, probe);
      long long L = forced > 0 ? forced : (long long)std::min((double)TILE_MAX, std::max((double)base, (double)base * gain));
      long long p1 = (long long)(std::upper_bound(off + p + 1, off + np + 1, off[p] + L) - off) - 1;      // last p1 with off[p1] - off[p] <= L
      if (p1 <= p) p1 = p + 1;
      const long long c = off[p1] - off[p];
      if (c == 0) { p = p1; continue; }
      omc_shor_launch_enum_stream(n, m, h->shor_W, h->sbits.as<uint64_t>(), segs[q].kind, segs[q].la, segs[q].lb, p, p1, h->bXin.as<double>(), k,
                                  h->sexist.as<uint64_t>(), n_existing_keys, thi, tlo, h->shi.as<uint64_t>(), h->slo.as<uint64_t>(), d_count,
                                  (unsigned long long)capacity, d_flag, h->stream);
      HIPCHK(hipGetLastError());
      unsigned long long w[2] = {0, 0};
      HIPCHK(hipMemcpyAsync(w, d_count, 16, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      if ((unsigned int)w[1] != 0 || (long long)w[0] > capacity) {
        // overflow: the tile is discarded.  Once, the buffer is compacted (if it holds anything new) and the same tile run again under the
        // raised threshold; after that the tile is halved until it fits -- one pair always does
        if ((rc = set_count(count))) return rc;
        if (!compacted_for_tile && count > K && count != compacted_at) { if ((rc = compact())) return rc; compacted_for_tile = true; forced = c; }
        else forced = std::max(c / 2, 1LL);
        continue;
      }
      const long long s = (long long)w[0] - count;
      count = (long long)w[0];
      ++h->shor_sel[1];
      gain = (double)c / (2.0 * (double)std::max(s, 1LL));
      p = p1; forced = 0; compacted_for_tile = false;
      if (count > K && count > compacted_at && (count - compacted_at > std::min(capacity, probe) / 2 || count > capacity / 2)) { if ((rc = compact())) return rc; }
      if (2 * s > c) probe = std::min(2 * probe, nominal);
    }
  }
  if (count < K) return fail(OMC_ERR_ARGUMENT, "internal: streaming selection kept fewer keys than requested");
  uint64_t bhi, blo;
  return shor_select_emit(h, count, K, &bhi, &blo, got);
}

int omc_violated_shor_minors(omc_instance* h, const double* X, int n_classes, const int* num_entries_present, int64_t n_existing,
                             const int64_t* existing, int n_minors, double* scores, int64_t* minors, int* n_out) {
  if (!h || !X || (n_classes > 0 && !num_entries_present) || (n_existing > 0 && !existing) || !n_out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (n_minors < 0 || n_existing < 0) return fail(OMC_ERR_ARGUMENT, "negative count");
  if (n_minors > 0 && (!scores || !minors)) return fail(OMC_ERR_ARGUMENT, "NULL output");
  *n_out = 0;
  int rc = shor_prepare(h);
  if (rc) return rc;
  const int n = h->n, m = h->m, k = h->k;
  std::vector<ShorSeg> segs;
  shor_segments(n_classes, num_entries_present, true, segs);   // setdiff! also removes duplicates (OMC.jl:2626)
  std::vector<long long> tot(segs.size(), 0);
  long long N = 0;
  for (size_t q = 0; q < segs.size(); ++q) { if ((rc = shor_scan(h, segs[q], 0, &tot[q]))) return rc; N += tot[q]; }
  const long long budget = (long long)std::max(h->tun.shor_select_kb, 0) * 1024;
  const bool stream = budget > 0 && N > budget / 16;           // 16 bytes of key per candidate
  h->shor_sel[0] = stream ? 1 : 0; h->shor_sel[1] = h->shor_sel[2] = h->shor_sel[3] = 0;
  if (N == 0 || n_minors == 0) return 0;
  // keys of the existing constraints, sorted and unique
  std::vector<uint64_t> ex; ex.reserve((size_t)n_existing);
  for (int64_t e = 0; e < n_existing; ++e) {
    const int64_t i1 = existing[4 * e] - 1, i2 = existing[4 * e + 1] - 1, j1 = existing[4 * e + 2] - 1, j2 = existing[4 * e + 3] - 1;
    if (i1 < 0 || i1 >= n || i2 < 0 || i2 >= n || j1 < 0 || j1 >= m || j2 < 0 || j2 >= m) continue;   // cannot equal any candidate
    ex.push_back((((uint64_t)i1 * n + i2) * m + j1) * m + j2 + 1);
  }
  std::sort(ex.begin(), ex.end()); ex.erase(std::unique(ex.begin(), ex.end()), ex.end());
  if ((rc = upload(h->sexist, ex.data(), ex.size() * 8, h->stream))) return rc;
  if ((rc = upload(h->bXin, X, sizeof(double) * (size_t)k * n * m, h->stream))) return rc;
  EventPair ev;
  if (ev.create()) return fail(999, "hipEventCreate failed");
  hipEvent_t e0 = ev.e0, e1 = ev.e1;
  long long K = 0; unsigned long long got = 0;
  if (stream) {
    // the excluded candidates are the distinct existing tuples that are candidates of a requested class: counted here, not per candidate
    bool want[5] = {false, false, false, false, false};
    for (int c = 0; c < n_classes; ++c) if (num_entries_present[c] >= 0 && num_entries_present[c] <= 4) want[num_entries_present[c]] = true;
    long long excluded = 0;
    for (uint64_t key : ex) {
      uint64_t r = key - 1;
      const uint64_t j2 = r % m; r /= m;
      const uint64_t j1 = r % m; r /= m;
      const uint64_t i2 = r % n, i1 = r / n;
      if (!(i1 < i2 && j1 < j2)) continue;
      const int pc = h->mask[(size_t)j1 * n + i1] + h->mask[(size_t)j2 * n + i1] + h->mask[(size_t)j1 * n + i2] + h->mask[(size_t)j2 * n + i2];
      if (want[pc]) ++excluded;
    }
    K = std::min<long long>(n_minors, N - excluded);            // fewer candidates than n_minors: all of them, sorted (OMC.jl:2634-2635)
    HIPCHK(hipEventRecord(e0, h->stream));
    if (K > 0 && (rc = shor_stream_select(h, segs, (long long)ex.size(), K, budget, &got))) return rc;
  } else {
    if ((rc = h->shi.ensure((size_t)N * 8)) || (rc = h->slo.ensure((size_t)N * 8))) return rc;
    h->shor_sel[3] = 16 * N;
    HIPCHK(hipMemsetAsync(h->scnt.p, 0, 16, h->stream));
    HIPCHK(hipEventRecord(e0, h->stream));
    long long base = 0;
    for (size_t q = 0; q < segs.size(); ++q) {
      long long t = 0;
      if ((rc = shor_scan(h, segs[q], base, &t))) return rc;
      omc_shor_launch_enum_keys(n, m, h->shor_W, h->sbits.as<uint64_t>(), segs[q].kind, segs[q].la, segs[q].lb, h->soff.as<long long>(),
                                h->shor_pairs, h->bXin.as<double>(), k, h->sexist.as<uint64_t>(), (long long)ex.size(),
                                h->shi.as<uint64_t>(), h->slo.as<uint64_t>(), h->scnt.as<unsigned long long>(), h->stream);
      HIPCHK(hipGetLastError());
      base += t;
    }
    unsigned long long excluded = 0;
    HIPCHK(hipMemcpyAsync(&excluded, h->scnt.p, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    K = std::min<long long>(n_minors, N - (long long)excluded);  // fewer candidates than n_minors: all of them, sorted (OMC.jl:2634-2635)
    uint64_t bhi, blo;
    if (K > 0 && (rc = shor_select_emit(h, N, K, &bhi, &blo, &got))) return rc;
  }
  if (K > 0) {
    HIPCHK(hipEventRecord(e1, h->stream));
    std::vector<uint64_t> ohi(got), olo(got);
    HIPCHK(hipMemcpyAsync(ohi.data(), h->sohi.p, got * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(olo.data(), h->solo.p, got * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<size_t> ord(got);
    for (size_t i = 0; i < got; ++i) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return ohi[a] != ohi[b] ? ohi[a] > ohi[b] : olo[a] > olo[b]; });
    for (long long r = 0; r < K; ++r) {
      const size_t i = ord[(size_t)r];
      double sc; memcpy(&sc, &ohi[i], 8);
      scores[r] = sc;
      uint64_t key = olo[i] - 1;
      const uint64_t j2 = key % m; key /= m;
      const uint64_t j1 = key % m; key /= m;
      const uint64_t i2 = key % n; const uint64_t i1 = key / n;
      minors[4 * r] = (int64_t)i1 + 1; minors[4 * r + 1] = (int64_t)i2 + 1; minors[4 * r + 2] = (int64_t)j1 + 1; minors[4 * r + 3] = (int64_t)j2 + 1;
    }
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    h->shor_last_ms = ms; h->shor_last_candidates = N;
  }
  *n_out = (int)K;
  return 0;
}

int omc_shor_last_stats(omc_instance* h, double* ms, int64_t* candidates) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (ms) *ms = h->shor_last_ms;
  if (candidates) *candidates = h->shor_last_candidates;
  return 0;
}

int omc_shor_last_select_stats(omc_instance* h, int64_t out[4]) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "handle or out is NULL");
  for (int i = 0; i < 4; ++i) out[i] = h->shor_sel[i];
  return 0;
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

// ---------------------------------------------------------------------------------------------------------------------
// RCCL communicator behind the C ABI
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
int rccl_load() {
  if (g_rccl.lib) return 0;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* lib = nullptr;
  for (const char* nm : names) { lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
  if (!lib) return fail(OMC_ERR_COMM, std::string("librccl not loadable: ") + (dlerror() ? dlerror() : "?"));
  Rccl r; r.lib = lib;
  r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
  r.CommInitRank = (decltype(r.CommInitRank))dlsym(lib, "ncclCommInitRank");
  r.AllReduce = (decltype(r.AllReduce))dlsym(lib, "ncclAllReduce");
  r.Broadcast = (decltype(r.Broadcast))dlsym(lib, "ncclBroadcast");
  r.AllGather = (decltype(r.AllGather))dlsym(lib, "ncclAllGather");
  r.CommDestroy = (decltype(r.CommDestroy))dlsym(lib, "ncclCommDestroy");
  r.GetErrorString = (decltype(r.GetErrorString))dlsym(lib, "ncclGetErrorString");
  if (!r.GetUniqueId || !r.CommInitRank || !r.AllReduce || !r.Broadcast || !r.AllGather || !r.CommDestroy) return fail(OMC_ERR_COMM, "librccl lacks an expected symbol");
  g_rccl = r;
  return 0;
}
int rccl_fail(ncclResult_t e, const char* what) {
  return fail(OMC_ERR_COMM, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "RCCL error"));
}
}  // namespace

int omc_comm_unique_id(void* id_out) {
  if (!id_out) return fail(OMC_ERR_ARGUMENT, "id_out is NULL");
  int rc = rccl_load(); if (rc) return rc;
  ncclUniqueId id;
  ncclResult_t e = g_rccl.GetUniqueId(&id);
  if (e != ncclSuccess) return rccl_fail(e, "ncclGetUniqueId");
  static_assert(sizeof(ncclUniqueId) == OMC_COMM_ID_BYTES, "unique id size");
  memcpy(id_out, &id, sizeof(id));
  return 0;
}

int omc_comm_init(omc_instance* h, int rank, int world_size, const void* id) {
  if (!h || !id) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (world_size < 1 || rank < 0 || rank >= world_size) return fail(OMC_ERR_ARGUMENT, "rank / world_size out of range");
  if (h->comm) return fail(OMC_ERR_ARGUMENT, "communicator already initialised");
  int rc = rccl_load(); if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  ncclUniqueId uid; memcpy(&uid, id, sizeof(uid));
  ncclComm_t c = nullptr;
  ncclResult_t e = g_rccl.CommInitRank(&c, world_size, uid, rank);
  if (e != ncclSuccess) return rccl_fail(e, "ncclCommInitRank");
  h->comm = (void*)c; h->comm_rank = rank; h->comm_world = world_size;
  if ((rc = h->bcomm.ensure(64))) return rc;
  return 0;
}

int omc_allreduce_bounds(omc_instance* h, double* ub, double* lb, int* owner) {
  if (!h || !ub || !lb) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (!h->comm) return fail(OMC_ERR_COMM, "omc_comm_init has not been called on this handle");
  HIPCHK(hipSetDevice(h->device));
  double* d = h->bcomm.as<double>();
  const double mine = *ub;
  double v[2] = {*ub, *lb};
  HIPCHK(hipMemcpyAsync(d, v, 16, hipMemcpyHostToDevice, h->stream));
  ncclResult_t e = g_rccl.AllReduce(d, d, 2, ncclDouble, ncclMin, (ncclComm_t)h->comm, h->stream);
  if (e != ncclSuccess) return rccl_fail(e, "ncclAllReduce(min, fp64[2])");
  HIPCHK(hipMemcpyAsync(v, d, 16, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *ub = v[0]; *lb = v[1];
  if (owner) {   // second 8-byte MIN: the smallest rank that holds the minimum (ties are common: every rank starts from the same root bound)
    double r = (mine == v[0]) ? (double)h->comm_rank : (double)h->comm_world;
    HIPCHK(hipMemcpyAsync(d + 2, &r, 8, hipMemcpyHostToDevice, h->stream));
    e = g_rccl.AllReduce(d + 2, d + 2, 1, ncclDouble, ncclMin, (ncclComm_t)h->comm, h->stream);
    if (e != ncclSuccess) return rccl_fail(e, "ncclAllReduce(min, owner)");
    HIPCHK(hipMemcpyAsync(&r, d + 2, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *owner = (int)r;
  }
  return 0;
}

int omc_bcast_incumbent(omc_instance* h, int root, double* X) {
  if (!h || !X) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (!h->comm) return fail(OMC_ERR_COMM, "omc_comm_init has not been called on this handle");
  if (root < 0 || root >= h->comm_world) return fail(OMC_ERR_ARGUMENT, "root out of range");
  HIPCHK(hipSetDevice(h->device));
  const size_t cnt = (size_t)h->n * h->m;
  int rc = h->bXin.ensure(8 * cnt + 64); if (rc) return rc;
  double* d = h->bXin.as<double>();
  if (h->comm_rank == root) HIPCHK(hipMemcpyAsync(d, X, 8 * cnt, hipMemcpyHostToDevice, h->stream));
  ncclResult_t e = g_rccl.Broadcast(d, d, cnt, ncclDouble, root, (ncclComm_t)h->comm, h->stream);
  if (e != ncclSuccess) return rccl_fail(e, "ncclBroadcast(X)");
  if (h->comm_rank != root) HIPCHK(hipMemcpyAsync(X, d, 8 * cnt, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// The per-node records every rank needs to grow the same tree (the serial loop OMC.jl:700-719 sees every relaxed node: status, objective,
// bound, eigenvalues, breakpoint vector, U -- 8 (6 + n + n k) bytes per node, never X or Y): all-gather of `cnt` rows of `width` doubles per rank.
// Ranks may hold different counts: the counts are gathered first (8 bytes per rank), the rows are padded to the largest count, and
// `out` receives the rows of rank 0, then rank 1, ... (sum of counts x width doubles; capacity = world x max_cnt_capacity rows).
int omc_allgather_records(omc_instance* h, const double* rows, int cnt, int width, double* out, int out_capacity_rows, int* counts /* world */) {
  if (!h || !out || !counts || (cnt > 0 && !rows)) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (cnt < 0 || width <= 0) return fail(OMC_ERR_ARGUMENT, "cnt / width out of range");
  if (!h->comm) return fail(OMC_ERR_COMM, "omc_comm_init has not been called on this handle");
  HIPCHK(hipSetDevice(h->device));
  const int W = h->comm_world;
  int rc = h->bcomm.ensure(64 + 8 * (size_t)W); if (rc) return rc;
  double* d = h->bcomm.as<double>();
  const double mine = (double)cnt;
  HIPCHK(hipMemcpyAsync(d + 4, &mine, 8, hipMemcpyHostToDevice, h->stream));
  ncclResult_t e = g_rccl.AllGather(d + 4, d + 8, 1, ncclDouble, (ncclComm_t)h->comm, h->stream);
  if (e != ncclSuccess) return rccl_fail(e, "ncclAllGather(counts)");
  std::vector<double> hc(W);
  HIPCHK(hipMemcpyAsync(hc.data(), d + 8, 8 * (size_t)W, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int cmax = 0; long tot = 0;
  for (int r = 0; r < W; ++r) { counts[r] = (int)hc[r]; cmax = std::max(cmax, counts[r]); tot += counts[r]; }
  if (tot > out_capacity_rows) return fail(OMC_ERR_ARGUMENT, "omc_allgather_records: out is too small for the gathered rows");
  if (cmax == 0) return 0;
  const size_t blk = (size_t)cmax * width;
  if ((rc = h->bXin.ensure(8 * blk * (size_t)(W + 1) + 64))) return rc;
  double* send = h->bXin.as<double>(); double* recv = send + blk;
  HIPCHK(hipMemsetAsync(send, 0, 8 * blk, h->stream));
  if (cnt) HIPCHK(hipMemcpyAsync(send, rows, 8 * (size_t)cnt * width, hipMemcpyHostToDevice, h->stream));
  e = g_rccl.AllGather(send, recv, blk, ncclDouble, (ncclComm_t)h->comm, h->stream);
  if (e != ncclSuccess) return rccl_fail(e, "ncclAllGather(records)");
  size_t o = 0;
  for (int r = 0; r < W; ++r) {
    if (counts[r]) HIPCHK(hipMemcpyAsync(out + o, recv + (size_t)r * blk, 8 * (size_t)counts[r] * width, hipMemcpyDeviceToHost, h->stream));
    o += (size_t)counts[r] * width;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int omc_comm_destroy(omc_instance* h) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy((ncclComm_t)h->comm);
  h->comm = nullptr; h->comm_rank = 0; h->comm_world = 1;
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

}  // extern "C"
