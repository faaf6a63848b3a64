// omc_api_shor.cpp -- Shor mode of the relaxation behind the C ABI of include/omc.h: omc_set_shor_penalties, the grouping of a batch's
// (minor list, SOC list) pairs and their index structures on the host and on the device (omc_shor_index_plan / _build,
// omc_last_shor_index_stats), omc_relax_reserve_shor, omc_relax_stage_shor, omc_set_shor_keep_V, omc_relax_fetch_shor / _shor_V /
// _done_shor, omc_relax_batch_shor, omc_relax_append_shor and the Shor half of the append path, and the Shor extension of the state pool
// (omc_shor_warm_compat, omc_state_pool_reserve_shor / _fetch_shor, omc_last_shor_warm_stats, omc_last_shor_subspace_stats).
//
// Mirrors matrix_completion_SDP_relaxation with add_Shor_valid_inequalities = true (OMC.jl = the reference driver's
// src/OptimalMatrixCompletion.jl): OMC.jl:1503-1525, 1755-1779, 1838-1846; node.Shor_info lists OMC.jl:37-40.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>

#include "omc_api_internal.h"
#include <chrono>
#include <mutex>
#include <unordered_map>

#include "omc_shor_relax.h"
#include "omc_shor_index.h"

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
  double* entries = nullptr; long long* headers = nullptr;      // the staged workspace takes both from the instance's buffers (omc_relax_stage_shor)
  BIND(nb, entries, (size_t)h->pool_cap * L.stride);
  BIND(nh, headers, (size_t)h->pool_cap * 4, h->stream);
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


// ---- Shor mode (rank 1): matrix_completion_SDP_relaxation with add_Shor_valid_inequalities = true ---------------------------------------
// OMC.jl:1503-1525, 1755-1779, 1838-1846; node.Shor_info lists OMC.jl:37-40.  Formulation: oracle/omc_oracle_shor.py, DESIGN.md 3.7.
int omc_set_shor_penalties(omc_instance* h, double rho, double r4, double r5) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (!(rho > 0.0) || !(r4 >= 0.0) || !(r5 > 0.0)) return fail(OMC_ERR_ARGUMENT, "rho and r5 must be positive, r4 non-negative (0 = automatic)");
  h->shor_rho = rho; h->shor_r4 = r4; h->shor_r5 = r5;
  return 0;
}

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
int shor_list_offsets(int B, const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx,
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
// Groups the nodes (out.so / out.co: from shor_list_offsets) and builds the index structure of every new list.  With `known`, a new list
// that the batch has no room for is refused (messages of omc_relax_append_shor); nothing is written anywhere but `out`.
int group_shor_lists(omc_instance* h, int B, const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx,
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
int upload_shor_groups(omc_instance* h, const ShorGrouping& g, int* dev_int, uint8_t* dev_byte, ShorGroupDev* dev_groups, int* dev_node_group, hipStream_t s,
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
  const size_t int_cap = tot_int + (size_t)res_lists * shor_stage_ints((size_t)res_nq, (size_t)n * m, (size_t)m);
  const size_t byte_cap = tot_byte + (size_t)res_lists * shor_stage_bytes((size_t)n * m, (size_t)m);
  ShWS& sh = h->sh;
  memset(&sh, 0, sizeof(sh));
  // ---- upload the index structures: the two arenas, the group table and the nodes' group ids ------------------------------------------
  {
    int *arena_int = nullptr, *node_group_dev = nullptr; uint8_t* arena_byte = nullptr; ShorGroupDev* groups_dev = nullptr;
    BIND(h->sgInts, arena_int, int_cap); BIND(h->sgBytes, arena_byte, byte_cap);
    BIND(h->sgGroups, groups_dev, (size_t)NG + (size_t)res_lists); BIND(h->sgNodeGroup, node_group_dev, (size_t)h->node_cap);
    sh.groups = groups_dev; sh.node_group = node_group_dev;
    ShorGroupImages img;
    if ((rc = upload_shor_groups(h, grp, arena_int, arena_byte, groups_dev, node_group_dev, s, img))) return rc;
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
  const size_t sB = (size_t)S, sN = (size_t)h->node_cap, nm = (size_t)n * m;      // per-node outputs: room for the appended nodes too
  const int NPb = (N + 15) & ~15;
  const int nmb = std::max(1, (nqmax + 255) / 256);
  const size_t nq1 = (size_t)std::max(nqmax, 1), nv11 = (size_t)std::max(nv1max, 1), nv21 = (size_t)std::max(nv2max, 1);
  // one statement per array that owns its buffer: buffer, ShWS pointer, elements, and the stream where it starts zeroed
  BIND(h->sX, sh.X, sB * nm); BIND(h->sW, sh.W, sB * nm); BIND(h->sTh, sh.Th, sB * m * m);
  BIND(h->sV1, sh.V1, sB * nv11); BIND(h->sV2, sh.V2, sB * nv21); BIND(h->sV3, sh.V3, sB * nq1);
  BIND(h->sD0, sh.D0, sB * N * N); BIND(h->sP0, sh.P0, sB * N * N); BIND(h->sMbufB, sh.MbufB, sB * NPb * NPb, s); BIND(h->sVrowB, sh.VrowB, sB * NPb * NPb, s);
  BIND(h->sTq, sh.Tq, sB * 15 * nq1); BIND(h->sPq, sh.Pq, sB * 15 * nq1); BIND(h->sNq, sh.Nq, sB * 15 * nq1);
  BIND(h->sD5x, sh.D5x, sB * nm); BIND(h->sD5t, sh.D5t, sB * m); BIND(h->snu5, sh.nu5, sB * m); BIND(h->sP5x, sh.P5x, sB * nm);
  BIND(h->scolpart, sh.colpart, sB * m * 4); BIND(h->sminpart, sh.minpart, sB * nmb, s); BIND(h->sminpart2, sh.minpart2, sB * nmb, s);
  ENS_CARVE(h->sfroB, [&](Carve& c) { walk_shor_fro(c, sB, sh); }); BIND(h->svvB, sh.vvalidB, sB); BIND(h->se1, sh.e1, sB * nv11); BIND(h->se2, sh.e2, sB * nv21);
  BIND(h->soX, sh.oX, sN * nm, s); BIND(h->soW, sh.oW, sN * nm, s); BIND(h->soTh, sh.oTh, sN * m * m, s);
  sh.n = n; sh.m = m; sh.k = h->k; sh.N = N; sh.NPb = NPb; sh.S = S; sh.Btot = B; sh.nqmax = nqmax; sh.nv1max = nv1max; sh.nv2max = nv2max; sh.nmb = nmb;
  sh.rx = w.relax; sh.r4 = h->shor_r4; sh.r5 = h->shor_r5; sh.gamma = h->gamma; sh.sc = sc;
  sh.node_of = w.node_of; sh.done = w.done; sh.init = w.init; sh.fin = w.fin; sh.rho_b = w.rho_b; sh.bfac = w.bfac;
  sh.Ah = h->sAh.as<double>(); sh.mask = h->dmask.as<uint8_t>();
  sh.Y = w.Y; sh.Yp = w.Yp; sh.rp = w.rp; sh.rd = w.rd;
  sh.objcol = w.objcol; sh.c0col = w.c0col; sh.lamDX = w.lamDX;
  sh.oV = nullptr;
  if (w.load_from || w.save_to) {      // indices that passed the filter above: the Shor extension of the pool beside the base entries
    const ShorPoolLayout PL = shor_pool_layout(n, m, (int)h->pool_nqmax);
    sh.load_from = w.load_from; sh.save_to = w.save_to; sh.pscal = w.pscal; sh.pY = w.pY; sh.rho_node = w.rho_node;
    sh.pS = h->pShor.as<double>(); sh.pShdr = h->pShorHdr.as<long long>(); sh.pstride = PL.stride; sh.pnq = (int)h->pool_nqmax;
    BIND(h->sloadpart, sh.loadpart, sB * NPb * 2);
  }
  if (h->keep_shor_cert) {      // best certificate per node, Shor part: blocks, paraboloid multipliers and points, per slot and per node of the capacity; zeroed
    size_t cb_bytes = 0, oc_bytes = 0;
    if (carve_ensure(h->scbD, [&](Carve& c) { walk_shor_cert(c, sB, nq1, m, nm, sh.cbGam, sh.cbZeta, sh.cbXi, sh.cbXbar); }, &cb_bytes) ||
        carve_ensure(h->socD, [&](Carve& c) { walk_shor_cert(c, sN, nq1, m, nm, sh.ocGam, sh.ocZeta, sh.ocXi, sh.ocXbar); }, &oc_bytes) ||
        bind(h->socNq, sh.ocNq, sN)) {      // the three fail under one message; the zeroing below keeps a code of its own
      (void)hipGetLastError();
      return fail(OMC_ERR_ALLOC, "omc_relax_stage_shor: the Shor-mode certificates need " + std::to_string(cb_bytes / sB) + " bytes per slot (" + std::to_string(S) +
                                 ") and per node of the capacity (" + std::to_string(h->node_cap) + "), which the device does not have (" + g_err + ")");
    }
    HIPCHK(hipMemsetAsync(h->scbD.p, 0, cb_bytes, s)); HIPCHK(hipMemsetAsync(h->socD.p, 0, oc_bytes, s)); HIPCHK(hipMemsetAsync(sh.ocNq, 0, sN * sizeof(int), s));
    sh.cert_flag = w.cert_flag; sh.cb_rho = w.cb_rho;
  }
  if (h->shor_keep_V) BIND(h->soV, sh.oV, sN * 5 * nq1, s);
  // ---- base workspace in Shor mode, and the view through which its eigen-kernels project the order-(n+m) cone -------------------------
  w.shor = 1; w.shN = N; w.shP0 = sh.P0; w.shD0 = sh.D0; w.inv_s2 = 1.0 / (sc * sc);
  OmcWS& wb = h->wbig;
  wb = w;      // with the cutoff pointer stage_base has just set: the view carries whatever the base workspace does
  wb.n = N; wb.np16 = NPb; wb.Mbuf = sh.MbufB; wb.Vrow = sh.VrowB; wb.vvalid = sh.vvalidB; wb.fro2 = sh.fro2B; wb.W1 = sh.P0;
  wb.sub_enable = 0; wb.cert_enable = 0; wb.ws_mode = 0; wb.clip_hi = 1e300; wb.sub_debug = 0; wb.ws_first = nullptr; wb.ws_need = nullptr; wb.ws_phase = 0;
  // the view's own geometry (only the eigen-kernels are launched through it)
  wb.geo = omc_plan_geometry(N, NPb, wb.k, wb.rmax, wb.Rmax, h->cmax, h->tun.global_nolds, h->tun.cone_multi_min, MW_MAX_ORDER + 1);
  BIND(h->sbigmw, wb.mw_stat, sB * 4, s);
  if (wb.geo.ws.slab_stride) BIND(h->sbigscr, wb.cone_scratch, sB * wb.geo.ws.slab_stride);
  // the big cone's input has a handful of positive eigenvalues once the iterate has settled (measured: 2 - 5 of n + m): the tracked-subspace
  // kernel of the base engine follows them; the warm-started full kernel seeds the block and is the fall-back
  wb.trM = sh.trB;
  if (wb.geo.ws_lpp && N >= 48 && wb.geo.sub_lds <= OMC_MAX_DYN_LDS && !h->tun.no_subspace && !h->tun.shor_no_subspace) {
    size_t subI_bytes = 0;
    BIND(h->sXsB, wb.Xs, sB * NPb * 16, s); BIND(h->ssubSB, wb.sub_theta, sB * 16, s);
    ENS_CARVE(h->ssubIB, [&](Carve& c) { walk_shor_sub_ints(c, sB, sh, wb); }, &subI_bytes);
    HIPCHK(hipMemsetAsync(h->ssubIB.p, 0, subI_bytes, s));
    wb.sub_enable = 1;
    wb.sub_zscratch = nullptr;
    // bsubz again, larger, after stage_base bound it for w: the two uses are exclusive.  w has it when w.np16 > 512, that is n >= 513 and
    // N = n + m >= 1026; above order 1024 the warm-started kernel does not exist (geo.ws_lpp = 0), so this branch is not taken
    if (NPb > 512) BIND(h->bsubz, wb.sub_zscratch, sB * 16 * (size_t)(NPb + 2));
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
int shor_append_plan(omc_instance* h, int first, int B2, const ShorAppendLists& l, std::vector<int>& load, std::vector<int>& save, ShorGrouping& g) {
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
int shor_append_write(omc_instance* h, const ShorGrouping& g, int first, hipStream_t s, ShorGroupImages& img) {
  return upload_shor_groups(h, g, h->sgInts.as<int>() + h->sh_int_used, h->sgBytes.as<uint8_t>() + h->sh_byte_used,
                            h->sgGroups.as<ShorGroupDev>() + h->sh_lists.size(), h->sgNodeGroup.as<int>() + first, s, img);
}

void shor_append_commit(omc_instance* h, ShorGrouping& g) {
  for (size_t q = 0; q < g.lists.size(); ++q) {
    h->sh_byhash[g.hashes[q]].push_back((int)h->sh_lists.size());
    h->sh_lists.push_back(std::move(g.lists[q]));
  }
  h->sh_int_used += g.tot_int; h->sh_byte_used += g.tot_byte;
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
