// omc_api_branch.cpp -- children of finished nodes by reference (include/omc.h "children by reference"): omc_branch_plan,
// omc_relax_append_children and the branch half of the one append path (append_nodes, omc_api.cpp), omc_relax_fetch_descriptor.
//
// Mirrors create_matrix_cut_child_nodes of the reference driver (OMC.jl:2520-2542): a child is its parent's cut list plus
// (breakpoint_vec, U_relax, directions).  Both vectors are on the device when the parent is harvested (OmcWS::obx, oU), so the child's
// descriptor is built there (omc_branch.hip) from the parent's; the host keeps three counts per node and decides every refusal from them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "omc_api_internal.h"

static int dir_codes(int cut_type, int codes[4]) {      // in the order of OMC.jl:2481-2491 (bnb.DIRECTIONS_OF)
  if (cut_type == OMC_CUT_LINEAR) { codes[0] = OMC_DIR_LEFT; codes[1] = OMC_DIR_RIGHT; return 2; }
  if (cut_type == OMC_CUT_LINEAR2) { codes[0] = OMC_DIR_LEFT; codes[1] = OMC_DIR_MIDDLE; codes[2] = OMC_DIR_RIGHT; return 3; }
  if (cut_type == OMC_CUT_LINEAR3) { codes[0] = OMC_DIR_LEFT; codes[1] = OMC_DIR_INNER_LEFT; codes[2] = OMC_DIR_INNER_RIGHT; codes[3] = OMC_DIR_RIGHT; return 4; }
  return 0;
}

int omc_branch_plan(int cut_type, int k, int capacity, int8_t* dirs, int* n_children) {
  if (!dirs || !n_children) return fail(OMC_ERR_ARGUMENT, "omc_branch_plan: NULL argument");
  { int rcc = check_cut_type(cut_type); if (rcc) return rcc; }
  if (k < 1 || k > 8) return fail(OMC_ERR_ARGUMENT, "omc_branch_plan: rank k must satisfy 1 <= k <= 8");
  int codes[4];
  const int nd = dir_codes(cut_type, codes);
  long long total = 1;
  for (int j = 0; j < k; ++j) total *= nd;
  *n_children = (int)total;
  if (capacity < total) return fail(OMC_ERR_ARGUMENT, "omc_branch_plan: capacity below the number of children (" + std::to_string(total) + ")");
  for (long long c = 0; c < total; ++c) {      // the first column varies fastest (Iterators.product)
    long long q = c;
    for (int j = 0; j < k; ++j) { dirs[c * k + j] = (int8_t)codes[q % nd]; q /= nd; }
  }
  return 0;
}

int branch_check(omc_instance* h, int first, int C, const BranchRefs& refs, const std::string& pre) {
  const OmcWS& w = h->ws;
  const int n = h->n, k = h->k;
  if (!h->br_ready || h->node_L.size() < (size_t)first + (size_t)C) return fail(OMC_ERR_ARGUMENT, pre + "the batch was staged without room for appended nodes (omc_relax_reserve)");
  if (n > BRANCH_NMAX) return fail(OMC_ERR_UNSUPPORTED, pre + "n above " + std::to_string(BRANCH_NMAX) + " is not supported by the branch kernels");
  for (int c = 0; c < C; ++c) {
    const int p = refs.parent_id[c];
    if (p < 0 || p >= first) return fail(OMC_ERR_ARGUMENT, pre + "parent " + std::to_string(p) + " is not a node of the batch");
    for (int j = 0; j < k; ++j) {
      double lo, hi, sl, ic;
      if (cut_piece(h->staged_cut_type, refs.dirs[(size_t)c * k + j], 0.0, h->params.reference_quirk_q1, &lo, &hi, &sl, &ic))
        return fail(OMC_ERR_INVALID_ENUM, pre + "direction code invalid for the staged cut type (OMC.jl:1580-1678)");
    }
    const std::string of = " of node " + std::to_string(p) + " ";
    if (h->node_L[p] + 1 > w.Lmax) return fail(OMC_ERR_ARGUMENT, pre + "a child" + of + "has more cuts than omc_relax_reserve allowed for (" + std::to_string(w.Lmax) + ")");
    if (h->node_R[p] + 2 * k + 1 > w.Rmax) return fail(OMC_ERR_ARGUMENT, pre + "a child" + of + "has more rows than the staged stride (" + std::to_string(w.Rmax) + ")");
    if (std::min(n, h->node_r[p] + 1) > w.rmax) return fail(OMC_ERR_ARGUMENT, pre + "a child" + of + "may have more row-subspace columns than the staged stride (" + std::to_string(w.rmax) + ")");
  }
  return 0;
}

int branch_write(omc_instance* h, int first, int C, const BranchRefs& refs, hipStream_t s) {
  const OmcWS& w = h->ws;
  const size_t k = (size_t)h->k;
  BranchWS scratch{};
  { Carve c(h->bbrS.p); walk_branch_scratch(c, BRANCH_CHUNK, (size_t)h->n, k, scratch); }
  std::vector<char> img;
  std::unordered_map<int, int> slot_of;
  for (int c0 = 0; c0 < C; c0 += BRANCH_CHUNK) {
    const int cn = std::min(C - c0, BRANCH_CHUNK);
    slot_of.clear();
    std::vector<int> parents;
    for (int c = 0; c < cn; ++c) if (slot_of.emplace(refs.parent_id[c0 + c], (int)parents.size()).second) parents.push_back(refs.parent_id[c0 + c]);
    const size_t ns = parents.size();
    // the chunk's index image, host and device laid out by the same walk at the chunk's own counts
    BranchWS hb = scratch, db = scratch;
    Carve measure; walk_branch_ints(measure, ns, (size_t)cn, k, hb);
    img.assign(measure.bytes(), 0);
    { Carve hc(img.data()); walk_branch_ints(hc, ns, (size_t)cn, k, hb); }
    { Carve dc(h->bbrI.p); walk_branch_ints(dc, ns, (size_t)cn, k, db); }
    for (size_t p = 0; p < ns; ++p) { hb.slot_node[p] = parents[p]; hb.slot_L[p] = h->node_L[parents[p]]; }
    for (int c = 0; c < cn; ++c) hb.child_slot[c] = slot_of[refs.parent_id[c0 + c]];
    memcpy(hb.dirs, refs.dirs + (size_t)c0 * k, (size_t)cn * k);
    db.cut_type = h->staged_cut_type; db.q1 = h->params.reference_quirk_q1;
    HIPCHK(hipMemcpyAsync(h->bbrI.p, img.data(), img.size(), hipMemcpyHostToDevice, s));
    omc_launch_branch(&w, &db, (int)ns, first + c0, cn, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));      // the image and the scratch serve the next chunk
  }
  return 0;
}

void branch_commit(omc_instance* h, int first, int C, const BranchRefs& refs) {
  for (int c = 0; c < C; ++c) {
    const int p = refs.parent_id[c];
    h->node_L[first + c] = h->node_L[p] + 1; h->node_R[first + c] = h->node_R[p] + 2 * h->k + 1; h->node_r[first + c] = std::min(h->n, h->node_r[p] + 1);
  }
  *refs.first_out = first;
}

int omc_relax_append_children(omc_instance* h, int C, const int* parent_id, const int8_t* dirs, const int* load_from, const int* save_to,
                              int* first_child_id) {
  if (!h || !h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_append_children: nothing staged");
  if (C <= 0) return fail(OMC_ERR_ARGUMENT, "omc_relax_append_children: C must be positive");
  if (!parent_id || !dirs || !first_child_id) return fail(OMC_ERR_ARGUMENT, "omc_relax_append_children: parent_id, dirs or first_child_id is NULL");
  if (h->shor_on) return fail(OMC_ERR_UNSUPPORTED, "omc_relax_append_children: the staged batch is in Shor mode (a child would inherit its parent's list: omc_relax_append_shor)");
  // before append_nodes takes the lock (this check takes it itself); a node that has finished stays finished
  { int rcf = require_finished_ids(h, C, parent_id, false, "omc_relax_append_children"); if (rcf) return rcf; }
  const BranchRefs refs = {parent_id, dirs, first_child_id};
  return append_nodes(h, "omc_relax_append_children", C, nullptr, nullptr, nullptr, nullptr, load_from, save_to, nullptr, &refs);
}

int omc_relax_fetch_descriptor(omc_instance* h, int node_id, int* R, int* rkind, int* rcut, int* rbi, int* rbj, double* rcoef, double* rrhs,
                               int* L, double* cutx, int* r, double* Q) {
  if (!h || !h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_descriptor: nothing staged");
  if (node_id < 0 || node_id >= h->Btot_live.load() || (size_t)node_id >= h->node_L.size())
    return fail(OMC_ERR_ARGUMENT, "omc_relax_fetch_descriptor: node " + std::to_string(node_id) + " is not a node of the batch");
  HIPCHK(hipSetDevice(h->device));
  if (!h->fetch_stream) HIPCHK(hipStreamCreateWithFlags(&h->fetch_stream, hipStreamNonBlocking));
  hipStream_t fs = h->fetch_stream;
  const OmcWS& w = h->ws;
  const size_t b = (size_t)node_id, n = w.n, k = w.k, Rm = w.Rmax, Lm = w.Lmax, rm = w.rmax;
  if (R) HIPCHK(hipMemcpyAsync(R, w.R + b, sizeof(int), hipMemcpyDeviceToHost, fs));
  if (rkind) HIPCHK(hipMemcpyAsync(rkind, w.rkind + b * Rm, sizeof(int) * Rm, hipMemcpyDeviceToHost, fs));
  if (rcut) HIPCHK(hipMemcpyAsync(rcut, w.rcut + b * Rm, sizeof(int) * Rm, hipMemcpyDeviceToHost, fs));
  if (rbi) HIPCHK(hipMemcpyAsync(rbi, w.rbi + b * Rm, sizeof(int) * Rm, hipMemcpyDeviceToHost, fs));
  if (rbj) HIPCHK(hipMemcpyAsync(rbj, w.rbj + b * Rm, sizeof(int) * Rm, hipMemcpyDeviceToHost, fs));
  if (rcoef) HIPCHK(hipMemcpyAsync(rcoef, w.rcoef + b * Rm * k, 8 * Rm * k, hipMemcpyDeviceToHost, fs));
  if (rrhs) HIPCHK(hipMemcpyAsync(rrhs, w.rrhs + b * Rm, 8 * Rm, hipMemcpyDeviceToHost, fs));
  if (cutx) HIPCHK(hipMemcpyAsync(cutx, w.cutx + b * Lm * n, 8 * Lm * n, hipMemcpyDeviceToHost, fs));
  if (r) HIPCHK(hipMemcpyAsync(r, w.rr + b, sizeof(int), hipMemcpyDeviceToHost, fs));
  if (Q) HIPCHK(hipMemcpyAsync(Q, w.Qb + b * n * rm, 8 * n * rm, hipMemcpyDeviceToHost, fs));
  HIPCHK(hipStreamSynchronize(fs));
  if (L) *L = h->node_L[b];
  return 0;
}
