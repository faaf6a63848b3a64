// omc_walks.h -- the packed device buffers of the host API, each as one walk over a Carve (omc_carve.h): every array is one take with its
// width written out, in the order the buffer holds them.  A walk run over a measuring Carve gives the bytes to allocate, the same walk over
// the allocation fills the pointers (carve_ensure, omc_host.h), so nothing else states a size or an offset.  Where code outside a walk
// relies on two arrays being adjacent (one copy or one memset over both), the walk says so, and that code takes its length from the
// pointers the walk handed out.  No HIP call: the structs are filled on the host by any compiler (tests/host/carve_check.cpp).
#pragma once
#include "omc_carve.h"
#include "omc_device.h"
#include "omc_branch.h"
#include "omc_shor_relax.h"
#include "omc_shor_cert.h"
#include "omc_shor_index.h"

// ---- omc_relax_stage: S slots (state), N nodes of the capacity (descriptors and outputs) ------------------------------------------------------
struct StageDims { size_t S, N, n, m, k, nnz, rmax, Rmax; };

inline void walk_gap(Carve& c, const StageDims& d, OmcWS& w) {
  w.gap_prev = c.take<double>(d.S); w.gap_rate = c.take<double>(d.S);
}
inline void walk_small_cone(Carve& c, const StageDims& d, OmcWS& w) {      // bsm
  const size_t vk = d.S * d.rmax * d.k, tk = d.S * d.k * d.k;
  w.Vt = c.take<double>(vk); w.D3V = c.take<double>(vk); w.W3V = c.take<double>(vk); w.Q3V = c.take<double>(vk);
  w.D3T = c.take<double>(tk); w.W3T = c.take<double>(tk); w.Q3T = c.take<double>(tk);
}
inline void walk_objcol(Carve& c, const StageDims& d, OmcWS& w) {
  w.objcol = c.take<double>(d.S * d.m); w.c0col = c.take<double>(d.S * d.m);
}
// bchk.  stamps sits behind chk_scratch and runs to the end of the buffer: omc_relax_stage zeroes it from there to the end of the walk
inline void walk_check(Carve& c, const StageDims& d, OmcWS& w) {
  w.chk_scratch = c.take<double>(d.S * d.n * d.k);
  w.stamps = c.take<double>(32 + 8 * d.S);      // 32 stamps, then 8 diagnostic doubles per slot (omc_debug_diag)
}
inline void walk_scalars(Carve& c, const StageDims& d, OmcWS& w) {      // bscal
  const size_t S = d.S;
  w.obj = c.take<double>(S); w.objout = c.take<double>(S); w.lb = c.take<double>(S); w.c0 = c.take<double>(S); w.evsum = c.take<double>(S);
  w.cpen = c.take<double>(S); w.cst = c.take<double>(S); w.rp = c.take<double>(S); w.rd = c.take<double>(S);
  w.lmin = c.take<double>(2 * S);
  w.objprev = c.take<double>(S); w.lbprev = c.take<double>(S); w.fro2 = c.take<double>(S); w.bfac = c.take<double>(S);
  (void)c.take<double>(S);      // a sixteenth slot that nothing addresses: keeps the allocation size it had before the walks
}
// bint.  ws_need is the word directly behind done[S]: the solve loop brings both back with one copy of S + 1 ints from done
// (omc_relax_solve.cpp, the copy of the done flags at a check)
inline void walk_slot_ints(Carve& c, const StageDims& d, OmcWS& w) {
  const size_t S = d.S;
  w.rowov = c.take<int>(S); w.status = c.take<int>(S); w.iters = c.take<int>(S); w.sweeps = c.take<int>(S); w.stall = c.take<int>(S);
  w.vvalid = c.take<int>(S); w.nbump = c.take<int>(S); w.lastbump = c.take<int>(S);
  w.done = c.take<int>(S); w.ws_need = c.take<int>(1);
  (void)c.take<int>(S - 1);      // one word is used; the rest of a tenth slot keeps the allocation size it had before the walks
}
// bslotint.  omc_relax_stage uploads node_of, init and fin as one host image laid out by this same walk
inline void walk_slot_map(Carve& c, const StageDims& d, int*& node_of, int*& init, int*& fin) {
  node_of = c.take<int>(d.S); init = c.take<int>(d.S); fin = c.take<int>(d.S);
}
inline void walk_sub_doubles(Carve& c, const StageDims& d, OmcWS& w) {      // bsubS
  w.sub_theta = c.take<double>(16 * d.S); w.trM = c.take<double>(d.S); w.V3 = c.take<double>(256 * d.S);
}
inline void walk_sub_ints(Carve& c, const StageDims& d, OmcWS& w) {      // bsubI (w1_fac: omc_relax_stage drops the pointer where the factored W1 is off)
  const size_t S = d.S;
  w.sub_on = c.take<int>(S); w.cone_done = c.take<int>(S); w.sub_stat = c.take<int>(8 * S); w.sub_wait = c.take<int>(S); w.sub_nfail = c.take<int>(S);
  w.v3valid = c.take<int>(S); w.ws_first = c.take<int>(S); w.w1_fac = c.take<int>(S);
}
inline void walk_subC_doubles(Carve& c, const StageDims& d, OmcWS& w) {      // bsubSC
  w.sub_thetaC = c.take<double>(16 * d.S); w.trMc = c.take<double>(d.S); w.lb_est = c.take<double>(d.S);
}
inline void walk_subC_ints(Carve& c, const StageDims& d, OmcWS& w) {      // bsubIC (sep_done: dropped by omc_relax_stage without the tracked subspace)
  w.sub_onC = c.take<int>(d.S); w.confirm = c.take<int>(d.S); w.sep_done = c.take<int>(d.S);
}
inline void walk_aa_ints(Carve& c, const StageDims& d, OmcWS& w) {      // baaI: zeroed as a whole
  const size_t S = d.S;
  w.aa_hist = c.take<int>(S); w.aa_head = c.take<int>(S); w.aa_pending = c.take<int>(S); w.aa_valid = c.take<int>(S);
  w.aa_nacc = c.take<int>(S); w.aa_nrej = c.take<int>(S);
}
inline void walk_out_scalars(Carve& c, const StageDims& d, OmcWS& w) {      // boscal
  w.oobj = c.take<double>(d.N); w.olb = c.take<double>(d.N); w.olmin = c.take<double>(2 * d.N); w.orho = c.take<double>(d.N);
}
inline void walk_out_ints(Carve& c, const StageDims& d, OmcWS& w) {
  w.ostatus = c.take<int>(d.N); w.oiters = c.take<int>(d.N);
}
// best certificate per slot (bcbD, bcbI) and per node (bocD); cnnz = 0 in Shor mode, which keeps no Lam (the caller drops the pointer)
inline void walk_cert_slot(Carve& c, const StageDims& d, size_t cnnz, OmcWS& w) {
  const size_t ps = (d.rmax + d.k) * (d.rmax + d.k);
  w.cb_rho = c.take<double>(d.S); w.cbBound = c.take<double>(d.S);
  w.cbLam = c.take<double>(d.S * cnnz); w.cblam = c.take<double>(d.S * d.Rmax); w.cbPsi = c.take<double>(d.S * ps);
}
inline void walk_cert_flags(Carve& c, const StageDims& d, OmcWS& w) {
  w.cert_flag = c.take<int>(d.S); w.cert_have = c.take<int>(d.S);
}
inline void walk_cert_node(Carve& c, const StageDims& d, size_t cnnz, OmcWS& w) {
  const size_t ps = (d.rmax + d.k) * (d.rmax + d.k);
  w.ocBound = c.take<double>(d.N);
  w.ocLam = c.take<double>(d.N * cnnz); w.oclam = c.take<double>(d.N * d.Rmax); w.ocPsi = c.take<double>(d.N * ps);
}

// omc_relax_append_children (omc_branch.h): bbrS, the scratch of `slots` distinct parents; bbrI, the index image of one chunk -- the host
// fills an image laid out by this same walk and uploads it with one copy from slot_node to the walk's end
inline void walk_branch_scratch(Carve& c, size_t slots, size_t n, size_t k, BranchWS& b) {
  b.vhat = c.take<double>(slots * k); b.q = c.take<double>(slots * n); b.keep = c.take<int>(slots);
}
inline void walk_branch_ints(Carve& c, size_t slots, size_t children, size_t k, BranchWS& b) {
  b.slot_node = c.take<int>(slots); b.slot_L = c.take<int>(slots); b.child_slot = c.take<int>(children); b.dirs = c.take<int8_t>(children * k);
}

// ---- omc_relax_stage_shor ----------------------------------------------------------------------------------------------------------------
// sfroB.  trB sits directly behind fro2B; the kernels write both through their own pointers and no copy or memset spans the two
inline void walk_shor_fro(Carve& c, size_t S, ShWS& sh) {
  sh.fro2B = c.take<double>(S); sh.trB = c.take<double>(S);
}
// Shor part of the best certificate, per slot (scbD, count = S) and per node (socD, count = N): blocks, paraboloid multipliers and points
inline void walk_shor_cert(Carve& c, size_t count, size_t nq1, size_t m, size_t nm, double*& Gam, double*& Zeta, double*& Xi, double*& Xbar) {
  Gam = c.take<double>(count * 15 * nq1); Zeta = c.take<double>(count * m); Xi = c.take<double>(count * nm); Xbar = c.take<double>(count * nm);
}
inline void walk_shor_sub_ints(Carve& c, size_t S, ShWS& sh, OmcWS& wb) {      // ssubIB: zeroed as a whole
  sh.sub_onB = c.take<int>(S); sh.cone_doneB = c.take<int>(S); sh.sub_waitB = c.take<int>(S); sh.sub_nfailB = c.take<int>(S);
  wb.sub_stat = c.take<int>(8 * S);
}

// ---- the private eigen-kernel view of the dual-bound evaluators: V views (nodes, or nodes x ways), k = 1 in Shor mode ---------------------------
struct EvalDims { size_t V, n, k, nnz, Rmax, rmax, Lmax; };
// what the evaluators keep beside the view: their multipliers on the device, and the ends of the two spans they address as one
struct EvalArrays {
  double *Lam, *lam, *Psi, *T1;
  double* scalars_end;      // c0, cpen, cst, fro2c, evsum are read back with one copy from c0 to here
  int* zero_end;            // done, vvalidC, sweeps, mw_stat are zeroed with one memset from done to here
};
// matrices: 32-byte rows for the multi-workgroup kernels (np16 * np16 and nn4 are multiples of 4 doubles).  MbufC and VrowC are zeroed with
// one memset from MbufC to Mchk.  slab = 0: the view's slab, if any, is a buffer of its own
inline void walk_eval_matrices(Carve& c, const EvalDims& d, size_t slab, OmcWS& w) {
  const size_t NP = (d.n + 15) & ~(size_t)15, nn4 = (d.n * d.n + 3) & ~(size_t)3;
  w.MbufC = c.take<double>(d.V * NP * NP, 32); w.VrowC = c.take<double>(d.V * NP * NP); w.Mchk = c.take<double>(d.V * nn4);
  if (slab) w.cone_scratch = c.take<double>(d.V * slab);
}
inline void walk_eval_doubles(Carve& c, const EvalDims& d, bool with_Lam, OmcWS& w, EvalArrays& a) {
  const size_t V = d.V, ps = (d.rmax + d.k) * (d.rmax + d.k);
  w.rcoef = c.take<double>(V * d.Rmax * d.k); w.rrhs = c.take<double>(V * d.Rmax); w.cutx = c.take<double>(V * d.Lmax * d.n); w.Qb = c.take<double>(V * d.n * d.rmax);
  a.Lam = with_Lam ? c.take<double>(V * d.nnz) : nullptr;
  a.lam = c.take<double>(V * d.Rmax); a.Psi = c.take<double>(V * ps); a.T1 = c.take<double>(V * d.n * d.rmax);
  w.chk_scratch = c.take<double>(V * d.n * d.k);
  w.c0 = c.take<double>(V); w.cpen = c.take<double>(V); w.cst = c.take<double>(V); w.fro2c = c.take<double>(V); w.evsum = c.take<double>(V);
  a.scalars_end = c.take<double>(0);
}
inline void walk_eval_ints(Carve& c, const EvalDims& d, OmcWS& w, EvalArrays& a) {
  const size_t V = d.V;
  w.R = c.take<int>(V); w.rr = c.take<int>(V);
  w.rkind = c.take<int>(V * d.Rmax); w.rcut = c.take<int>(V * d.Rmax); w.rbi = c.take<int>(V * d.Rmax); w.rbj = c.take<int>(V * d.Rmax);
  w.done = c.take<int>(V); w.vvalidC = c.take<int>(V); w.sweeps = c.take<int>(V); w.mw_stat = c.take<int>(4 * V);
  a.zero_end = c.take<int>(0);
}
// omc_dual_bound_batch: dbM, dbD, dbI
inline void walk_dual_matrices(Carve& c, const EvalDims& d, OmcWS& w) { walk_eval_matrices(c, d, 0, w); }
inline void walk_dual_doubles(Carve& c, const EvalDims& d, OmcWS& w, EvalArrays& a) { walk_eval_doubles(c, d, true, w, a); }
inline void walk_dual_ints(Carve& c, const EvalDims& d, OmcWS& w, EvalArrays& a) { walk_eval_ints(c, d, w, a); }

// omc_shor_dual_bound_batch: B nodes with the caller's multipliers, V views of them; sdD holds every double, sdI every int
struct ScertDims { size_t B, nqs, nmb, nv1max, nv2max, m, slab; bool store_clean; };
struct ScertArrays { double *scale, *Gam, *zeta, *xi, *Xbar; int *node_group, *view_node, *view_way; };
inline void walk_scert_doubles(Carve& c, const ScertDims& s, const EvalDims& d, ShorCertWS& sc, ScertArrays& in, OmcWS& w, EvalArrays& a) {
  const size_t B = s.B, V = d.V, nm = d.n * s.m;
  sc.scale = in.scale = c.take<double>(B); sc.Gam = in.Gam = c.take<double>(B * 15 * s.nqs); sc.zeta = in.zeta = c.take<double>(B * s.m);
  sc.xi = in.xi = c.take<double>(B * nm); sc.Xbar = in.Xbar = c.take<double>(B * nm);
  sc.GamC = s.store_clean ? c.take<double>(B * 15 * s.nqs) : nullptr;
  sc.cleanpart = c.take<double>(B * s.nmb);
  sc.e1 = c.take<double>(V * s.nv1max); sc.e2 = c.take<double>(V * s.nv2max); sc.row8 = c.take<double>(V * 8 * s.nqs); sc.minpart = c.take<double>(V * s.nmb * 2);
  sc.lamDX = w.lamDX = c.take<double>(V * nm); sc.c0col = c.take<double>(V * s.m); sc.colmu = c.take<double>(V * s.m);
  walk_eval_matrices(c, d, s.slab, w);
  walk_eval_doubles(c, d, false, w, a);
}
inline void walk_scert_ints(Carve& c, const ScertDims& s, const EvalDims& d, ShorCertWS& sc, ScertArrays& in, OmcWS& w, EvalArrays& a) {
  sc.node_group = in.node_group = c.take<int>(s.B); sc.view_node = in.view_node = c.take<int>(d.V); sc.view_way = in.view_way = c.take<int>(d.V);
  sc.colbad = c.take<int>(d.V * s.m);
  walk_eval_ints(c, d, w, a);
}

// ---- omc_psd_project_batch: pjD, pjI -----------------------------------------------------------------------------------------------------
inline void walk_project_doubles(Carve& c, size_t B, size_t NP, OmcWS& w) {
  w.fro2 = c.take<double>(B); w.ev_out = c.take<double>(B * NP);
}
// uploaded and read back as one host image from done to ints_end
inline void walk_project_ints(Carve& c, size_t B, OmcWS& w, int*& ints_end) {
  w.done = c.take<int>(B); w.vvalid = c.take<int>(B); w.sweeps = c.take<int>(B); w.mw_stat = c.take<int>(4 * B);
  ints_end = c.take<int>(0);
}

// ---- index structures built on the device (omc_shor_index.h): sxD ---------------------------------------------------------------------------
// scratch for lists of up to nq minors (two key / member buffers of 4 nq items, tile x digit counts, head flags, block sums, the wire tuples
// and one chunk of soc_cap SOC pairs, the result word), then the staging room of the built lists: ints, and bytes in 16-byte units
struct ShorIndexDims { size_t nq = 0, soc_cap = 0, stage_ints = 0, stage_bytes = 0; };
inline void walk_shor_index(Carve& c, const ShorIndexDims& d, ShorIndexWS& w, int*& stage_int, uint8_t*& stage_byte) {
  const ShorIndexPlan P = shor_index_plan(2, 2, (long long)d.nq);
  w.keyA = c.take<unsigned long long>((size_t)P.items); w.keyB = c.take<unsigned long long>((size_t)P.items);
  w.idx = c.take<long long>(4 * d.nq); w.soc = c.take<long long>(2 * d.soc_cap);
  w.valA = c.take<unsigned>((size_t)P.items); w.valB = c.take<unsigned>((size_t)P.items);
  w.hist = c.take<unsigned>((size_t)P.hist); w.flag = c.take<unsigned>((size_t)P.flag); w.sums = c.take<unsigned>((size_t)P.sums);
  w.meta = c.take<int>(4);
  stage_int = c.take<int>(d.stage_ints); stage_byte = c.take<uint8_t>(d.stage_bytes, 16);
}
// one list in the staging room, every array at its capacity: 20 nq + nm + m + 3 ints.  mi, kid, cptr and cent are adjacent and as long as in
// the packed arena image, so one copy moves the four
inline void walk_shor_index_list(Carve& c, size_t nq, size_t nm, size_t m, ShorIndexWS& w) {
  w.mi = c.take<int>(4 * nq); w.kid = c.take<int>(4 * nq); w.cptr = c.take<int>(nm + 1); w.cent = c.take<int>(4 * nq);
  w.v1ptr = c.take<int>(2 * nq + 1); w.v1ent = c.take<int>(2 * nq); w.v2ptr = c.take<int>(2 * nq + 1); w.v2ent = c.take<int>(2 * nq);
  w.slackrow = c.take<int>(m);
}
