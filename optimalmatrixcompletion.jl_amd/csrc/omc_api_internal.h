// omc_api_internal.h -- what more than one of the omc_api*.cpp sources needs: declared here once, defined in exactly one of them (named at
// each group).  Private to the host side of libomc_hip.so; nothing here is exported.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "omc_cut_piece.h"
#include "omc_host.h"

#pragma GCC visibility push(hidden)

// ---- omc_api.cpp: staging ----------------------------------------------------------------------------------------------------------------
int upload(DevBuf& b, const void* src, size_t bytes, hipStream_t s);

// rows (OMC.jl:1558-1685) and row subspace of a set of nodes, on the host: shared by omc_relax_stage and omc_relax_append
struct NodePack {
  std::vector<std::vector<int>> rk, rc, rbi, rbj;
  std::vector<std::vector<double>> rcoef, rrhs, Qn;
  std::vector<int> rrv;
  int Rmax = 0, rmax = 1, Lmax = 0;
};
int pack_nodes(omc_instance* h, const omc_relax_params& P, int cut_type, int B, const int* L, const double* cut_x, const double* cut_Uhat,
               const int8_t* cut_dir, const double* U_lower, const double* U_upper, NodePack& pk);
int put_descriptors(const OmcWS& w, const NodePack& pk, int B, size_t rows, size_t first, const int* L, const double* cut_x, hipStream_t s);

// What the callers of the one staging routine ask of it beyond omc_relax_stage's arguments.  It travels with the call: nothing is left on
// the instance when a stage call returns early.
struct StageMode {
  bool shor = false;            // omc_relax_stage_shor: the base workspace of a Shor-mode batch
  bool warm_filtered = false;   // omc_relax_stage_shor: the warm-start indices have passed its filter
  int colprox_force = 0;        // omc_column_prox_batch: 1 = no block kernel, 2 = the block kernel for every non-empty column
};
int check_cut_type(int cut_type);
int stage_base(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L, const double* cut_x, const double* cut_Uhat,
               const int8_t* cut_dir, const double* U_lower, const double* U_upper, const StageMode& mode);

// ---- omc_api.cpp: objective cutoff ---------------------------------------------------------------------------------------------------------
void cutoff_solve_begin(omc_instance* h);      // a solve begins: its counters start at zero, its checks know whether a cutoff is set

// ---- omc_api.cpp: fetches -----------------------------------------------------------------------------------------------------------------
int require_finished_ids(omc_instance* h, int n_ids, const int* ids, bool upto_read_only, const char* who);
int require_certificates(const OmcWS& w, int n_ids, const int* ids, hipStream_t fs, const char* who);

// ---- omc_api_shor.cpp: Shor lists -----------------------------------------------------------------------------------------------------------
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
int shor_list_offsets(int B, const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx,
                      std::vector<size_t>& so, std::vector<size_t>& co);
using ShorListKey = omc_instance::ShorListKey;
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
int group_shor_lists(omc_instance* h, int B, const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx,
                     const ShorKnownLists* known, ShorGrouping& out);
struct ShorGroupImages { std::vector<int> hi; std::vector<uint8_t> hb; std::vector<ShorGroupDev> gd; };
int upload_shor_groups(omc_instance* h, const ShorGrouping& g, int* dev_int, uint8_t* dev_byte, ShorGroupDev* dev_groups, int* dev_node_group, hipStream_t s,
                       ShorGroupImages& img);

// the Shor half of the one append path (append_nodes, omc_api.cpp): the lists of the nodes of an omc_relax_append_shor call
struct ShorAppendLists { const int64_t *n_shor, *shor_idx, *n_soc, *soc_idx; };
int shor_append_plan(omc_instance* h, int first, int B2, const ShorAppendLists& l, std::vector<int>& load, std::vector<int>& save, ShorGrouping& g);
int shor_append_write(omc_instance* h, const ShorGrouping& g, int first, hipStream_t s, ShorGroupImages& img);
void shor_append_commit(omc_instance* h, ShorGrouping& g);
// the branch half of the one append path (omc_api_branch.cpp): the nodes of an omc_relax_append_children call are given by reference, child c =
// node parent_id[c] + one cut with the directions dirs[c * k ..]; *first_out receives the id of the first child
struct BranchRefs { const int* parent_id; const int8_t* dirs; int* first_out; };
int branch_check(omc_instance* h, int first, int C, const BranchRefs& refs, const std::string& pre);      // every refusal, from the host copies (node_L ...)
int branch_write(omc_instance* h, int first, int C, const BranchRefs& refs, hipStream_t s);               // the two kernels, chunk by chunk
void branch_commit(omc_instance* h, int first, int C, const BranchRefs& refs);                            // the children's host copies
// the one append path (omc_api.cpp): omc_relax_append, with `lists` omc_relax_append_shor, with `refs` omc_relax_append_children
int append_nodes(omc_instance* h, const char* who, int B2, const int* L, const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir,
                 const int* load_from, const int* save_to, const ShorAppendLists* lists, const BranchRefs* refs = nullptr);

#pragma GCC visibility pop

// two timing events that are destroyed on every exit path; create() != 0: the caller returns the code its call has always returned
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  hipError_t create() { hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
