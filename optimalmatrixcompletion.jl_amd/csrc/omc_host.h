// omc_host.h -- what the host sources of libomc_hip.so share (omc_api.cpp and the omc_api_*.cpp beside it, omc_relax_solve.cpp): the error
// string, the device and page-locked buffers, the tuning knobs, the instance behind the opaque handle of omc.h, and the per-kernel timing
// events.  Private.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "omc.h"
#include "omc_carve.h"
#include "omc_device.h"
#include "omc_shor_relax.h"
#include "omc_shor_index.h"
#include "omc_walks.h"

extern thread_local std::string g_err;      // omc_last_error of the calling thread (defined in omc_api.cpp)
static inline int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x)                                                                                         \
  do {                                                                                                    \
    hipError_t e_ = (x);                                                                                  \
    if (e_ != hipSuccess) {                                                                               \
      g_err = std::string(#x) + ": " + hipGetErrorString(e_);                                             \
      return (int)e_ > 0 ? (int)e_ : 999;                                                                 \
    }                                                                                                     \
  } while (0)

struct DevBuf {
  void* p = nullptr; size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) { g_err = std::string("hipMalloc: ") + hipGetErrorString(e); return (int)e; }
    cap = want;
    return 0;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() { return (T*)p; }
};
#define ENS(buf, bytes) do { int r_ = (buf).ensure(bytes); if (r_) return r_; } while (0)

// A packed buffer from one definition: `walk` (a callable over a Carve, omc_walks.h) is run once over a null base for the size, the buffer
// is made at least that large, and the same walk over the allocation hands out the pointers.  Returns ensure's code; *bytes: the walk's total.
template <class F> static inline int carve_ensure(DevBuf& b, F&& walk, size_t* bytes = nullptr) {
  Carve measure;
  walk(measure);
  if (bytes) *bytes = measure.bytes();
  const int rc = b.ensure(measure.bytes());
  if (rc) return rc;
  Carve place(b.p);
  walk(place);
  return 0;
}
#define ENS_CARVE(buf, ...) do { int r_ = carve_ensure(buf, __VA_ARGS__); if (r_) return r_; } while (0)

// A device array that owns its buffer, in one statement: `b` is made to hold `count` elements, `field` (the workspace's pointer to the
// array) is set, and with a stream exactly those count * sizeof(T) bytes are cleared on it.  Returns ensure's code, or HIPCHK's of the memset.
template <class T> static inline int bind(DevBuf& b, T*& field, size_t count) {
  field = nullptr;
  const int rc = b.ensure(count * sizeof(T));
  if (rc) return rc;
  field = (T*)b.p;
  return 0;
}
template <class T> static inline int bind(DevBuf& b, T*& field, size_t count, hipStream_t zero_on) {
  const int rc = bind(b, field, count);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(b.p, 0, count * sizeof(T), zero_on));
  return 0;
}
#define BIND(...) do { int r_ = bind(__VA_ARGS__); if (r_) return r_; } while (0)

// page-locked host memory: copies from and to it are asynchronous, so the host may go on while one is in flight
struct PinBuf {
  void* p = nullptr; size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) { g_err = std::string("hipHostMalloc: ") + hipGetErrorString(e); return (int)e; }
    cap = bytes;
    return 0;
  }
  template <class T> T* as() { return (T*)p; }
};

// Tuning knobs.  The environment is read in ONE place -- tuning_from_env, called by omc_instance_create and by omc_tuning_reload_env -- and a
// caller that does not want its environment to matter sets the knobs through omc_tuning_set; nothing else in the library calls getenv
// (behaviour of the shipped library depended on the caller's environment at every solve, one knob even per iteration).
// A flag is on when its variable is set to any value ("0" included); a number is atoi of the value when set, its default otherwise.
struct Tuning {
  bool altmin_nolds = false;       // OMC_ALTMIN_NOLDS: the altmin kernel on its global slab even where its LDS would do
  bool colprox_no_xcd = false;     // OMC_COLPROX_NO_XCD: no XCD-local placement of the column workgroups
  bool cone_512 = false;           // OMC_CONE_512: 512-thread form of the full eigen-kernel at large orders
  bool dense_proj = false;         // OMC_DENSE_PROJ: dense W1 and the Yp store instead of the factored projections
  bool host_phases = false;        // OMC_HOST_PHASES: every solve prints its host time between the iterations (omc_last_host_phases) to stderr when it ends
  bool global_nolds = false;       // OMC_GLOBAL_NOLDS: k_global's target in its L2-resident scratch instead of LDS
  bool no_colprox_pair = false;    // OMC_NO_COLPROX_PAIR: k_colprox for every column
  bool no_graph = false;           // OMC_NO_GRAPH: no hipGraph replay of the iteration body
  bool no_subspace = false;        // OMC_NO_SUBSPACE: no tracked subspace (k_cone_sub) for the cone block
  bool no_ws_split = false;        // OMC_NO_WS_SPLIT: the full eigen-kernel as one launch after k_cone_sub
  bool segv_trace = false;         // OMC_SEGV_TRACE: print the native frames of a crashing thread
  bool setup_gram_inline = false;  // OMC_SETUP_GRAM_INLINE: k_setup forms the rows' Gram matrix itself (one workgroup per slot) instead of k_setup_gram
  bool shor_explicit = false;      // OMC_SHOR_EXPLICIT: rank k > 1 Shor batches by the Shor engine even where the base engine would serve them
  bool shor_no_subspace = false;   // OMC_SHOR_NO_SUBSPACE: no tracked subspace for the order-(n+m) cone of Shor mode
  int check_xs = 16;               // OMC_CHECK_XS: cut vectors of the rows with a nonzero multiplier that k_check_build stages in LDS (the rest is read from global memory)
  int colprox_dpp = 1;             // OMC_COLPROX_DPP: k_colprox_pair's gather, sweep and solves by lane broadcast (DPP operands, no LDS); 0 = the staged body, the A/B arm with bit-identical results
  int colprox_block_min = 65;      // OMC_COLPROX_BLOCK_MIN: columns with at least this many observed rows take k_colprox_block (one workgroup per column, blocked MFMA Cholesky); a value above every column length is the path without it
  int cone_multi_min = 1025;       // OMC_CONE_MULTI_MIN: cone orders from this value on (never below 145) take the multi-workgroup eigen-kernels; the default is where only the cold kernel existed
  int event_merge = 1;             // OMC_EVENT_MERGE: 0 = every timed launch records two events of its own and the forks and joins of an iteration theirs (EventTape, omc_events.h)
  int graph_max = 16;              // OMC_GRAPH_MAX: hipGraph replay for batches staged with at most this many nodes
  int harvest_async = 1;           // OMC_HARVEST_ASYNC: 0 = every harvest is waited for, booked and refilled before the next iteration
  int harvest_async_min_live = 256;   // OMC_HARVEST_ASYNC_MIN_LIVE: live slots from which a harvest runs beside the next interval (omc_harvest_plan)
  int plain_multi_min = 1025;      // OMC_PLAIN_MULTI_MIN: cone orders from this value on (never below 145) run separation, rounding and the left singular vectors on the multi-workgroup eigen-kernels; the default is where only the cold kernel existed
  int shor_index_device_min = 0;   // OMC_SHOR_INDEX_DEVICE_MIN: Shor lists with at least this many minors get their index structure built on the device (omc_shor_index.hip); 0 = every list on the host
  int small_chain = 1;             // OMC_SMALL_CHAIN: 0 = k_small's projection runs the body it had before its chain was shortened (small_proj_chain), the A/B arm with bit-identical results
  int shor_select_kb = 1048576;    // OMC_SHOR_SELECT_KB: violated-minor selection streams (no materialised keys) when 16 B per candidate exceed this many KiB; 0 = always materialise
  int streams = 4;                 // OMC_STREAMS: <= 1 serialises a solve on one stream
  int sub_debug = 0;               // OMC_SUB_DEBUG: diagnostics of k_cone_sub (3: histograms for omc_debug_stamps)
  int sub_qmax = 24;               // OMC_SUB_QMAX: step budget of k_cone_sub
  int timing_stride = 1;           // OMC_TIMING_STRIDE: event timing of every s-th iteration, 0 = none
  int ws_quiet = 1;                // OMC_WS_QUIET: 0 = every iteration enqueues both phases of the full eigen-kernel, also in quiet intervals
};
struct Knob { const char* name; bool Tuning::*flag; int Tuning::*num; };
inline const Knob OMC_KNOBS[] = {
  {"OMC_ALTMIN_NOLDS", &Tuning::altmin_nolds, nullptr},      {"OMC_COLPROX_NO_XCD", &Tuning::colprox_no_xcd, nullptr},
  {"OMC_CONE_512", &Tuning::cone_512, nullptr},              {"OMC_DENSE_PROJ", &Tuning::dense_proj, nullptr},
  {"OMC_GLOBAL_NOLDS", &Tuning::global_nolds, nullptr},      {"OMC_HOST_PHASES", &Tuning::host_phases, nullptr},
  {"OMC_NO_COLPROX_PAIR", &Tuning::no_colprox_pair, nullptr},
  {"OMC_NO_GRAPH", &Tuning::no_graph, nullptr},              {"OMC_NO_SUBSPACE", &Tuning::no_subspace, nullptr},
  {"OMC_NO_WS_SPLIT", &Tuning::no_ws_split, nullptr},        {"OMC_SEGV_TRACE", &Tuning::segv_trace, nullptr},
  {"OMC_SETUP_GRAM_INLINE", &Tuning::setup_gram_inline, nullptr},
  {"OMC_SHOR_EXPLICIT", &Tuning::shor_explicit, nullptr},    {"OMC_SHOR_NO_SUBSPACE", &Tuning::shor_no_subspace, nullptr},
  {"OMC_COLPROX_BLOCK_MIN", nullptr, &Tuning::colprox_block_min},  {"OMC_COLPROX_DPP", nullptr, &Tuning::colprox_dpp},
  {"OMC_CHECK_XS", nullptr, &Tuning::check_xs},              {"OMC_CONE_MULTI_MIN", nullptr, &Tuning::cone_multi_min},
  {"OMC_EVENT_MERGE", nullptr, &Tuning::event_merge},
  {"OMC_GRAPH_MAX", nullptr, &Tuning::graph_max},            {"OMC_SHOR_SELECT_KB", nullptr, &Tuning::shor_select_kb},
  {"OMC_SHOR_INDEX_DEVICE_MIN", nullptr, &Tuning::shor_index_device_min},
  {"OMC_HARVEST_ASYNC", nullptr, &Tuning::harvest_async},    {"OMC_HARVEST_ASYNC_MIN_LIVE", nullptr, &Tuning::harvest_async_min_live},
  {"OMC_WS_QUIET", nullptr, &Tuning::ws_quiet},
  {"OMC_STREAMS", nullptr, &Tuning::streams},                {"OMC_PLAIN_MULTI_MIN", nullptr, &Tuning::plain_multi_min},
  {"OMC_SUB_DEBUG", nullptr, &Tuning::sub_debug},            {"OMC_SUB_QMAX", nullptr, &Tuning::sub_qmax},
  {"OMC_SMALL_CHAIN", nullptr, &Tuning::small_chain},
  {"OMC_TIMING_STRIDE", nullptr, &Tuning::timing_stride},
};

struct omc_instance {
  int n = 0, m = 0, k = 0, device = 0, nnz = 0, cmax = 0;
  double gamma = 0, sumA2 = 0;
  std::vector<int> col_ptr, col_idx; std::vector<double> col_val;
  std::vector<double> A; std::vector<uint8_t> mask;
  std::vector<double> Ncnt;
  std::vector<int> row_ptr, row_idx; std::vector<double> row_val;
  DevBuf drow_ptr, drow_idx, drow_val, aR, arkind, arcut, arbi, arbj, arcoef, arrhs, acutx, aU0, aU, aV, aobj, aint, aG, aG2;
  hipStream_t stream = nullptr;
  Tuning tun;
  // main / column / small-cone streams of an iteration and its fork, join, done events (see omc_relax_solve)
  hipStream_t gs[3] = {};
  hipEvent_t gev[5] = {};
  hipEvent_t gevc[5] = {};      // the same fork / join events for bodies recorded under stream capture: an event is never used both inside a captured graph and eagerly
  hipEvent_t ev_main = nullptr;
  // between the iterations (check, harvest, refill): page-locked images of the slot flags and of the slot list, two of each so that the host
  // writes one while the copy of the other may still be in flight (ev_up: recorded behind each copy, waited for before the image is rewritten),
  // of the done flags, and of the (slot, node) jobs of k_setup_gram with their device copy; ev_gram marks that kernel's end on its stream
  PinBuf pin_flags[2], pin_list[2], pin_done, pin_jobs; DevBuf bgramjobs;
  hipEvent_t ev_up[4] = {}; bool ev_up_rec[4] = {}; hipEvent_t ev_gram = nullptr; bool ev_gram_rec = false;
  // host time of the last solve between the iterations, by piece (omc_last_host_phases): milliseconds and events
  double host_ms[OMC_HOST_NPHASE] = {0}; int64_t host_cnt[OMC_HOST_NPHASE] = {0};
  DevBuf dA, dmask, dcol_ptr, dcol_idx, dcol_val, dNcnt, dwY, dsolo, dwide;
  int nwide = 0;      // columns outside the pairs with at most 64 observed rows (k_colprox_wide)
  int nsolo = 0;      // columns that k_colprox_pair leaves to k_colprox (more than 32 observed rows, unpaired last column)
  // k_colprox_block: its two column lists (tiles in LDS / in the slab), the per-column flag, the longest column of each list, the non-empty
  // columns it leaves and the longest of them; the lists follow (block_min, pair kernel on) and are rebuilt at a stage call when either changed
  DevBuf dblock, dslab, disblock, bcpb, bnfact;
  int nblock = 0, nslab = 0, nrest = 0, cpb_cl = 0, cpb_cs = 0, crest_max = 0;
  bool lists_valid = false; int lists_block_min = 0; bool lists_pair = true;
  // batch workspace
  DevBuf bYx, bY, bYp, bU, bD1, bD3, bW1, bE3, bQb, brr, bsm, bdS, balpha, balphaX, bsval, bMchk, bsmall, bchk;
  DevBuf bR, brkind, brcut, brbi, brbj, brcoef, brrhs, bcutx, bG, blam;
  DevBuf bobjcol, baaF, baaG, baaZ, baaS, baaI, bMbufC, bVrowC, bchkS, bchkI;
  DevBuf bslotlist, bgap, bvotes, blamDX, bXsC, bsubSC, bsubIC;
  DevBuf bsubz, bscal, bbx, bint, bcp, bcone, bglob, bXout, bThout, bXin, bMbuf, bVrow, bXs, bsubS, bsubI;
  long long sub_tot[8] = {0};
  DevBuf bmwstat, sbigmw, pjM, pjV, pjW, pjS, pjD, pjI;      // sweep statistics of the multi-workgroup eigen-kernels (base workspace, Shor view) ; buffers of omc_psd_project_batch
  long long mw_tot[5] = {0};      // omc_last_cone_multi_stats
  DevBuf bpmwstat; long long pmw_tot[4] = {0};      // the plain operations on those kernels: per-slot counters (OmcWS::pmw_stat), omc_last_plain_multi_stats
  OmcWS ws{};
  omc_relax_params params{};
  bool staged = false;
  double last_solve_seconds = 0; long long total_sweeps = 0; int last_iters_total = 0;
  std::thread worker; std::atomic<int> worker_running{0}, nodes_done{0}; int worker_rc = 0; std::string worker_err;
  // appending nodes to a staged / running batch (omc_relax_reserve, omc_relax_append): descriptor and output arrays are sized for node_cap nodes,
  // the strides (rows, row-subspace columns, cuts per node) for reserve_cuts cuts; Btot_live is what the solve loop reads at its refill points
  int reserve_nodes = 0, reserve_cuts = 0, node_cap = 0, staged_cut_type = 0; std::atomic<int> Btot_live{0}; bool append_closed = true; std::mutex append_mu; hipStream_t append_stream = nullptr;
  // omc_relax_append_children: per node of the capacity its cuts, rows and an upper bound of its row-subspace columns (staged and appended nodes:
  // from their NodePack; a child: L + 1, R + 2k + 1, min(n, r + 1)), written at stage time and under append_mu, so that every refusal is
  // decided without a device read; scratch and index image of the branch kernels (walk_branch_*), sized at stage time for BRANCH_CHUNK children
  std::vector<int> node_L, node_R, node_r; DevBuf bbrS, bbrI; bool br_ready = false;
  std::atomic<int> hold{0};      // omc_relax_hold: a solve that has run dry waits for omc_relax_append instead of ending
  std::vector<int> done_q; size_t done_read = 0; std::mutex done_mu; hipStream_t fetch_stream = nullptr;      // nodes harvested so far, in harvest order (omc_relax_fetch_done)
  void* comm = nullptr; int comm_rank = 0, comm_world = 1; DevBuf bcomm, amobj; int amobj_B = 0;
  int wall_khz = 0;      // rate of the device's constant clock (wall_clock64) for the time_limit of omc_altmin_batch; 0: unknown, the limit is not enforced inside a launch
  std::vector<double> rho_scale_per_node; DevBuf brho, brhon, blamD, bslotint, boY, boU, boal, bobx, boscal, boint;
  int Btot = 0;
  // best certificates per node (omc_relax_keep_certificates): asked for before a stage call; that call allocates the per-slot buffers and the
  // per-node arena (OmcWS::cert_flag ...) and nothing exists while the request is off
  bool keep_cert = false; DevBuf bcbD, bcbI, bocD, bocI;
  // the same for Shor mode (omc_relax_keep_shor_certificates), a switch of its own: the omc_relax_stage_shor call allocates the base buffers above
  // without Lam (lam, Psi3, bound, flags) and the Shor ones (ShWS::cbGam ...)
  bool keep_shor_cert = false; DevBuf scbD, socD, socNq;
  DevBuf dbD, dbI, dbM, dbS, dbL;      // omc_dual_bound_batch: descriptors and multipliers, ints, matrices, eigen-kernel slab, dense Lam
  // omc_shor_dual_bound_batch: every double (multipliers, scratch, descriptors, matrices, slab), every int, and the index structures of the
  // call's distinct lists (ints, bytes, group table); event time of the last call's kernels in ms (omc_last_shor_dual_bound_ms)
  DevBuf sdD, sdI, sdGi, sdGb, sdGr; double sdb_ms = 0.0;
  // Shor minors (a10 / a11): row bitsets and per-pair popcounts, built at the first call
  DevBuf sbits, scb, scx, scz, soff, stot, sout, shi, slo, sexist, shist, sohi, solo, scnt;
  bool shor_ready = false; int shor_W = 0; long long shor_pairs = 0;
  double shor_last_ms = 0; long long shor_last_candidates = 0;
  int64_t shor_sel[4] = {0, 0, 0, 0};      // omc_shor_last_select_stats: streamed, tiles, compactions, peak key / survivor bytes
  // Shor-mode relaxation (omc_relax_stage_shor): index structures of the distinct lists, explicit X / W / Theta state, view of the workspace
  // through which the base eigen-kernels project the order-(n+m) cone
  bool shor_on = false, shor_keep_V = false, shor_via_base = false; std::vector<int> shor_slackrow; DevBuf soV; double shor_rho = 0.05, shor_r4 = 0.0, shor_r5 = 2.0;      // r4 = 0: automatic per list
  ShWS sh{}; OmcWS wbig{};
  DevBuf sgInts, sgBytes, sgGroups, sgNodeGroup, sAh, sX, sW, sTh, sV1, sV2, sV3, sD0, sP0, sMbufB, sVrowB, sTq, sPq, sNq, sD5x, sD5t, snu5, sP5x,
      scolpart, sminpart, sminpart2, sfroB, svvB, se1, se2, soX, soW, soTh, sbigscr, sXsB, ssubSB, ssubIB;
  long long big_sub_tot[8] = {0};
  // appending Shor nodes (omc_relax_reserve_shor, omc_relax_append_shor): the reservation of the NEXT omc_relax_stage_shor, and for the life of the
  // staged batch the lists it knows (staged or appended; hash -> groups, with a host copy of every list to tell equal hashes apart), the group
  // table's capacity and how much of the two index arenas is in use.  Written at stage time and under append_mu.
  struct ShorListKey { int64_t nq = 0, nsoc = 0; uint64_t hlist = 0; std::vector<int64_t> idx, soc; };
  int64_t reserve_shor_nq = 0; int reserve_shor_lists = 0; bool reserve_shor_set = false;
  std::unordered_map<uint64_t, std::vector<int>> sh_byhash; std::vector<ShorListKey> sh_lists;
  int sh_group_cap = 0; size_t sh_int_used = 0, sh_int_cap = 0, sh_byte_used = 0, sh_byte_cap = 0;
  // index structures built on the device (OMC_SHOR_INDEX_DEVICE_MIN, omc_shor_index_build): sort scratch and the staging room in which built
  // lists wait until every refusal of a call is decided, one packed buffer (walk_shor_index) that only grows and never while a solve runs;
  // the knob's value for the staged batch (appends follow it); lists and milliseconds since the last stage call, launches of the last build
  DevBuf sxD; ShorIndexDims sx_dims{}; ShorIndexWS sx{}; int* sx_stage_int = nullptr; uint8_t* sx_stage_byte = nullptr;
  int sh_index_min = 0; double shidx_stats[5] = {0, 0, 0, 0, 0};      // host lists, device lists, host ms, device ms, launches
  // warm-start pool (omc_state_pool_create / omc_relax_set_warm)
  int pool_cap = 0; DevBuf pY, pD1, pD3, pU, palpha, psval, pXs, ptheta, pscal, bwarmL, bwarmS; std::vector<int> warm_load, warm_save;
  // Shor extension of the pool (omc_state_pool_reserve_shor) and the host's signature of every entry: which mode saved it and for which lists.
  // A signature is written when the node that saves is harvested (solve thread) and read at stage / append time (caller's thread): sig_mu.
  struct PoolSig { int kind = 0; int64_t nq = 0, nsoc = 0; uint64_t hlist = 0, hsoc = 0; };      // kind: 0 empty, 1 base, 2 Shor
  bool pool_shor = false; int64_t pool_nqmax = 0; DevBuf pShor, pShorHdr, sloadpart;
  std::vector<PoolSig> pool_sig, node_sig; std::mutex sig_mu;
  std::vector<int> save_host;      // per node of the staged batch: the entry its final state goes to (-1: none), as the device sees it
  int64_t shor_warm_stats[4] = {0, 0, 0, 0};      // omc_last_shor_warm_stats
  // Objective cutoff (omc_relax_set_cutoff): the value lives here and survives staging; the device holds a copy in a buffer of its own
  // (OmcWS::cutoff points at it, set again by every stage call) that the setter refreshes with one 8-byte copy from its page-locked image on
  // a stream of its own (created by the first call), under cutoff_mu.  The setter touches nothing else: not the workspace, no DevBuf::ensure, not the tuning map.
  // cutoff_armed: some value other than +inf has been given since the running solve began (or before it) -- only then does a check read the
  // slots' statuses back for the counters.  The counters are reset where a solve begins (omc_relax_submit, or omc_relax_solve called directly).
  DevBuf bcutoff; PinBuf pin_cutoff; hipStream_t cutoff_stream = nullptr; std::mutex cutoff_mu; std::atomic<double> cutoff{HUGE_VAL};
  std::atomic<int> cutoff_armed{0}, solve_active{0}; std::atomic<int64_t> cutoff_nodes{0}, cutoff_iters{0}, cutoff_live{0};
  // kernel stats
  int64_t launches[OMC_KERNEL_NCLASS] = {0}; double ms[OMC_KERNEL_NCLASS] = {0}; int64_t units[OMC_KERNEL_NCLASS] = {0};
  size_t nnz_rows() const { return row_idx.size(); }
  // timing events: two pools that swap at a check, so that the pool of the interval that has just ended is read after the next iteration has
  // been enqueued while the launches of that iteration record into the other one.  Which event is recorded where, and which launch it times, is
  // kept by the solve loop's EventTape (omc_events.h) for the length of a solve; the events themselves live as long as the instance.
  std::vector<hipEvent_t> ev_pool[2];
};

static constexpr int MAX_SWEEPS = 30;          // sweep cap of the warm-started Jacobi kernel (k_cone_ws)
