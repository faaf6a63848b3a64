// omc_relax_solve.cpp -- the solve loop of a staged batch: omc_relax_solve and the two host rules it exports for the tests.
//
// Two things happen between the ADMM iterations: the slot bookkeeping (which node a slot holds, what is parked or in flight, which node is
// next: SlotBook, omc_slots.h -- plain C++, no device call) and the HIP enqueue order on four streams (SolveLoop below, one member function
// per phase).  SlotBook says what to enqueue; SolveLoop enqueues it.
#include <algorithm>
#include <chrono>
#include <stdio.h>

#include "omc_events.h"
#include "omc_api_internal.h"
#include "omc_host.h"
#include "omc_slots.h"

static_assert(SLOT_HARVEST_NONE == OMC_HARVEST_NONE && SLOT_HARVEST_SYNC == OMC_HARVEST_SYNC && SLOT_HARVEST_ASYNC == OMC_HARVEST_ASYNC, "omc_slots.h restates the plans of omc.h");

namespace {

using Clock = std::chrono::steady_clock;

// totals of a view's tracked-subspace counters (8 per slot), which are then cleared
int sum_sub_stat(int* sub_stat, int S, long long tot[8], hipStream_t s) {
  std::vector<int> ss(8 * (size_t)S);
  HIPCHK(hipMemcpyAsync(ss.data(), sub_stat, sizeof(int) * ss.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int q = 0; q < 8; ++q) tot[q] = 0;
  for (int b = 0; b < S; ++b) for (int q = 0; q < 8; ++q) tot[q] += ss[8 * b + q];
  HIPCHK(hipMemsetAsync(sub_stat, 0, sizeof(int) * ss.size(), s));
  return 0;
}

// EventTape's backend: the tape's streams are T_S (the instance's stream) and the three streams of an iteration (with OMC_STREAMS=1 all four
// are one stream, and one id), its events the two pools of the instance, which grow on demand.
enum { T_S = 0, T_M = 1, T_B = 2, T_C = 3, T_NSTREAM = 4 };
struct HipEvents {
  omc_instance* h; hipStream_t st[T_NSTREAM] = {}; hipError_t last = hipSuccess;
  bool record(int pool, int i, int stream) {
    std::vector<hipEvent_t>& p = h->ev_pool[pool];
    while (p.size() <= (size_t)i) {
      hipEvent_t e;
      if ((last = hipEventCreate(&e)) != hipSuccess) return false;
      p.push_back(e);
    }
    return (last = hipEventRecord(p[i], st[stream])) == hipSuccess;
  }
  bool wait(int stream, int pool, int i) { return (last = hipStreamWaitEvent(st[stream], h->ev_pool[pool][i], 0)) == hipSuccess; }
};
using Tape = EventTape<HipEvents>;

// Per-kernel timing: the launch `call` on the stream with the tape's id `id`, between a start and a stop event of the tape; finish_events reads
// the pair.  If the tape has no event to give (one cannot be created, a record fails) the launch runs, and is counted, untimed.
// counted = false: a launch timed into class `cls` that is not one of the class's launches (k_setup_gram: ms of the setup class, see
// omc_last_kernel_stats).
#define TIMED_ON(id, cls, counted, units_, call)                                                          \
  do {                                                                                                    \
    const Tape::Ev t0_ = tape.begin(id);                                                                  \
    call;                                                                                                 \
    tape.touch(id);                                                                                       \
    if (t0_.valid()) { const Tape::Ev t1_ = tape.end(id); if (t1_.valid()) tape.launch(t0_, t1_, cls); }  \
    if (counted) { h->launches[cls] += 1; h->units[cls] += (units_); }                                    \
  } while (0)
#define TIMED(cls, units_, call) TIMED_ON(T_S, cls, true, units_, call)

// The state of one solve.  Every exit of omc_relax_solve, error exits included, closes the batch to omc_relax_append (CloseGuard) and
// destroys the graph executables (GraphGuard).
struct SolveLoop {
  struct CloseGuard { omc_instance* h; ~CloseGuard() { std::lock_guard<std::mutex> lk(h->append_mu); h->append_closed = true; h->ws.Btot = h->Btot_live.load(); h->Btot = h->ws.Btot; if (h->shor_on) h->sh.Btot = h->ws.Btot; } };
  struct ActiveGuard { omc_instance* h; ~ActiveGuard() { h->solve_active.store(0); } };      // omc_relax_set_cutoff counts the calls it takes while a solve runs
  struct GraphGuard { hipGraphExec_t e[2] = {nullptr, nullptr}; ~GraphGuard() { for (int q = 0; q < 2; ++q) if (e[q]) (void)hipGraphExecDestroy(e[q]); } };

  omc_instance* const h;
  CloseGuard close_guard; ActiveGuard active_guard;
  const OmcWS& w; const ShWS& sw; const omc_relax_params& P;
  const Tuning tun;      // copied once: omc_tuning_set may run on the caller's thread while a submitted solve runs on the worker
  const int S, check_every;
  // Streams.  Inside an iteration the three blocks are independent of each other (columns: Y, Yp, alpha -> alpha, Lambda;
  // cone: Y - D1 -> W1; small cone: Y, D3, V -> E3, W3*): a main stream (cone, then the global step) and two side streams
  // (columns, small cone) forked and joined by events, so that the latency-bound column waves and the small workgroups
  // share the CUs with the LDS-bound cone kernel (measured on config 2, 2048 slots: 212 -> 235 node-relaxations/s).
  // OMC_STREAMS=1 serialises everything on one stream (kernel-by-kernel measurements).
  const bool multi, shor;
  const hipStream_t s;
  hipStream_t sm = nullptr, sb = nullptr, sc = nullptr;
  int im = T_S, ib = T_S, ic = T_S;      // their ids on the tape
  // Event records.  Timing brackets every launch of a sampled iteration with two events, and the fork and the joins of the three streams are
  // events too; most of them mark a point of a stream that an event already marks (the stop of k_global, the fork and the start of k_cone_sub
  // are one point of the main stream).  The tape hands the event that is still adjacent out again (omc_events.h), and the fork and the joins
  // of a timed iteration wait for the tape's events: 8 records instead of 13 in a quiet iteration, 10 instead of 16 in a split one.  Every
  // enqueue on one of the four streams that is not a record of the tape tells the tape (touch).  On the instance's stream adjacency is trusted
  // only inside one enqueue function (setup_slots, enqueue_check, enqueue_harvest touch it when they begin): copies and fills go there from
  // many places.  OMC_EVENT_MERGE=0: the order before the tape, record for record.
  // A pool event is recorded once per generation of its pool, and a pool is drained (finish_events) only after the check that follows the
  // interval it was filled in: every wait that names one of its events was enqueued in that interval, two checks before the event is
  // recorded again.
  HipEvents hip_events; Tape tape;
  int Btot;      // nodes staged so far: omc_relax_append may add more while the loop runs (re-read at every check)
  int* done = nullptr; int* jobs = nullptr;      // page-locked images of the done flags and of the k_setup_gram jobs (prepare)
  SlotBook book;
  std::vector<int> harvested_ids, cut_img;
  int harvested = 0, it = 0, nlist = 0, flags_cur = 0, list_cur = 0;
  bool timed_out = false;
  int drain_pool = -1;       // timing-event pool that waits to be read (finish_events): filled up to the last check, read after the next iteration is enqueued
  bool wait_main = true;     // the iteration streams must wait for the work queued on the main stream (setup, checks, refills)
  bool ev_main_set = false;  // ev_main has been recorded for the next iteration already (ahead of the harvest kernels)
  // Multi-workgroup eigen-kernels (geo.mw): a call is a sequence of launches whose sweep budget the host fixes when it enqueues them.  The
  // budget is the full bound while a slot may be on its first call (cold start), else the most sweeps a call needed since the last check + 2
  // (read at the check, where the host synchronises anyway).  An interval without a call (the tracked block served every slot) says nothing
  // about the next one, a fall-back from a basis that has gone stale: omc_cone_multi_budget then gives the full bound again.
  // [0] base cone, [1] big cone of Shor mode; the certificate launches keep the bound.
  bool mw_any = false; int mw_budget[2] = {MAX_SWEEPS, MAX_SWEEPS};
  // The full eigen-kernel runs the slots that have no tracked block (or are backing off) -- a handful per launch, each a long single-workgroup
  // job, known before the iteration starts (ws_first) -- on a stream of its own beside k_cone_sub; what k_cone_sub then could not do (a failed
  // call, ~1 in 30 000) is a second, almost empty launch behind both.  One launch after k_cone_sub made every iteration wait for the sum.
  bool split_solve = false;
  // Quiet intervals: with warm starts the full kernel has nothing to do for whole intervals (w.ws_need stayed 0), and its two launches are then
  // two empty links in the latency chain of an iteration that is not saturated.  An interval after a check that found the word 0 and set no
  // slot up enqueues the unsplit form -- one launch behind k_cone_sub, which also serves a call that fails inside the interval (serially, for
  // that iteration; the word is then set and the next interval is split again).  The two forms are bit-identical.  A captured graph keeps
  // the split it was captured with.
  bool quiet = false, quiet_next = false;
  // Small batches are launch-bound (batch 1: ~190 us of launches, event records and waits around ~115 us of kernels per iteration; replayed:
  // 266 instead of 322 us): the body of an iteration (fork, three concurrent blocks, join, global step) is captured once into a hipGraph and
  // replayed -- only for batches that are small FROM THE START (<= OMC_GRAPH_MAX = 16 nodes staged: one capture per solve).  The draining tail
  // of a large batch re-captured the graph at every harvest, and a sporadic host crash inside omc_relax_solve was seen three times in round 3,
  // always in or after solves on that path, never with replay off; not located.  Per-kernel HIP-event timing is not
  // available inside a graph, so the large batches that the bench times keep the eager path.
  int graph_max = 0, gexec_n = -1; GraphGuard graphs;
  // per check: slots the asynchronous harvest of the previous check refilled; the slot list has gone out already
  int nrefilled = 0; bool list_pushed = false;
  // Shor mode: a node is also checked at its iteration cap when the cap is no multiple of check_every (as the oracle does: it % check_every
  // == 0 or it == max_iters, counted from the node's own start).  starts: the iterations at which slots were set up and whose nodes may still
  // run.  With caps on the grid every start is on it and nothing is added to the checks.
  std::vector<int> starts;
  // (omc_last_host_phases also carries two counts of the iterations themselves: the event records and the stream waits they enqueued)
  // host stamps between the iterations (omc_last_host_phases): stamp(q) charges the time since the previous stamp to piece q
  const Clock::time_point t0; Clock::time_point t_last, t_check;

  explicit SolveLoop(omc_instance* h_)
      : h(h_), close_guard{h_}, active_guard{h_}, w(h_->ws), sw(h_->sh), P(h_->params), tun(h_->tun), S(h_->ws.B), check_every(std::max(1, h_->params.check_every)),
        multi(h_->tun.streams > 1), shor(h_->shor_on), s(h_->stream),
        hip_events{h_}, tape(&hip_events, T_NSTREAM, h_->tun.event_merge != 0), Btot(h_->Btot_live.load()), book(h_->ws.B, nullptr, nullptr), t0(Clock::now()), t_last(t0), t_check(t0) {}

  void stamp_begin() { t_last = Clock::now(); }
  void stamp(int q) { const auto t = Clock::now(); h->host_ms[q] += std::chrono::duration<double, std::milli>(t - t_last).count(); h->host_cnt[q] += 1; t_last = t; }
  double elapsed() const { return std::chrono::duration<double>(Clock::now() - t0).count(); }

  // every launch the pool has timed must have completed
  void finish_events(int pool) {
    for (const Tape::Launch& l : tape.launches(pool)) {
      float msv = 0.f;
      if (hipEventElapsedTime(&msv, h->ev_pool[pool][l.start], h->ev_pool[pool][l.stop]) == hipSuccess) h->ms[l.cls] += msv;
    }
    tape.drain(pool);
  }

  // `to` (and `to2`, if >= 0) wait for the present end of the queue of `from`.  on_tape: that point is an event of the tape -- the stop event of
  // the last launch on `from` when nothing has followed it; otherwise, or when the tape has no event to give, `fb` is recorded for it.
  int depend(int from, int to, int to2, bool on_tape, hipEvent_t fb, bool counted = true) {
    if (on_tape) {
      const Tape::Ev e = tape.mark(from);
      if (e.valid()) {
        if (!tape.wait(to, e) || (to2 >= 0 && !tape.wait(to2, e))) HIPCHK(hip_events.last);
        return 0;
      }
    }
    HIPCHK(hipEventRecord(fb, hip_events.st[from])); tape.touch(from); if (counted) tape.count_record();
    HIPCHK(hipStreamWaitEvent(hip_events.st[to], fb, 0)); tape.touch(to); if (counted) tape.count_wait();
    if (to2 >= 0) { HIPCHK(hipStreamWaitEvent(hip_events.st[to2], fb, 0)); tape.touch(to2); if (counted) tape.count_wait(); }
    return 0;
  }
  // the two side streams join the main stream: both points first, then both waits
  int join_sides(bool on_tape, hipEvent_t fb_b, hipEvent_t fb_c, bool counted) {
    Tape::Ev eb, ec;
    if (on_tape) eb = tape.mark(ib);
    if (!eb.valid()) { HIPCHK(hipEventRecord(fb_b, sb)); tape.touch(ib); if (counted) tape.count_record(); }
    if (on_tape) ec = tape.mark(ic);
    if (!ec.valid()) { HIPCHK(hipEventRecord(fb_c, sc)); tape.touch(ic); if (counted) tape.count_record(); }
    if (eb.valid()) { if (!tape.wait(im, eb)) HIPCHK(hip_events.last); }
    else { HIPCHK(hipStreamWaitEvent(sm, fb_b, 0)); tape.touch(im); if (counted) tape.count_wait(); }
    if (ec.valid()) { if (!tape.wait(im, ec)) HIPCHK(hip_events.last); }
    else { HIPCHK(hipStreamWaitEvent(sm, fb_c, 0)); tape.touch(im); if (counted) tape.count_wait(); }
    return 0;
  }

  // ---- host images and their uploads ------------------------------------------------------------------------------------------------
  // Page-locked images (see omc_instance): an upload returns at once, and an image is rewritten only after the copy that last read it has
  // completed (its event; two images alternate, so that wait is over long before it is asked for)
  int image_free(int q) {      // q: 0, 1 flags; 2, 3 slot list
    if (h->ev_up_rec[q]) { HIPCHK(hipEventSynchronize(h->ev_up[q])); h->ev_up_rec[q] = false; }
    return 0;
  }
  // sync: the caller needs the stream drained behind the upload (the harvest kernels' outputs); nothing else waits for a flags upload
  int push_flags(bool sync) {
    const int q = flags_cur; flags_cur ^= 1;
    { int rc = image_free(q); if (rc) return rc; }
    int* flags = h->pin_flags[q].as<int>();
    book.write_flags(flags);
    HIPCHK(hipMemcpyAsync(w.node_of, flags, sizeof(int) * 3 * (size_t)S, hipMemcpyHostToDevice, s));
    tape.touch(T_S);
    HIPCHK(hipEventRecord(h->ev_up[q], s)); h->ev_up_rec[q] = true;
    if (sync) HIPCHK(hipStreamSynchronize(s));
    return 0;
  }
  // compact list of the slots that hold a running node: the per-iteration kernels launch over it (rebuilt when slots finish or are refilled)
  int push_list() {
    const int q = list_cur; list_cur ^= 1;
    { int rc = image_free(2 + q); if (rc) return rc; }
    int* alist = h->pin_list[q].as<int>();
    nlist = book.write_list(alist);
    tape.touch(T_S);
    if (nlist) { HIPCHK(hipMemcpyAsync(h->bslotlist.p, alist, sizeof(int) * nlist, hipMemcpyHostToDevice, s)); HIPCHK(hipEventRecord(h->ev_up[2 + q], s)); h->ev_up_rec[2 + q] = true; }
    return 0;
  }

  // ---- setting slots up ---------------------------------------------------------------------------------------------------------------
  // The Gram matrix of the rows of every node that is about to get a slot (k_setup_gram): G depends on the node's descriptor only and nothing
  // but k_setup and k_global touches it, so it is formed on the column stream -- idle between a check and the next iteration -- beside the
  // harvest kernels of the slot's previous node, and joined to the main stream behind k_setup (gram_join), ahead of the next k_global.
  // jobs: (slot, node) pairs in pin_jobs.  Its time goes to the setup class; it is not a launch of that class.
  int gram_launch(int njobs) {
    if (tun.setup_gram_inline || njobs <= 0) return 0;
    for (int q = 0; q < njobs; ++q)      // the host builds the list: a job outside the slots or the nodes is a bookkeeping error, not something to skip
      if (jobs[2 * q] < 0 || jobs[2 * q] >= S || jobs[2 * q + 1] < 0 || jobs[2 * q + 1] >= Btot) return fail(OMC_ERR_ARGUMENT, "omc_relax_solve: k_setup_gram job outside the slots / nodes");
    HIPCHK(hipMemcpyAsync(h->bgramjobs.p, jobs, sizeof(int) * 2 * (size_t)njobs, hipMemcpyHostToDevice, sb));
    tape.touch(ib);
    TIMED_ON(ib, OMC_KERNEL_SETUP, false, 0, omc_launch_setup_gram(&w, h->bgramjobs.as<int>(), njobs, Btot, sb));
    HIPCHK(hipEventRecord(h->ev_gram, sb)); h->ev_gram_rec = true;      // the host waits for this one (gram_jobs_free): an event of its own
    tape.touch(ib);
    return 0;
  }
  int gram_jobs_free() {      // before pin_jobs is rewritten
    if (h->ev_gram_rec) { HIPCHK(hipEventSynchronize(h->ev_gram)); h->ev_gram_rec = false; }
    return 0;
  }
  int gram_join() {
    if (h->ev_gram_rec && sb != s) { HIPCHK(hipStreamWaitEvent(s, h->ev_gram, 0)); tape.touch(T_S); }
    return 0;
  }
  // What every site that hands nodes to slots ends with, once the job list and the init flags have gone out (when they go differs by site):
  // the Shor state of the slots (before the base setup, which clears the init flags), k_setup, the Gram matrices joined behind it, and the
  // first calls of the new nodes are cold -- the full sweep budget, no quiet interval.
  int setup_slots(int units) {
    tape.touch(T_S);
    if (shor && std::find(starts.begin(), starts.end(), it) == starts.end()) starts.push_back(it);
    if (shor) omc_shor_launch_setup(&sw, s);
    TIMED(OMC_KERNEL_SETUP, units, omc_launch_setup(&w, s));
    { int rc = gram_join(); if (rc) return rc; }
    mw_budget[0] = mw_budget[1] = MAX_SWEEPS;
    quiet = quiet_next = false;
    return 0;
  }

  int prepare() {
    for (int c = 0; c < OMC_KERNEL_NCLASS; ++c) { h->launches[c] = 0; h->ms[c] = 0; h->units[c] = 0; }
    tape.reset();
    for (int q = 0; q < OMC_HOST_NPHASE; ++q) { h->host_ms[q] = 0; h->host_cnt[q] = 0; }
    for (int q = 0; q < 2; ++q) { int rc = h->pin_flags[q].ensure(sizeof(int) * 3 * (size_t)S); if (rc) return rc; rc = h->pin_list[q].ensure(sizeof(int) * (size_t)S); if (rc) return rc; }
    { int rc = h->pin_done.ensure(sizeof(int) * ((size_t)S + 1)); if (rc) return rc; rc = h->pin_jobs.ensure(sizeof(int) * 2 * (size_t)S); if (rc) return rc; rc = h->bgramjobs.ensure(sizeof(int) * 2 * (size_t)S); if (rc) return rc; }
    for (int q = 0; q < 4; ++q) { if (!h->ev_up[q]) HIPCHK(hipEventCreateWithFlags(&h->ev_up[q], hipEventDisableTiming)); h->ev_up_rec[q] = false; }
    if (!h->ev_gram) HIPCHK(hipEventCreateWithFlags(&h->ev_gram, hipEventDisableTiming));
    h->ev_gram_rec = false;
    if (multi && !h->ev_main) {
      for (hipStream_t& q : h->gs) HIPCHK(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
      for (int q = 0; q < 5; ++q) { HIPCHK(hipEventCreateWithFlags(&h->gev[q], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&h->gevc[q], hipEventDisableTiming)); }
      HIPCHK(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
    }
    sm = multi ? h->gs[0] : s; sb = multi ? h->gs[1] : s; sc = multi ? h->gs[2] : s;
    if (multi) { im = T_M; ib = T_B; ic = T_C; }
    hip_events.st[T_S] = s; hip_events.st[T_M] = sm; hip_events.st[T_B] = sb; hip_events.st[T_C] = sc;
    h->ws.setup_gram_inline = tun.setup_gram_inline ? 1 : 0;
    h->ws.small_chain = tun.small_chain ? 1 : 0;
    h->ws.check_xs = std::min(std::max(0, tun.check_xs), CB_XS);      // at most CB_XS doubles are staged: more vectors than that never fit
    // with omc_relax_reserve there may be more slots than nodes staged so far: the others start idle
    done = h->pin_done.as<int>(); jobs = h->pin_jobs.as<int>();
    book = SlotBook(S, jobs, done);
    int rc = gram_launch(book.start(Btot)); if (rc) return rc;
    rc = push_flags(false); if (rc) return rc;
    if (book.active() < S) { HIPCHK(hipMemcpyAsync(w.done, done, sizeof(int) * S, hipMemcpyHostToDevice, s)); HIPCHK(hipStreamSynchronize(s)); }      // idle slots are skipped by every kernel
    rc = setup_slots(S); if (rc) return rc;
    rc = push_list(); if (rc) return rc;
    h->total_sweeps = 0;
    graph_max = Btot <= tun.graph_max ? tun.graph_max : 0;
    mw_any = w.geo.mw || w.geo.plain_mw || (shor && h->wbig.geo.mw);      // plain_mw: 30 (nb - 1) + 4 launches per harvest (omc_launch_cone_plain_mw)
    for (int q = 0; q < 5; ++q) h->mw_tot[q] = 0;
    for (int q = 0; q < 4; ++q) h->pmw_tot[q] = 0;
    split_solve = multi && !tun.no_ws_split && w.sub_enable && w.geo.ws_lpp && w.ws_first;
    return 0;
  }

  // nodes appended while every slot was idle (or while the loop was about to end): hand them to idle slots
  int refill_idle() {
    if (book.next_node() >= Btot) return 0;
    int rc = gram_jobs_free(); if (rc) return rc;
    const int ninit = book.refill_idle(Btot);
    if (!ninit) return 0;
    rc = gram_launch(ninit); if (rc) return rc;
    rc = push_flags(false); if (rc) return rc;
    rc = setup_slots(ninit); if (rc) return rc;
    rc = push_list(); if (rc) return rc;
    wait_main = true;
    return 0;
  }

  // nodes [next, Btot) that never got a slot: status `st` without values
  int close_unslotted(int st) {
    const int first = book.close_unslotted(Btot);
    if (first >= Btot) return 0;
    const size_t c = (size_t)(Btot - first);
    std::vector<int> stv(c, st), itz(c, 0);
    std::vector<double> inf(c, 1e300), ninf(c, -1e300);
    HIPCHK(hipMemcpyAsync(w.ostatus + first, stv.data(), sizeof(int) * c, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w.oiters + first, itz.data(), sizeof(int) * c, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w.oobj + first, inf.data(), 8 * c, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w.olb + first, ninf.data(), 8 * c, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
  }

  // No slot holds a node.  The end of the batch is decided under the lock omc_relax_append takes: a node is either seen here or refused there.
  int run_dry(bool* ended) {
    *ended = false;
    {
      std::lock_guard<std::mutex> lk(h->append_mu);
      Btot = h->Btot_live.load();
      if (timed_out) { int rc = close_unslotted(OMC_ST_TIME); if (rc) return rc; }      // appended after the time limit struck
      if (book.next_node() >= Btot && (!h->hold.load() || elapsed() > P.time_limit)) { h->append_closed = true; *ended = true; return 0; }
    }
    if (book.next_node() >= Btot) { std::this_thread::sleep_for(std::chrono::microseconds(100)); return 0; }      // held open (omc_relax_hold): wait for the host's next push
    return refill_idle();
  }

  // ---- an iteration -------------------------------------------------------------------------------------------------------------------
  int enqueue_body(const OmcWS& wg, bool timed, bool with_aa, bool capturing) {
    const int gact = book.running();
    const bool split = split_solve && (capturing || !quiet);
    hipEvent_t* const ev = capturing ? h->gevc : h->gev;
    // a timed iteration forks and joins on the tape's events: the fork is the stop event of the previous iteration's last kernel (and the
    // start event of the first kernel on the main stream), a join the stop event of a side stream's last kernel
    const bool tp = timed && !capturing && tun.event_merge;
    const bool cnt = !capturing;
    if (multi) { int rc = depend(im, ib, ic, tp, ev[0], cnt); if (rc) return rc; }
#define MAYBE_TIMED(id, cls, units_, call) do { if (timed) TIMED_ON(id, cls, true, units_, call); else { call; tape.touch(id); } } while (0)
    if (shor) {
      // Shor mode: clip on the main stream, the order-(n+m) cone on the second, small cone + order-5 blocks on the third; then the
      // global step: rows / Y (base kernel), columns (X, W, Theta, duals of the big cone), duals of the order-5 blocks, per-slot sums
      OmcWS wb = h->wbig; wb.nB = wg.nB; wb.slot_list = wg.slot_list;
      if (w.sub_enable) MAYBE_TIMED(im, OMC_KERNEL_CONESUB, gact, omc_launch_cone_sub(&wg, sm));
      if (wb.sub_enable) MAYBE_TIMED(ib, OMC_KERNEL_SHOR_BIGCONE, 0, omc_launch_cone_sub(&wb, sb));
      wb.mw_budget = mw_budget[1];
      if (wb.geo.ws_lpp || wb.geo.mw) MAYBE_TIMED(ib, OMC_KERNEL_SHOR_BIGCONE, gact, omc_launch_cone_ws(&wb, sb));
      else MAYBE_TIMED(ib, OMC_KERNEL_SHOR_BIGCONE, gact, omc_launch_cone(&wb, CONE_BIG, sb));
      if (w.geo.ws_lpp || w.geo.mw) MAYBE_TIMED(im, OMC_KERNEL_CONE, gact, omc_launch_cone_ws(&wg, sm));
      else MAYBE_TIMED(im, OMC_KERNEL_CONE, gact, omc_launch_cone(&wg, CONE_CLIP01, sm));
      MAYBE_TIMED(ic, OMC_KERNEL_SMALL, gact, omc_launch_small(&wg, SMALL_PROJ, sc));
      MAYBE_TIMED(ic, OMC_KERNEL_SHOR_MINORS, gact, { omc_shor_launch_minor_pre(&sw, sc); omc_shor_launch_vkeys(&sw, sc); });
      if (multi) { int rc = join_sides(tp, ev[1], ev[2], cnt); if (rc) return rc; }
      MAYBE_TIMED(im, OMC_KERNEL_GLOBAL, gact, omc_launch_global(&wg, sm));
      MAYBE_TIMED(im, OMC_KERNEL_SHOR_COLS, gact, omc_shor_launch_cols(&sw, sm));
      MAYBE_TIMED(im, OMC_KERNEL_SHOR_MINORS, gact, { omc_shor_launch_minor_post(&sw, sm); omc_shor_launch_reduce(&sw, sm); });
      return 0;
    }
    Tape::Ev e4;
    if (split) {      // on the small-cone stream, behind k_small (a fifth stream would share a hardware queue with one of the other four: measured, k_small then ran behind it)
      MAYBE_TIMED(ic, OMC_KERNEL_SMALL, gact, omc_launch_small(&wg, SMALL_PROJ, sc));
      OmcWS wA = wg; wA.ws_phase = 1;
      MAYBE_TIMED(ic, OMC_KERNEL_CONE, gact, omc_launch_cone_ws(&wA, sc));
      if (tp) e4 = tape.mark(ic);      // the stop event of phase 1
      if (!e4.valid()) { HIPCHK(hipEventRecord(ev[4], sc)); tape.touch(ic); if (cnt) tape.count_record(); }
    }
    // the cone workgroups are few (two per CU, long serial phases) and the column waves many: the cone kernel goes first so that its
    // workgroups are resident when the column kernel floods the wave slots
    if (w.sub_enable) MAYBE_TIMED(im, OMC_KERNEL_CONESUB, gact, omc_launch_cone_sub(&wg, sm));
    MAYBE_TIMED(ib, OMC_KERNEL_COLPROX, (int64_t)gact * w.m, omc_launch_colprox(&wg, 0, sb));
    if (split) {
      if (e4.valid()) { if (!tape.wait(im, e4)) HIPCHK(hip_events.last); }
      else { HIPCHK(hipStreamWaitEvent(sm, ev[4], 0)); tape.touch(im); if (cnt) tape.count_wait(); }
      OmcWS wB = wg; wB.ws_phase = 2;
      MAYBE_TIMED(im, OMC_KERNEL_CONE, 0, omc_launch_cone_ws(&wB, sm));
    }
    else if (w.geo.ws_lpp || w.geo.mw) MAYBE_TIMED(im, OMC_KERNEL_CONE, gact, omc_launch_cone_ws(&wg, sm));
    else MAYBE_TIMED(im, OMC_KERNEL_CONE, gact, omc_launch_cone(&wg, CONE_CLIP01, sm));
    if (!split) MAYBE_TIMED(ic, OMC_KERNEL_SMALL, gact, omc_launch_small(&wg, SMALL_PROJ, sc));
    if (multi) { int rc = join_sides(tp, ev[1], ev[2], cnt); if (rc) return rc; }
    MAYBE_TIMED(im, OMC_KERNEL_GLOBAL, gact, omc_launch_global(&wg, sm));
    if (with_aa) MAYBE_TIMED(im, OMC_KERNEL_ACCEL, gact, omc_launch_aa(&wg, sm));
#undef MAYBE_TIMED
    return 0;
  }

  // (re)capture: one graph without and one with the acceleration kernel at its end
  int capture_body(const OmcWS& wg) {
    hipGraphExec_t* const gexec = graphs.e;
    for (int q = 0; q < 2; ++q) { if (gexec[q]) { (void)hipGraphExecDestroy(gexec[q]); gexec[q] = nullptr; } }
    for (int q = 0; q < (w.accel ? 2 : 1); ++q) {
      hipGraph_t gr = nullptr;
      HIPCHK(hipStreamBeginCapture(sm, hipStreamCaptureModeThreadLocal));
      int rc = enqueue_body(wg, false, q == 1, true);
      hipError_t ce = hipStreamEndCapture(sm, &gr);
      if (rc) { if (gr) (void)hipGraphDestroy(gr); return rc; }
      HIPCHK(ce);
      hipError_t ie = hipGraphInstantiate(&gexec[q], gr, nullptr, nullptr, 0);
      (void)hipGraphDestroy(gr);
      HIPCHK(ie);
    }
    gexec_n = nlist;
    return 0;
  }

  int enqueue_iteration(bool* is_check) {
    ++it;
    *is_check = (it % check_every == 0);
    if (shor) {
      for (int s0 : starts) { const int l = it - s0; if (l == P.max_iters || (s0 % check_every != 0 && l % check_every == 0)) *is_check = true; }
      starts.erase(std::remove_if(starts.begin(), starts.end(), [&](int s0) { return it - s0 >= P.max_iters; }), starts.end());
    }
    if (multi && wait_main && !ev_main_set) { HIPCHK(hipEventRecord(h->ev_main, s)); tape.touch(T_S); }
    ev_main_set = false;
    const long long nrec0 = tape.records(), nwait0 = tape.waits();
    // per-kernel HIP-event timing brackets every launch of a sampled iteration (two event records per kernel: ~25 us of queue bubbles per
    // iteration at small batches); OMC_TIMING_STRIDE=s samples every s-th iteration (averages per launch are over the sampled launches), 0 = none
    const bool sampled = tun.timing_stride > 0 && (it % tun.timing_stride) == 0;
    const bool use_graph = multi && nlist <= graph_max && !tun.no_graph && !(sampled && tun.timing_stride > 1) && !mw_any;      // hundreds of launches per call: eager
    if (book.running() > 0) {
      OmcWS wg = w; wg.slot_list = h->bslotlist.as<int>(); wg.nB = nlist; wg.mw_budget = mw_budget[0];
      if (multi && wait_main) { HIPCHK(hipStreamWaitEvent(sm, h->ev_main, 0)); tape.count_wait(); }
      if (wait_main) tape.touch(im);      // with one stream: what went onto it since the last iteration
      if (use_graph) {
        if (gexec_n != nlist) { int rc = capture_body(wg); if (rc) return rc; }
        HIPCHK(hipGraphLaunch(graphs.e[(!*is_check && w.accel) ? 1 : 0], sm));
        tape.touch(im);
        h->launches[OMC_KERNEL_GLOBAL] += 1; h->units[OMC_KERNEL_GLOBAL] += book.running();
      } else {
        if (quiet && split_solve && (it - 1) % check_every == 0) h->host_cnt[OMC_HOST_QUIET_INTERVALS] += 1;
        int rc = enqueue_body(wg, sampled, !*is_check && w.accel, false); if (rc) return rc;
      }
      // the check waits for the iteration: for the stop event of its last kernel when the tape has it
      if (multi && *is_check) { int rc = depend(im, T_S, -1, sampled && !use_graph && tun.event_merge, h->gev[3]); if (rc) return rc; }
    }
    h->host_cnt[OMC_HOST_BODY_RECORDS] += tape.records() - nrec0; h->host_cnt[OMC_HOST_BODY_WAITS] += tape.waits() - nwait0;
    wait_main = false;
    if (drain_pool >= 0) {      // the timing events of the interval before the last check, now that the device has the next iteration to run
      stamp_begin(); finish_events(drain_pool); drain_pool = -1; stamp(OMC_HOST_EVENT_DRAIN);
    }
    return 0;
  }

  // ---- a certificate check ------------------------------------------------------------------------------------------------------------
  void enqueue_check() {
    const int nactive = book.active();
    wait_main = true;
    tape.touch(T_S);
    timed_out = elapsed() > P.time_limit;
    TIMED(OMC_KERNEL_CHECK_COL, nactive, {
      if (shor) omc_shor_launch_check(&sw, s);      // primal value, constants and the dense multiplier of the Shor program
      else { omc_launch_check_zero(&w, s); omc_launch_colprox(&w, 1, s); }
    });
    TIMED(OMC_KERNEL_CHECK_BUILD, nactive, omc_launch_check_build(&w, s));
    TIMED(OMC_KERNEL_CHECK, nactive, {
      if (w.cert_enable) {        // estimate by the tracked block, decisions, rigorous evaluation of the slots that are about to finish
        omc_launch_cert_sub(&w, s);
        omc_launch_check_final(&w, timed_out ? OMC_ST_TIME : 0, 0, s);
        OmcWS wc = w; wc.ws_mode = 1; omc_launch_cone_ws(&wc, s);
        omc_launch_check_final(&w, timed_out ? OMC_ST_TIME : 0, 1, s);
      } else {
        if (w.geo.ws_lpp || w.geo.mw) { OmcWS wc = w; wc.ws_mode = 1; omc_launch_cone_ws(&wc, s); }
        else omc_launch_cone(&w, CONE_EVALS, s);
        omc_launch_check_final(&w, timed_out ? OMC_ST_TIME : 0, 2, s);      // per-slot iteration cap is applied on the device
      }
      if (shor && sw.cbGam) omc_shor_launch_cert_snapshot(&sw, s);      // Shor mode: blocks, paraboloid multipliers and points, ahead of the kernel that clears the flag
      if (w.cert_flag) omc_launch_cert_snapshot(&w, s);      // the multipliers of a bound that has just been taken, at the penalty it was computed with
      if (w.bump_max > 0) { if (shor) omc_shor_launch_rescale(&sw, s); omc_launch_rho_rescale(&w, s); }
      if (w.accel) omc_launch_aa(&w, s);      // after the certificate (computed on an image of the map), skips finished slots
    });
  }

  // statistics of the multi-workgroup eigen-kernels since the last call of this function -> totals and the next budgets
  int mw_collect() {
    if (!mw_any) return 0;
    std::vector<int> st(4 * (size_t)S);
    for (int v = 0; v < 2; ++v) {
      const OmcWS& wv = v ? h->wbig : w;
      if (!(v ? shor && wv.geo.mw : wv.geo.mw)) continue;
      HIPCHK(hipMemcpyAsync(st.data(), wv.mw_stat, sizeof(int) * st.size(), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      HIPCHK(hipMemsetAsync(wv.mw_stat, 0, sizeof(int) * st.size(), s));
      int mx = 0;
      for (int b = 0; b < S; ++b) { h->mw_tot[0] += st[4 * b]; h->mw_tot[2] += st[4 * b + 2]; mx = std::max(mx, st[4 * b + 3]); }
      if (mx) h->mw_tot[1] = mx;      // an interval without a call keeps the last figure
      h->mw_tot[3] = std::max<long long>(h->mw_tot[3], mx);
      mw_budget[v] = omc_cone_multi_budget(mx);
    }
    return 0;
  }

  // omc_last_cutoff_stats: the slots this check finished (done in the image that has just come back, not yet parked by the scan) whose status
  // is OMC_CUTOFF, and their iterations.  Only while a cutoff other than +inf has been given: without one no check copies anything more.
  int count_cutoffs() {
    cut_img.resize(2 * (size_t)S);
    HIPCHK(hipMemcpyAsync(cut_img.data(), w.status, sizeof(int) * S, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cut_img.data() + S, w.iters, sizeof(int) * S, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int b = 0; b < S; ++b)
      if (book.node(b) >= 0 && done[b] && !book.is_parked(b) && cut_img[b] == OMC_ST_CUTOFF) { h->cutoff_nodes.fetch_add(1); h->cutoff_iters.fetch_add(cut_img[S + b]); }
    return 0;
  }

  // the done flags (and the word of the quiet intervals) come back; the timing pools swap; Btot is re-read; first_wins is decided
  int read_check() {
    stamp_begin();
    const bool track_quiet = split_solve && tun.ws_quiet && w.ws_need;
    done[S] = 1;
    HIPCHK(hipMemcpyAsync(done, w.done, sizeof(int) * ((size_t)S + (track_quiet ? 1 : 0)), hipMemcpyDeviceToHost, s));      // with w.ws_need behind the flags
    if (track_quiet) HIPCHK(hipMemsetAsync(w.ws_need, 0, sizeof(int), s));      // ahead of everything the next interval runs
    HIPCHK(hipStreamSynchronize(s));
    stamp(OMC_HOST_CHECK_WAIT);
    quiet_next = track_quiet && done[S] == 0;
    t_check = t_last;
    nrefilled = 0; list_pushed = false;
    { int rc = mw_collect(); if (rc) return rc; }
    // every timed launch of the interval has joined s (the side streams join sm before k_global, sm joins s at a check) and so has completed:
    // its pool is read once the next iteration is enqueued; what is launched from here on records into the other pool, which is empty
    if (drain_pool >= 0) { finish_events(drain_pool); drain_pool = -1; }
    drain_pool = tape.current(); tape.swap();
    Btot = h->Btot_live.load();
    if (h->cutoff_armed.load()) { int rc = count_cutoffs(); if (rc) return rc; }
    if (!P.first_wins) return 0;
    // the first certified node ends the batch (penalty autotune): everything still running is harvested as it stands
    std::vector<int> stv(S);
    HIPCHK(hipMemcpyAsync(stv.data(), w.status, sizeof(int) * S, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    bool won = false;
    for (int b = 0; b < S; ++b) if (book.node(b) >= 0 && done[b] && stv[b] == OMC_ST_OPTIMAL) won = true;
    if (!won) return 0;
    book.finish_all();
    HIPCHK(hipMemcpyAsync(w.done, done, sizeof(int) * S, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return close_unslotted(OMC_ST_SLOW);
  }

  void enqueue_harvest(int nslots) {
    tape.touch(T_S);
    TIMED(OMC_KERNEL_HARVEST, nslots, {
      if (w.save_to) omc_launch_state_save(&w, s);                              // warm-start pool: before the recovery overwrites the iterate U = Q Vt
      if (shor) omc_shor_launch_state_save(&sw, s);                             // its Shor extension (no-op without indices)
      omc_launch_small(&w, SMALL_RECOVER, s);   // a U with U U' <= Y and the same Q'U
      if (w.sep_done) omc_launch_sep_sub(&w, s);                                // separation vector from the tracked block where there is one
      omc_launch_cone(&w, CONE_SEP, s);           // separation vector (OMC.jl:2466-2477)
      omc_launch_harvest(&w, s);
      if (w.cert_flag) omc_launch_cert_harvest(&w, s);
      if (shor && sw.cbGam) omc_shor_launch_cert_harvest(&sw, s);
      if (shor) omc_shor_launch_harvest(&sw, s);
    });
  }
  // the nodes of harvested_ids, once the stream has been synchronised behind their harvest kernels: the entries they saved to hold their state
  // from here on, and their results can be fetched
  void book_harvested() {
    if (w.save_to) {
      std::lock_guard<std::mutex> lk(h->sig_mu);
      for (int id : harvested_ids) {
        const int sv = (size_t)id < h->save_host.size() ? h->save_host[id] : -1;
        if (sv < 0 || (size_t)sv >= h->pool_sig.size()) continue;
        if (shor) { h->pool_sig[sv] = h->node_sig[id]; ++h->shor_warm_stats[3]; }
        else { h->pool_sig[sv] = omc_instance::PoolSig{}; h->pool_sig[sv].kind = 1; }
      }
    }
    std::lock_guard<std::mutex> lk(h->done_mu); h->done_q.insert(h->done_q.end(), harvested_ids.begin(), harvested_ids.end());
  }

  // An asynchronous harvest of the previous check: the wait of read_check was also the wait for its kernels (s is in order), so its nodes are
  // booked and its slots refilled now -- a node still starts at a check boundary, one interval later than after a synchronous harvest
  int book_async_harvest() {
    harvested += book.pending_harvests(); h->nodes_done.store(harvested);
    int rc = gram_jobs_free(); if (rc) return rc;
    nrefilled = book.book_async(Btot, timed_out, harvested_ids);
    book_harvested();
    stamp(OMC_HOST_HARVEST_BOOK);
    rc = gram_launch(nrefilled); if (rc) return rc;
    rc = push_flags(false); if (rc) return rc;      // the new nodes and their init flags; the fin flags of the harvest are cleared
    if (nrefilled) { rc = setup_slots(nrefilled); if (rc) return rc; }
    stamp(OMC_HOST_SETUP_ENQUEUE);
    return 0;
  }

  // The finished slots stay parked with their node until the next check books and refills them.  The slot list and the event the next
  // iteration waits for go ahead of the harvest kernels: nothing a live slot reads is written by them.
  int harvest_async() {
    const int npend = book.mark_async();
    int rc = push_list(); if (rc) return rc;
    list_pushed = true;
    stamp(OMC_HOST_LIST);
    if (multi) { HIPCHK(hipEventRecord(h->ev_main, s)); ev_main_set = true; tape.touch(T_S); }
    rc = push_flags(false); if (rc) return rc;
    stamp(OMC_HOST_HARVEST_FLAGS);
    enqueue_harvest(npend);
    stamp(OMC_HOST_HARVEST_ENQUEUE);
    h->host_cnt[OMC_HOST_ASYNC_HARVESTS] += 1;
    return 0;
  }

  // Harvest, wait, book and refill before the next iteration.  Which pending node goes to which finished slot is known before the harvest
  // kernels are enqueued, so the Gram matrices of the new nodes are formed beside them.
  int harvest_sync(int nfin) {
    int rc = gram_jobs_free(); if (rc) return rc;
    rc = gram_launch(book.mark_sync(Btot, timed_out)); if (rc) return rc;
    rc = push_flags(false); if (rc) return rc;
    stamp(OMC_HOST_HARVEST_FLAGS);
    enqueue_harvest(nfin);
    stamp(OMC_HOST_HARVEST_ENQUEUE);
    harvested += nfin; h->nodes_done.store(harvested);
    const int ninit = book.harvest_sync(Btot, timed_out, harvested_ids);
    rc = push_flags(true); if (rc) return rc;      // synchronises the stream: the harvest kernels have written the per-node outputs
    stamp(OMC_HOST_HARVEST_WAIT);
    book_harvested();
    stamp(OMC_HOST_HARVEST_BOOK);
    if (ninit) { rc = setup_slots(ninit); if (rc) return rc; }
    stamp(OMC_HOST_SETUP_ENQUEUE);
    return 0;
  }

  // the slot list if it changed, appended nodes for slots that had gone idle, the nodes the time limit leaves without a slot
  int finish_check(bool harvested_now, bool list_changed) {
    quiet = quiet_next;      // refill_idle below takes it back when it sets slots up
    book.recount();
    if (!list_pushed && list_changed) { int rc = push_list(); if (rc) return rc; stamp(OMC_HOST_LIST); }
    if (book.next_node() < Btot && !timed_out && book.active() < S) { int rc = refill_idle(); if (rc) return rc; }
    if (timed_out) { int rc = close_unslotted(OMC_ST_TIME); if (rc) return rc; }
    const int q = harvested_now ? OMC_HOST_HARVEST_TOTAL : OMC_HOST_CHECK_TOTAL;
    h->host_ms[q] += std::chrono::duration<double, std::milli>(Clock::now() - t_check).count(); h->host_cnt[q] += 1;
    return 0;
  }

  int collect_statistics() {
    { int rc = mw_collect(); if (rc) return rc; }
    if (w.geo.plain_mw && w.pmw_stat) {      // the separation launches of the harvests: the slots' counters since the batch was staged
      std::vector<int> st(4 * (size_t)S);
      HIPCHK(hipMemcpyAsync(st.data(), w.pmw_stat, sizeof(int) * st.size(), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      for (int b = 0; b < S; ++b) {
        h->pmw_tot[0] += st[4 * b]; h->pmw_tot[2] += st[4 * b + 2];
        h->pmw_tot[1] = std::max<long long>(h->pmw_tot[1], st[4 * b + 3]);
      }
    }
    std::vector<int> sweeps(S);
    HIPCHK(hipMemcpyAsync(sweeps.data(), w.sweeps, sizeof(int) * S, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int v : sweeps) h->total_sweeps += v;
    { int rc = sum_sub_stat(w.sub_stat, S, h->sub_tot, s); if (rc) return rc; }
    if (shor && h->wbig.sub_enable) { int rc = sum_sub_stat(h->wbig.sub_stat, S, h->big_sub_tot, s); if (rc) return rc; }      // the big cone's (same layout as omc_last_subspace_stats)
    HIPCHK(hipGetLastError());
    if (drain_pool >= 0) finish_events(drain_pool);      // the older pool first: the sums are formed in launch order
    finish_events(tape.current());
    h->last_solve_seconds = elapsed();
    h->last_iters_total = it;
    if (tun.host_phases) {
      static const char* const nm[OMC_HOST_NPHASE] = {"check_wait", "check_scan", "list", "event_drain", "harvest_flags", "harvest_enqueue", "harvest_wait", "harvest_book", "setup_enqueue", "check_total", "harvest_total", "async_harvests", "quiet_intervals", "body_records", "body_waits"};
      fprintf(stderr, "omc host phases (solve %.1f ms, %d iterations):", 1e3 * h->last_solve_seconds, it);
      for (int q = 0; q < OMC_HOST_NPHASE; ++q) fprintf(stderr, " %s %.3f ms / %lld", nm[q], h->host_ms[q], (long long)h->host_cnt[q]);
      fprintf(stderr, "\n");
    }
    return 0;
  }
};

}  // namespace

extern "C" {

// Sweep budget of the next multi-workgroup calls of a view (omc_relax_solve reads the counts at a certificate check).  interval_max: most
// sweeps of a call since the last check, 0 = no call in that interval.  Warm calls: what the last interval needed + 2.  After an interval
// without a call the next one is a fall-back from a basis that has gone stale by an unknown amount (on a warm-started solve not even the
// first calls were cold): the full bound -- the launches of the sweeps not needed leave at once.  Exported for the tests.
int omc_cone_multi_budget(int interval_max) { return interval_max > 0 ? std::min(MAX_SWEEPS, interval_max + 2) : MAX_SWEEPS; }

// The rule of omc_slots.h, exported for the tests.
int omc_harvest_plan(int nlive, int nfin, int pending, int check_index, int async_min_live) {
  return slot_harvest_plan(nlive, nfin, pending, check_index, async_min_live);
}

int omc_relax_solve(omc_instance* h) {
  if (!h || !h->staged) return fail(OMC_ERR_ARGUMENT, "omc_relax_solve: nothing staged");
  if (!h->ws.cutoff) return fail(OMC_ERR_ARGUMENT, "omc_relax_solve: the staged workspace has no cutoff pointer");      // k_check_final reads through it
  HIPCHK(hipSetDevice(h->device));
  if (!h->worker_running.load()) cutoff_solve_begin(h);      // a submitted solve began in omc_relax_submit
  SolveLoop L(h);
  int rc = L.prepare(); if (rc) return rc;
  for (;;) {
    if (L.book.active() == 0) {      // wait for appended nodes, or end
      bool ended = false;
      rc = L.run_dry(&ended); if (rc) return rc;
      if (ended) break;
      continue;
    }
    bool is_check = false;
    rc = L.enqueue_iteration(&is_check); if (rc) return rc;
    if (!is_check) continue;
    L.enqueue_check();
    rc = L.read_check(); if (rc) return rc;
    if (L.book.pending_harvests()) { rc = L.book_async_harvest(); if (rc) return rc; }
    // harvest finished slots, hand them the next pending nodes (when and how: SlotBook::check)
    const SlotBook::Check c = L.book.check(L.Btot, L.timed_out, L.multi, L.P.first_wins != 0, L.tun.harvest_async ? L.tun.harvest_async_min_live : 0);
    L.stamp(OMC_HOST_CHECK_SCAN);
    const int nfin = c.plan == OMC_HARVEST_NONE ? 0 : c.nfin;
    if (c.plan == OMC_HARVEST_ASYNC) rc = L.harvest_async();
    else if (nfin) rc = L.harvest_sync(nfin);
    if (rc) return rc;
    rc = L.finish_check(nfin != 0, nfin || c.nnew || L.nrefilled); if (rc) return rc;
  }
  return L.collect_statistics();
}

}  // extern "C"
