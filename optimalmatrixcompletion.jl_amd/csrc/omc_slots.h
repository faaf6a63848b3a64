// omc_slots.h -- slot bookkeeping of omc_relax_solve (omc_relax_solve.cpp): which node each slot holds, which slots are parked or in flight,
// the next pending node, and the host images the device reads (job list, slot flags, slot list, done flags).  Plain C++17: no HIP header, no
// device call, no knowledge of streams.  Every operation returns what the driver has to enqueue for it (counts, harvested node ids, the plan),
// so the rules can be read and run on their own (tests/host/slot_book_check.cpp).
#pragma once
#include <algorithm>
#include <vector>

enum { SLOT_HARVEST_NONE = 0, SLOT_HARVEST_SYNC = 1, SLOT_HARVEST_ASYNC = 2 };      // OMC_HARVEST_* of omc.h

static constexpr int REFILL_EVERY = 3;               // finished slots are harvested and refilled at every third check
static constexpr int REFILL_AT_ONCE_LIVE = 256;      // fewer live slots than this no longer fill the chip: harvest and refill at every check

// Harvest and refill every REFILL_EVERY-th check only (or when nothing is left running): a refilled slot spends its first dozen
// iterations in the full eigendecomposition, the straggler of every launch it is part of, and each harvest is 1 - 3 ms of few-workgroup
// kernels on the main stream -- batching them halves the launches that carry young slots.  A finished slot waits (done = 1, skipped
// by every kernel and left out of the slot list) for at most REFILL_EVERY - 1 check intervals.
// With pending nodes: every REFILL_EVERY-th check, at once when the live slots no longer fill the chip; without: the finished slots can
// wait longer (nothing to hand them), until nothing runs any more.
// Nothing a live slot reads is written by the harvest kernels, so with enough live slots to fill the chip they run beside the next interval
// (ASYNC) and the host books and refills at the next check; below that, refilling at once is worth more than the stall.
inline int slot_harvest_plan(int nlive, int nfin, int pending, int check_index, int async_min_live) {
  if (nfin <= 0) return SLOT_HARVEST_NONE;
  if (nlive <= 0) return SLOT_HARVEST_SYNC;
  const bool now = pending ? (check_index % REFILL_EVERY == 0 || nlive < REFILL_AT_ONCE_LIVE) : (check_index % (4 * REFILL_EVERY) == 0);
  if (!now) return SLOT_HARVEST_NONE;
  return (async_min_live > 0 && nlive >= async_min_live) ? SLOT_HARVEST_ASYNC : SLOT_HARVEST_SYNC;
}

class SlotBook {
 public:
  struct Check { int plan, nfin, nlive, nnew; };      // nfin: finished slots, those parked at earlier checks included; nnew: parked at this one

  // jobs: 2 S ints, the (slot, node) pairs of k_setup_gram; done: S ints, the image of the device's done flags (read back at every check)
  SlotBook(int S_, int* jobs_, int* done_) : S(S_), node_of(S_, -1), parked(S_, 0), inflight(S_, 0), init(S_, 0), fin(S_, 0), jobs(jobs_), done(done_) {}

  int slots() const { return S; }
  int next_node() const { return next; }
  int pending_harvests() const { return npend; }      // slots of an asynchronous harvest that the next check books
  int active() const { return nactive; }              // slots that hold a node
  int running() const { return gact; }                // of those, not parked: the units of an iteration's launches
  int node(int b) const { return node_of[b]; }        // -1 = idle
  bool is_parked(int b) const { return parked[b] != 0; }
  bool is_inflight(int b) const { return inflight[b] != 0; }

  // Slot b < min(S, Btot) holds node b and is set up; the others start idle (done = 1: skipped by every kernel).  Returns the jobs.
  int start(int Btot) {
    next = std::min(S, Btot); npend = 0; check_index = 0;
    for (int b = 0; b < S; ++b) {
      node_of[b] = b < Btot ? b : -1; parked[b] = 0; inflight[b] = 0; fin[b] = 0;
      init[b] = node_of[b] >= 0 ? 1 : 0; done[b] = node_of[b] >= 0 ? 0 : 1;
      if (node_of[b] >= 0) { jobs[2 * b] = b; jobs[2 * b + 1] = b; }
    }
    recount();
    return next;
  }

  // The asynchronous harvest of the previous check (pending_harvests() > 0), now that its kernels have completed: the in-flight slots give
  // up their nodes (ids, ascending slots) and take the next pending ones, or go idle.  A slot refilled here is live in the scan of the same
  // check (its done flag is cleared in the image).  Returns the slots refilled = the jobs.
  int book_async(int Btot, bool timed_out, std::vector<int>& ids) {
    clear_flags(); ids.clear();
    int nj = 0;
    for (int b = 0; b < S; ++b) {
      if (!inflight[b]) continue;
      inflight[b] = 0; parked[b] = 0;
      ids.push_back(node_of[b]);
      if (next < Btot && !timed_out) { take(b, nj++); done[b] = 0; }
      else node_of[b] = -1;
    }
    npend = 0;
    return nj;
  }

  // The scan of a check and what to do with the finished slots: slot_harvest_plan, with ASYNC taken back to SYNC where the stall buys
  // something or the end of the batch is near -- one stream, the time limit, first_wins, and idle slots that pending nodes are about to take
  // (refill_idle sets them up on the main stream, which the next iteration then waits for).
  Check check(int Btot, bool timed_out, bool multi, bool first_wins, int async_min_live) {
    clear_flags();
    Check c{SLOT_HARVEST_NONE, 0, 0, 0};
    for (int b = 0; b < S; ++b) {
      if (node_of[b] < 0) continue;
      if (done[b]) { ++c.nfin; if (!parked[b]) { parked[b] = 1; ++c.nnew; } } else ++c.nlive;
    }
    ++check_index;
    c.plan = slot_harvest_plan(c.nlive, c.nfin, next < Btot ? 1 : 0, check_index, async_min_live);
    if (c.plan == SLOT_HARVEST_ASYNC && (!multi || timed_out || first_wins || (next < Btot && c.nfin + c.nlive < S))) c.plan = SLOT_HARVEST_SYNC;
    return c;
  }

  // ASYNC: the finished slots get their fin flag and are in flight; they stay parked with their node (out of the slot list, done on the
  // device) until the next check books them.  Returns their count.
  int mark_async() {
    for (int b = 0; b < S; ++b) if (node_of[b] >= 0 && done[b]) { fin[b] = 1; inflight[b] = 1; ++npend; }
    recount();
    return npend;
  }

  // SYNC, before the harvest kernels: the finished slots get their fin flag and leave the parked set; the jobs preview the assignment that
  // harvest_sync makes (ascending finished slots take ascending pending nodes; none after the time limit).  Returns the jobs.
  int mark_sync(int Btot, bool timed_out) {
    for (int b = 0; b < S; ++b) if (node_of[b] >= 0 && done[b]) { fin[b] = 1; parked[b] = 0; }
    int nj = 0;
    if (!timed_out) for (int b = 0, nx = next; b < S && nx < Btot; ++b) if (fin[b]) { jobs[2 * nj] = b; jobs[2 * nj + 1] = nx++; ++nj; }
    return nj;
  }

  // SYNC, once the harvest kernels are enqueued: the marked slots give up their nodes (ids, ascending slots) and take the next pending
  // ones, or go idle.  Returns the slots refilled.
  int harvest_sync(int Btot, bool timed_out, std::vector<int>& ids) {
    ids.clear();
    int ninit = 0;
    for (int b = 0; b < S; ++b) {
      if (!fin[b]) continue;
      fin[b] = 0;
      ids.push_back(node_of[b]);
      if (next < Btot && !timed_out) { node_of[b] = next++; init[b] = 1; ++ninit; }
      else node_of[b] = -1;
    }
    return ninit;
  }

  // Pending nodes for idle slots (nodes appended while slots were idle), ascending.  Returns the slots set up = the jobs.
  int refill_idle(int Btot) {
    clear_flags();
    int nj = 0;
    for (int b = 0; b < S && next < Btot; ++b) if (node_of[b] < 0) { take(b, nj++); parked[b] = 0; }
    if (nj) recount();
    return nj;
  }

  // The nodes [next, Btot) never get a slot (time limit, first_wins won) and never enter the queue of harvested nodes.  Returns the first.
  int close_unslotted(int Btot) { const int first = next; next = std::max(next, Btot); return first; }

  void finish_all() { for (int b = 0; b < S; ++b) done[b] = 1; }      // first_wins won: everything still running is harvested as it stands

  void recount() {
    nactive = 0; gact = 0;
    for (int b = 0; b < S; ++b) if (node_of[b] >= 0) { ++nactive; if (!parked[b]) ++gact; }
  }

  // image: 3 S ints -- node of each slot (0 for an idle one), init flags, fin flags
  void write_flags(int* image) const {
    for (int b = 0; b < S; ++b) { image[b] = node_of[b] < 0 ? 0 : node_of[b]; image[S + b] = init[b]; image[2 * (size_t)S + b] = fin[b]; }
  }
  // list: S ints -- the slots that hold a node and are not parked, ascending.  Returns their count.
  int write_list(int* list) const {
    int nl = 0;
    for (int b = 0; b < S; ++b) if (node_of[b] >= 0 && !parked[b]) list[nl++] = b;
    return nl;
  }

 private:
  void clear_flags() { std::fill(init.begin(), init.end(), 0); std::fill(fin.begin(), fin.end(), 0); }
  void take(int b, int job) { jobs[2 * job] = b; jobs[2 * job + 1] = next; node_of[b] = next++; init[b] = 1; }      // slot b takes the next pending node

  int S, next = 0, npend = 0, check_index = 0, nactive = 0, gact = 0;
  std::vector<int> node_of;                 // node of each slot, -1 = idle
  std::vector<char> parked, inflight;       // finished and waiting for a harvest; of those, being harvested beside the running interval
  std::vector<int> init, fin;               // flags of the next write_flags
  int* jobs; int* done;
};
