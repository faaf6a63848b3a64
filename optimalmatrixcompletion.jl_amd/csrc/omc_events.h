// omc_events.h -- EventTape: which event records the solve loop (omc_relax_solve.cpp) enqueues for its per-launch timing and for the forks
// and joins of its streams.  Plain C++17: no HIP header.  The tape knows streams and events as small integers; a backend turns them into
// runtime calls, so the rules can be read and run on their own with a backend that only writes down what it is asked to do
// (tests/host/event_tape_check.cpp).
//
// A launch is timed by two events on its stream, one recorded directly in front of it and one directly behind it; a fork or a join is an
// event recorded on one stream that another stream waits for.  Many of these mark the same point of the same stream: the stop of a kernel is
// the start of the next one behind it, and the point a join waits for.  An event is *adjacent* on its stream while nothing has been enqueued
// there since its record; the tape remembers the adjacent event per stream and hands it out again instead of recording another one.
//
// Backend:  bool record(int pool, int index, int stream)   record event `index` of pool `pool` on `stream`; false: no such event could be
//                                                           made or the record failed (nothing has been enqueued)
//           bool wait(int stream, int pool, int index)     `stream` waits for that event as recorded last
//
// Events come from two pools that swap at a certificate check (swap): the launches of an interval record into the current pool, and the pool
// of the interval before is read (launches) and emptied (drain) once every launch in it has completed.  An event is handed out once per
// generation of its pool -- between two drains -- and a pool is drained only after the check that follows its interval: every wait that
// names one of its events was enqueued in that interval, long before the event is recorded again.
#pragma once
#include <vector>

template <class Backend>
class EventTape {
 public:
  struct Ev { int pool = -1, index = -1; bool valid() const { return index >= 0; } };
  struct Launch { int start, stop, cls; };      // indices into the pool the launch was recorded in

  // merge = false: every begin, end and mark records an event of its own (the order without the tape's savings)
  EventTape(Backend* be_, int nstreams, bool merge_) : be(be_), merge(merge_), adj(nstreams, -1) {}

  // something that is not one of the tape's records has been put on the stream: a launch, a wait, a copy, a fill, a foreign event
  void touch(int stream) { adj[stream] = -1; }

  // an event that marks the present end of the stream's queue: the adjacent one, else the next pool event, recorded now
  Ev mark(int stream) {
    if (merge && adj[stream] >= 0) return Ev{cur, adj[stream]};
    return fresh(stream);
  }
  Ev begin(int stream) { return mark(stream); }      // start event of the launch that is enqueued next on the stream
  Ev end(int stream) { return fresh(stream); }       // stop event of the launch that has just been enqueued: always a record of its own

  // `stream` waits for `e` (recorded on another stream)
  bool wait(int stream, Ev e) {
    const bool ok = be->wait(stream, e.pool, e.index);
    if (ok) { touch(stream); ++nwaits; }
    return ok;
  }

  void launch(Ev start, Ev stop, int cls) { timed[cur].push_back(Launch{start.index, stop.index, cls}); }

  int current() const { return cur; }
  // the check: what follows records into the other pool, which must have been drained; no event of the old pool starts a launch of the new one
  void swap() { cur ^= 1; for (int& a : adj) a = -1; }
  const std::vector<Launch>& launches(int pool) const { return timed[pool]; }
  void drain(int pool) { timed[pool].clear(); used[pool] = 0; if (pool == cur) for (int& a : adj) a = -1; }
  void reset() { drain(0); drain(1); cur = 0; nrecords = nwaits = 0; }

  long long records() const { return nrecords; }      // since reset, through the tape
  long long waits() const { return nwaits; }
  void count_record() { ++nrecords; }                 // a record / wait the driver enqueued past the tape (its fork and join events)
  void count_wait() { ++nwaits; }

 private:
  Ev fresh(int stream) {
    const int i = used[cur];
    if (!be->record(cur, i, stream)) return Ev{};
    used[cur] = i + 1; ++nrecords;
    adj[stream] = i;
    return Ev{cur, i};
  }

  Backend* be;
  bool merge;
  int cur = 0;
  int used[2] = {0, 0};
  std::vector<int> adj;      // per stream: index (current pool) of the event still adjacent, -1: none
  std::vector<Launch> timed[2];
  long long nrecords = 0, nwaits = 0;
};
