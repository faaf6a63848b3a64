// slot_book_check.cpp -- drives SlotBook (csrc/omc_slots.h) from scripts on stdin, in the order in which omc_relax_solve calls it, and prints
// what every operation returned and left behind (tests/test_slot_book_cpu.py compares the output with a model of the rules).
//
// A script:   S Btot async_min_live multi first_wins            the solve starts with Btot nodes staged
//             C Btot timed_out won d_0 ... d_{S-1}              a check: the Btot it sees, the done flags read back from the device
//             I Btot timed_out                                  no slot holds a node: the loop looks for appended nodes
//             E                                                 end of the script (another may follow)
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "omc_slots.h"

static void put(const char* name, const int* v, int n) {
  printf(" %s=[", name);
  for (int i = 0; i < n; ++i) printf(i ? ",%d" : "%d", v[i]);
  printf("]");
}

struct Run {
  int S;
  std::vector<int> jobs, done, flags, list;
  SlotBook book;
  explicit Run(int S_) : S(S_), jobs(2 * (size_t)S_, -7), done(S_, 0), flags(3 * (size_t)S_, -7), list(S_, -7), book(S_, jobs.data(), done.data()) {}
  void dump(const char* tag, int njobs, const std::vector<int>* ids) {
    printf("%s", tag);
    if (njobs >= 0) put("jobs", jobs.data(), 2 * njobs);
    if (ids) put("ids", ids->data(), (int)ids->size());
    std::vector<int> node(S), parked(S), inflight(S);
    for (int b = 0; b < S; ++b) { node[b] = book.node(b); parked[b] = book.is_parked(b); inflight[b] = book.is_inflight(b); }
    put("node_of", node.data(), S); put("parked", parked.data(), S); put("inflight", inflight.data(), S); put("done", done.data(), S);
    book.write_flags(flags.data());
    put("flags", flags.data(), 3 * S);
    put("list", list.data(), book.write_list(list.data()));
    printf(" next=%d npend=%d nactive=%d gact=%d\n", book.next_node(), book.pending_harvests(), book.active(), book.running());
  }
};

int main() {
  int S, Btot, async_min_live, multi, first_wins;
  while (std::cin >> S >> Btot >> async_min_live >> multi >> first_wins) {
    Run r(S);
    std::vector<int> ids;
    r.dump("start", r.book.start(Btot), nullptr);
    std::string op;
    while (std::cin >> op && op != "E") {
      int timed_out = 0;
      std::cin >> Btot >> timed_out;
      if (op == "I") {
        if (timed_out) printf("closed first=%d\n", r.book.close_unslotted(Btot));
        if (r.book.next_node() < Btot) r.dump("refill", r.book.refill_idle(Btot), nullptr);
        continue;
      }
      int won = 0;
      std::cin >> won;
      for (int b = 0; b < S; ++b) std::cin >> r.done[b];
      if (won) { r.book.finish_all(); printf("closed first=%d\n", r.book.close_unslotted(Btot)); }
      if (r.book.pending_harvests()) r.dump("book", r.book.book_async(Btot, timed_out != 0, ids), &ids);
      const SlotBook::Check c = r.book.check(Btot, timed_out != 0, multi != 0, first_wins != 0, async_min_live);
      printf("check plan=%d nfin=%d nlive=%d nnew=%d\n", c.plan, c.nfin, c.nlive, c.nnew);
      if (c.plan == SLOT_HARVEST_ASYNC) { const int n = r.book.mark_async(); printf("async n=%d\n", n); }
      else if (c.plan == SLOT_HARVEST_SYNC) {
        r.dump("mark", r.book.mark_sync(Btot, timed_out != 0), nullptr);
        const int ninit = r.book.harvest_sync(Btot, timed_out != 0, ids);
        printf("harvest ninit=%d\n", ninit);
        r.dump("harvested", -1, &ids);
      }
      r.book.recount();
      if (r.book.next_node() < Btot && !timed_out && r.book.active() < S) r.dump("refill", r.book.refill_idle(Btot), nullptr);
      if (timed_out) printf("closed first=%d\n", r.book.close_unslotted(Btot));
      r.dump("end", -1, nullptr);
    }
    printf("E\n");
  }
  return 0;
}
