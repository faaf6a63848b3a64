// event_tape_check.cpp -- drives EventTape (csrc/omc_events.h) from a script on stdin with a backend that writes down what it is asked to do
// (tests/test_event_tape_cpu.py compares the output with a model and checks the invariants on it).  Includes nothing of the project but
// that header.
//
//   N <nstreams> <merge>   a new tape            T <s>   touch             K <s> <id>   a kernel goes onto stream s (touch)
//   B <s> / E <s> / M <s>  begin / end / mark: the result goes to the next register and is printed ("= pool index", "= -")
//   W <s> <reg>            stream s waits for the event in a register      L <r0> <r1> <cls>   launch(start, stop, class)
//   G <s> <g> / V <s> <g>  an event that is not the tape's is recorded on / waited for by stream s (touch, counted)
//   X <n>                  the backend refuses its next n records          S   swap      D <pool>   print and drain      C   counts
//   # ...                  echoed
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "omc_events.h"

struct Log {
  int refuse = 0;
  bool record(int pool, int index, int stream) {
    if (refuse > 0) { --refuse; printf("refused %d %d %d\n", pool, index, stream); return false; }
    printf("R %d %d %d\n", pool, index, stream);
    return true;
  }
  bool wait(int stream, int pool, int index) { printf("W %d %d %d\n", stream, pool, index); return true; }
};
using Tape = EventTape<Log>;

int main() {
  Log log;
  std::vector<Tape> tapes;      // the last one is driven
  std::vector<Tape::Ev> reg;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    if (line[0] == '#') { printf("%s\n", line.c_str()); continue; }
    std::istringstream in(line);
    char op = 0; int a = 0, b = 0, c = 0;
    in >> op >> a >> b >> c;
    if (op == 'N') { tapes.clear(); tapes.emplace_back(&log, a, b != 0); reg.clear(); log.refuse = 0; printf("N %d %d\n", a, b); continue; }
    if (tapes.empty()) { fprintf(stderr, "no tape\n"); return 2; }
    Tape& t = tapes.back();
    switch (op) {
      case 'T': t.touch(a); break;
      case 'K': t.touch(a); printf("K %d %d\n", a, b); break;
      case 'B': case 'E': case 'M': {
        const Tape::Ev e = op == 'B' ? t.begin(a) : op == 'E' ? t.end(a) : t.mark(a);
        reg.push_back(e);
        if (e.valid()) printf("= %d %d\n", e.pool, e.index); else printf("= -\n");
        break;
      }
      case 'W': if (!t.wait(a, reg.at(b))) return 3; break;
      case 'L': t.launch(reg.at(a), reg.at(b), c); break;
      case 'G': t.touch(a); t.count_record(); printf("G %d %d\n", a, b); break;
      case 'V': t.touch(a); t.count_wait(); printf("V %d %d\n", a, b); break;
      case 'X': log.refuse = a; break;
      case 'S': t.swap(); printf("S %d\n", t.current()); break;
      case 'D': {
        printf("D %d", a);
        for (const Tape::Launch& l : t.launches(a)) printf(" %d:%d:%d", l.start, l.stop, l.cls);
        printf("\n");
        t.drain(a);
        break;
      }
      case 'C': printf("C %lld %lld\n", t.records(), t.waits()); break;
      default: fprintf(stderr, "bad op %c\n", op); return 2;
    }
  }
  return 0;
}
