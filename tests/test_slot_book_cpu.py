"""CPU test of SlotBook (csrc/omc_slots.h), the slot bookkeeping of omc_relax_solve: tests/host/slot_book_check.cpp, a stand-alone program
that includes nothing of the project but that header, is compiled with the standard library's assertions on (every std::vector index is
bounds-checked) and fed seeded random scripts -- solves with 1 to 7 slots and up to 30 nodes, nodes appended mid-run, the time limit
striking at a random check, the asynchronous harvest at thresholds 0 to 3, one stream and several, first_wins.  Its output is compared
step by step with a model in Python that restates the rules, and the invariants of the bookkeeping are asserted on the way."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimalmatrixcompletion.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "slot_book_check.cpp")
NONE, SYNC, ASYNC = 0, 1, 2
NSCRIPTS = 3000


def fmt(name, v):
    return " %s=[%s]" % (name, ",".join(str(int(x)) for x in v))


class Model:
    """The rules, one method per step of a script; self.lines is what the program must print."""

    def __init__(self, S, Btot, async_min_live, multi, first_wins):
        self.S, self.aml, self.multi, self.first_wins = S, async_min_live, multi, first_wins
        self.node = [b if b < Btot else -1 for b in range(S)]
        self.done = [0 if b < Btot else 1 for b in range(S)]
        self.parked, self.inflight = [0] * S, [0] * S
        self.init = [1 if b < Btot else 0 for b in range(S)]
        self.fin = [0] * S
        self.next = min(S, Btot)
        self.npend = self.checks = 0
        self.harvested, self.closed = [], []
        self.recount()
        self.Btot = Btot
        self.lines = [self.dump("start", [(b, b) for b in range(self.next)])]

    def recount(self):
        self.nactive = sum(1 for b in range(self.S) if self.node[b] >= 0)
        self.gact = sum(1 for b in range(self.S) if self.node[b] >= 0 and not self.parked[b])

    def slot_list(self):
        return [b for b in range(self.S) if self.node[b] >= 0 and not self.parked[b]]

    def dump(self, tag, jobs=None, ids=None):
        for s, n in jobs or []:      # every job names a slot and a staged node
            assert 0 <= s < self.S and 0 <= n < self.Btot, (s, n, self.S, self.Btot)
        assert self.npend == sum(self.inflight)
        out = tag
        if jobs is not None:
            out += fmt("jobs", [x for j in jobs for x in j])
        if ids is not None:
            out += fmt("ids", ids)
        out += fmt("node_of", self.node) + fmt("parked", self.parked) + fmt("inflight", self.inflight) + fmt("done", self.done)
        out += fmt("flags", [max(v, 0) for v in self.node] + self.init + self.fin) + fmt("list", self.slot_list())
        return out + " next=%d npend=%d nactive=%d gact=%d" % (self.next, self.npend, self.nactive, self.gact)

    def take(self, b):
        self.node[b] = self.next
        self.next += 1
        self.init[b] = 1
        return (b, self.node[b])

    def close(self, Btot):
        self.closed += list(range(self.next, Btot))
        first, self.next = self.next, max(self.next, Btot)
        return "closed first=%d" % first

    def refill(self, Btot):
        self.init, self.fin = [0] * self.S, [0] * self.S
        jobs = []
        for b in range(self.S):
            if self.node[b] < 0 and self.next < Btot:
                jobs.append(self.take(b))
                self.parked[b] = 0
        if jobs:
            self.recount()
        return self.dump("refill", jobs)

    def idle(self, Btot, timed_out):
        self.Btot = Btot
        out = []
        if timed_out:
            out.append(self.close(Btot))
        if self.next < Btot:
            out.append(self.refill(Btot))
        self.lines += out

    def check(self, Btot, timed_out, won, bits):
        S, out = self.S, []
        self.Btot = Btot
        self.done = list(bits)
        if won:
            self.done = [1] * S
            out.append(self.close(Btot))
        if self.npend:                                   # the asynchronous harvest of the previous check is booked
            self.init, self.fin = [0] * S, [0] * S
            ids, jobs = [], []
            for b in range(S):
                if not self.inflight[b]:
                    continue
                self.inflight[b] = self.parked[b] = 0
                ids.append(self.node[b])
                if self.next < Btot and not timed_out:
                    jobs.append(self.take(b))
                    self.done[b] = 0
                else:
                    self.node[b] = -1
            self.npend = 0
            self.harvested += ids
            out.append(self.dump("book", jobs, ids))
        self.init, self.fin = [0] * S, [0] * S            # scan
        held = [b for b in range(S) if self.node[b] >= 0]
        finished = [b for b in held if self.done[b]]
        nfin, nlive = len(finished), len(held) - len(finished)
        nnew = sum(1 for b in finished if not self.parked[b])
        for b in finished:
            self.parked[b] = 1
        self.checks += 1                                  # plan
        pending = self.next < Btot
        if nfin == 0:
            plan = NONE
        elif nlive == 0:
            plan = SYNC
        elif not ((self.checks % 3 == 0 or nlive < 256) if pending else self.checks % 12 == 0):
            plan = NONE
        else:
            plan = ASYNC if self.aml > 0 and nlive >= self.aml else SYNC
        if plan == ASYNC and (not self.multi or timed_out or self.first_wins or (pending and nfin + nlive < S)):
            plan = SYNC
        out.append("check plan=%d nfin=%d nlive=%d nnew=%d" % (plan, nfin, nlive, nnew))
        if plan == ASYNC:
            for b in finished:
                self.fin[b] = self.inflight[b] = 1
            self.npend = len(finished)
            self.recount()
            out.append("async n=%d" % self.npend)
        elif plan == SYNC:
            for b in finished:
                self.fin[b], self.parked[b] = 1, 0
            preview = [] if timed_out else list(zip(finished, range(self.next, Btot)))
            out.append(self.dump("mark", preview))
            ids, ninit = [], 0
            for b in finished:
                self.fin[b] = 0
                ids.append(self.node[b])
                if self.next < Btot and not timed_out:
                    assert self.take(b) == preview[ninit]      # the gram jobs did preview the assignment
                    ninit += 1
                else:
                    self.node[b] = -1
            self.harvested += ids
            out.append("harvest ninit=%d" % ninit)
            out.append(self.dump("harvested", None, ids))
        self.recount()
        if self.next < Btot and not timed_out and self.nactive < S:
            out.append(self.refill(Btot))
        if timed_out:
            out.append(self.close(Btot))
        out.append(self.dump("end"))
        self.lines += out


def make_script(rng):
    """One solve: the script for the program and the model that has run it."""
    S = rng.choice([1, 2, 3, 4, 7])
    N = rng.randint(1, 30)                                # nodes in the end, unless the time limit or a won race closes some
    Btot = rng.randint(1, N)
    first_wins = int(rng.random() < 0.15)
    head = (S, Btot, rng.choice([0, 1, 2, 3]), rng.randint(0, 1), first_wins)
    m = Model(*head)
    script = ["%d %d %d %d %d" % head]
    limit_at = rng.randint(1, 25) if rng.random() < 0.3 else None      # the check at which the time limit strikes
    p_done, p_append = rng.choice([0.1, 0.3, 0.6]), rng.choice([0.0, 0.2, 0.5])
    timed_out = False
    for _ in range(2000):
        if Btot < N and rng.random() < p_append:
            Btot = rng.randint(Btot + 1, N)
        if m.nactive == 0:
            script.append("I %d %d" % (Btot, timed_out))
            m.idle(Btot, timed_out)
            if m.nactive == 0 and m.next >= Btot:
                if Btot < N and rng.random() < 0.7:       # held open: more nodes arrive
                    continue
                break
            continue
        timed_out = timed_out or (limit_at is not None and m.checks + 1 >= limit_at)
        bits = [1 if (m.node[b] < 0 or m.parked[b] or timed_out or rng.random() < p_done) else 0 for b in range(S)]
        won = int(first_wins and rng.random() < 0.3 and any(bits[b] and m.node[b] >= 0 for b in range(S)))
        script.append("C %d %d %d %s" % (Btot, timed_out, won, " ".join(map(str, bits))))
        m.check(Btot, timed_out, won, bits)
    else:
        raise AssertionError("the script does not end")
    script.append("E")
    m.lines.append("E")
    return script, m


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slot_book") / "slot_book_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


def test_header_is_plain_cpp():
    """omc_slots.h includes <vector> and <algorithm> and nothing else: no HIP header, nothing of the project."""
    import re
    inc = re.findall(r"^\s*#\s*include\s*(\S+)", open(os.path.join(CSRC, "omc_slots.h")).read(), flags=re.M)
    assert sorted(inc) == ["<algorithm>", "<vector>"]


def test_random_scripts_against_the_model(program):
    rng = random.Random(20250117)
    runs = [make_script(rng) for _ in range(NSCRIPTS)]
    text = "\n".join(line for script, _ in runs for line in script) + "\n"
    got = subprocess.run([program], input=text, capture_output=True, text=True, check=True, timeout=120).stdout.split("\n")
    want = [line for _, m in runs for line in m.lines]
    assert len(got) == len(want) + 1 and got[-1] == ""
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    seen = {"async": 0, "appended": 0, "timed": 0, "won": 0, "idle_refill": 0}
    for script, m in runs:
        # every node is harvested exactly once or closed without a slot; nothing is left in flight, in a slot or pending
        assert sorted(m.harvested + m.closed) == list(range(m.Btot)), script
        assert not any(m.inflight) and m.npend == 0 and m.nactive == 0 and m.next == m.Btot
        seen["async"] += any(l.startswith("async") for l in m.lines)
        seen["appended"] += m.Btot > int(script[0].split()[1])
        seen["timed"] += any(l.startswith("C") and l.split()[2] == "1" for l in script)
        seen["won"] += any(l.startswith("C") and l.split()[3] == "1" for l in script)
        seen["idle_refill"] += any(l.startswith("refill") for l in m.lines)
    print(seen)
    assert all(v >= 50 for v in seen.values()), seen      # the scripts do reach every path
