"""CPU test of EventTape (csrc/omc_events.h), which decides the event records of the solve loop: tests/host/event_tape_check.cpp, a
stand-alone program that includes nothing of the project but that header, is compiled with the standard library's assertions on and driven
with a backend that writes down every record and wait.  The scripts are every shape of an iteration body (quiet and split, one and three
streams, with and without k_aa, check and non-check, with and without the wait for the main stream, Shor and base, merged and not, timed
and not) in sequences with checks between them, and seeded random sequences of touch / begin / end / mark / wait / swap / drain with
refused records.  The output is compared line by line with the model of tests/event_tape_model.py, and the invariants are checked on the
program's own output:
  - a launch's start event is recorded on the launch's stream with nothing but event records between it and the kernel, after the last wait
    or kernel enqueued there before; its stop event is the first thing enqueued behind the kernel;
  - a wait names an event recorded earlier in program order, on another stream;
  - no event is recorded twice between two drains of its pool;
  - the records per iteration: 8 quiet and 10 split for the base body on three streams, against 13 and 16 unmerged."""
import itertools
import os
import random
import re
import subprocess

import pytest

from event_tape_model import Drive, S_MAIN, solve_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimalmatrixcompletion.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "event_tape_check.cpp")
NRANDOM = 3000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("event_tape") / "event_tape_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


def run(program, drives):
    text = "\n".join(line for d in drives for line in d.script) + "\n"
    got = subprocess.run([program], input=text, capture_output=True, text=True, check=True, timeout=120).stdout.split("\n")
    want = [line for d in drives for line in d.want]
    assert len(got) == len(want) + 1 and got[-1] == ""
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    return got[:-1]


def check_log(script, log):
    """The invariants, on what the program printed for one tape (`log`) and the launches the script declared."""
    queue = {}                     # stream -> what was enqueued there, in order
    recorded = {}                  # (pool, index) -> (stream, position in that stream's queue): the last record of the generation
    results = []                   # the events begin / end / mark returned, in register order
    nrec = nwait = 0
    for line in log:
        f = line.split()
        if f[0] == "R":
            pool, idx, s = int(f[1]), int(f[2]), int(f[3])
            assert (pool, idx) not in recorded, ("recorded twice in a generation", line)
            q = queue.setdefault(s, [])
            recorded[(pool, idx)] = (s, len(q))
            q.append(("R", (pool, idx)))
            nrec += 1
        elif f[0] == "W":
            s, ev = int(f[1]), (int(f[2]), int(f[3]))
            assert ev in recorded and recorded[ev][0] != s, ("wait for an event not recorded before, or on the waiting stream", line)
            queue.setdefault(s, []).append(("W", ev))
            nwait += 1
        elif f[0] == "K":
            queue.setdefault(int(f[1]), []).append(("K", int(f[2])))
        elif f[0] in "GV":
            queue.setdefault(int(f[1]), []).append((f[0], int(f[2])))
            nrec += f[0] == "G"
            nwait += f[0] == "V"
        elif f[0] == "=":
            results.append(None if f[1] == "-" else (int(f[1]), int(f[2])))
        elif f[0] == "D":
            for ev in [e for e in recorded if e[0] == int(f[1])]:
                del recorded[ev]
        elif f[0] == "C":
            assert (nrec, nwait) == (int(f[1]), int(f[2]))
    # the launches: "L r0 r1 cls" follows the "K s id" of its kernel in the script
    kernel = None
    where = {}
    for s, q in queue.items():
        for pos, item in enumerate(q):
            if item[0] == "K":
                where[item[1]] = (s, pos)
    nlaunch = 0
    for line in script:
        f = line.split()
        if f[0] == "K":
            kernel = int(f[2])
        elif f[0] == "L":
            start, stop = results[int(f[1])], results[int(f[2])]
            s, pos = where[kernel]
            q = queue[s]
            assert q[pos + 1] == ("R", stop), (line, q[pos - 3:pos + 2])
            back = pos - 1
            while q[back] != ("R", start):
                assert q[back][0] == "R", ("something but records between a start event and its kernel", line, q[back])
                back -= 1
                assert back >= 0
            nlaunch += 1
    return nlaunch


def split_tapes(drives, log):
    out, i = [], 0
    for d in drives:
        out.append(log[i:i + len(d.want)])
        i += len(d.want)
    return out


def test_header_is_plain_cpp():
    inc = re.findall(r"^\s*#\s*include\s*(\S+)", open(os.path.join(CSRC, "omc_events.h")).read(), flags=re.M)
    assert inc == ["<vector>"]


SHAPES = [dict(multi=m, split=sp, shor=sh, with_aa=aa, sub=sub, big_sub=bs)
          for m, sp, sh, aa, sub, bs in itertools.product((True, False), (False, True), (False, True), (False, True), (True, False), (True, False))
          if not (sp and (sh or not m)) and not (sh and aa) and (sh or bs)]


def body_sequence(merge, shape, stride):
    """Three intervals of four iterations of one shape with checks (the second with a harvest) between them."""
    d = Drive(4, merge)
    per_iter = []
    it = 0
    for interval in range(3):
        for q in range(4):
            it += 1
            d.note("iteration %d" % it)
            per_iter.append(d.iteration(timed=stride > 0 and it % stride == 0, is_check=q == 3, wait_main=q == 0, **dict(shape, with_aa=shape["with_aa"] and q != 3)))
        d.note("check")
        d.check(harvest=interval == 1)
    d.drain(d.cur ^ 1)
    d.drain(d.cur)
    d.counts()
    return d, per_iter


def test_every_body_shape(program):
    drives, meta = [], []
    for shape in SHAPES:
        for merge in (True, False):
            for stride in (1, 2, 0):
                d, per_iter = body_sequence(merge, shape, stride)
                drives.append(d)
                meta.append((shape, merge, stride, per_iter))
    logs = split_tapes(drives, run(program, drives))
    for d, log, (shape, merge, stride, per_iter) in zip(drives, logs, meta):
        nlaunch = check_log(d.script, log)
        nk = sum(1 for line in d.script if line.startswith("K"))
        assert stride != 1 or nlaunch == nk      # every kernel of a timed solve is a launch with both events
        if stride == 1:
            # a steady iteration (not the first of its interval, not the check): its launches, and in the unmerged order 2 records each + fork + joins
            kernels = sum(1 for line in d.script[:d.script.index("# iteration 2")] if line.startswith("K"))
            extra = (3 + shape["split"]) if shape["multi"] else 0
            steady = per_iter[1][0]
            if not merge:
                assert steady == 2 * kernels + extra
            else:
                # one record per kernel (its stop; its start is the stop in front of it) + one per stream whose first launch follows a wait:
                # both side streams and, behind the joins, the main stream; split: the main stream once more behind the wait for phase 1
                assert steady == kernels + ((3 + shape["split"]) if shape["multi"] else 0)
                assert per_iter[0][0] == steady + 1      # the fork finds no adjacent event behind the wait for the main stream
                assert per_iter[3][0] == steady - (1 if shape["with_aa"] else 0)      # the check's wait takes the stop event of the last kernel; no k_aa at a check
            assert per_iter[1][1] == ((4 + shape["split"]) if shape["multi"] else 0)


def test_record_counts_of_the_base_body(program):
    """8 and 10 records per iteration against 13 and 16 (three streams, k_cone_sub on, no k_aa)."""
    for split, merged, plain in ((False, 8, 13), (True, 10, 16)):
        for merge, n in ((True, merged), (False, plain)):
            d, per_iter = body_sequence(merge, dict(multi=True, split=split, shor=False, with_aa=False, sub=True, big_sub=True), 1)
            assert per_iter[1] == per_iter[2] == (n, 5 if split else 4)
            check_log(d.script, run(program, [d]))
    assert solve_counts(True, True, 100, 25, 1, split_intervals=1, split_solve=True)[0] == 8 * 100 + 2 * 25 + 4
    assert solve_counts(False, True, 100, 25, 1, split_intervals=1, split_solve=True)[0] == 13 * 100 + 3 * 25 + 4


def test_random_sequences(program):
    rng = random.Random(20250611)
    drives = []
    for _ in range(NRANDOM):
        ns = rng.randint(1, 4)
        d = Drive(ns, rng.random() < 0.8)
        open_launch = {}                   # stream -> register of a start event whose kernel is still to come
        events = []                        # registers of valid events of the current generation, with their streams
        for _ in range(rng.randint(5, 60)):
            s = rng.randrange(ns)
            r = rng.random()
            if r < 0.35:
                if rng.random() < 0.1:
                    d.refuse_next(rng.randint(1, 2))
                d.timed_on(s, rng.randrange(5))
                d.refuse_next(0)
            elif r < 0.5:
                reg = d.mark(s)
                if d.valid(reg):
                    events.append((reg, s))
            elif r < 0.65:
                cand = [(reg, es) for reg, es in events if es != s]
                if cand:
                    d.wait(s, rng.choice(cand)[0])
            elif r < 0.75:
                d.touch(s)
            elif r < 0.85:
                d.kernel(s)
            elif r < 0.9:
                d.foreign_record(s, rng.randrange(5))
            elif r < 0.97:
                d.check(harvest=rng.random() < 0.3)
                events = [(reg, es) for reg, es in events if d.reg[reg][0] == d.cur ^ 1]      # the pool just left is drained at the next check
            else:
                d.swap() if not (d.timed[d.cur ^ 1] or d.used[d.cur ^ 1]) else d.drain(d.cur ^ 1)
                events = [(reg, es) for reg, es in events if d.reg[reg][0] == d.cur]
        d.counts()
        drives.append(d)
    logs = split_tapes(drives, run(program, drives))
    launches = sum(check_log(d.script, log) for d, log in zip(drives, logs))
    shared = sum(1 for d in drives for line in d.want if line.startswith("= ")) - sum(1 for d in drives for line in d.want if line.startswith("R "))
    print("launches", launches, "events handed out again", shared)
    assert launches > 10000 and shared > 5000
