"""A model of EventTape (csrc/omc_events.h) and of the order in which the solve loop (csrc/omc_relax_solve.cpp) drives it, restated in
Python for tests/test_event_tape_cpu.py (which runs scripts through tests/host/event_tape_check.cpp) and tests/test_event_tape.py (which
compares the record counter of a solve with the model's count).

Drive writes a script for the program and, beside it, the lines the program must print for it.  iteration() is one ADMM iteration of the
loop: the wait for the main stream, the body (base: quiet or split; Shor), the check's wait."""

S_MAIN, S_M, S_B, S_C = 0, 1, 2, 3      # T_S, T_M, T_B, T_C


class Drive:
    def __init__(self, nstreams, merge):
        self.script, self.want = [], []
        self.merge = merge
        self.adj = [-1] * nstreams
        self.cur, self.used, self.timed = 0, [0, 0], [[], []]
        self.reg = []
        self.refuse = 0
        self.nrec = self.nwait = 0
        self.kernels = 0
        self._op("N %d %d" % (nstreams, int(merge)), "N %d %d" % (nstreams, int(merge)))

    def _op(self, line, *out):
        self.script.append(line)
        self.want += list(out)

    def note(self, text):
        self._op("# " + text, "# " + text)

    def touch(self, s):
        self.adj[s] = -1
        self._op("T %d" % s)

    def kernel(self, s):
        self.adj[s] = -1
        self.kernels += 1
        self._op("K %d %d" % (s, self.kernels), "K %d %d" % (s, self.kernels))
        return self.kernels

    def _fresh(self, s, out):
        i = self.used[self.cur]
        if self.refuse > 0:
            self.refuse -= 1
            out.append("refused %d %d %d" % (self.cur, i, s))
            return None
        out.append("R %d %d %d" % (self.cur, i, s))
        self.used[self.cur] = i + 1
        self.nrec += 1
        self.adj[s] = i
        return (self.cur, i)

    def _event(self, op, s):
        out = []
        if op != "E" and self.merge and self.adj[s] >= 0:
            e = (self.cur, self.adj[s])
        else:
            e = self._fresh(s, out)
        out.append("= %d %d" % e if e else "= -")
        self.reg.append(e)
        self._op("%s %d" % (op, s), *out)
        return len(self.reg) - 1

    def begin(self, s):
        return self._event("B", s)

    def end(self, s):
        return self._event("E", s)

    def mark(self, s):
        return self._event("M", s)

    def valid(self, r):
        return self.reg[r] is not None

    def wait(self, s, r):
        self.adj[s] = -1
        self.nwait += 1
        self._op("W %d %d" % (s, r), "W %d %d %d" % ((s,) + self.reg[r]))

    def launch(self, r0, r1, cls):
        self.timed[self.cur].append((self.reg[r0][1], self.reg[r1][1], cls))
        self._op("L %d %d %d" % (r0, r1, cls))

    def foreign_record(self, s, g):
        self.adj[s] = -1
        self.nrec += 1
        self._op("G %d %d" % (s, g), "G %d %d" % (s, g))

    def foreign_wait(self, s, g):
        self.adj[s] = -1
        self.nwait += 1
        self._op("V %d %d" % (s, g), "V %d %d" % (s, g))

    def refuse_next(self, n):
        self.refuse = n
        self._op("X %d" % n)

    def swap(self):
        self.cur ^= 1
        self.adj = [-1] * len(self.adj)
        self._op("S", "S %d" % self.cur)

    def drain(self, pool):
        self._op("D %d" % pool, "D %d" % pool + "".join(" %d:%d:%d" % l for l in self.timed[pool]))
        self.timed[pool] = []
        self.used[pool] = 0
        if pool == self.cur:
            self.adj = [-1] * len(self.adj)

    def counts(self):
        self._op("C", "C %d %d" % (self.nrec, self.nwait))

    # ---- what the solve loop does with the tape ----------------------------------------------------------------------------------------
    def timed_on(self, s, cls):
        """TIMED_ON: start event, the launch, stop event."""
        r0 = self.begin(s)
        self.kernel(s)
        if self.valid(r0):
            r1 = self.end(s)
            if self.valid(r1):
                self.launch(r0, r1, cls)

    def run(self, s, cls, timed):
        if timed:
            self.timed_on(s, cls)
        else:
            self.kernel(s)

    def depend(self, src, to, to2, on_tape, g):
        if on_tape:
            r = self.mark(src)
            if self.valid(r):
                self.wait(to, r)
                if to2 is not None:
                    self.wait(to2, r)
                return
        self.foreign_record(src, g)
        self.foreign_wait(to, g)
        if to2 is not None:
            self.foreign_wait(to2, g)

    def join_sides(self, ids, on_tape):
        im, ib, ic = ids
        rb = self.mark(ib) if on_tape else None
        if rb is None or not self.valid(rb):
            rb = None
            self.foreign_record(ib, 1)
        rc = self.mark(ic) if on_tape else None
        if rc is None or not self.valid(rc):
            rc = None
            self.foreign_record(ic, 2)
        for r, g in ((rb, 1), (rc, 2)):
            if r is not None:
                self.wait(im, r)
            else:
                self.foreign_wait(im, g)

    def iteration(self, multi, timed, split=False, shor=False, with_aa=False, is_check=False, wait_main=False, sub=True, big_sub=True):
        """One eager iteration (enqueue_iteration / enqueue_body); returns (records, waits) it enqueued."""
        rec0, wait0 = self.nrec, self.nwait
        ids = (S_M, S_B, S_C) if multi else (S_MAIN, S_MAIN, S_MAIN)
        im, ib, ic = ids
        tp = timed and self.merge
        if multi and wait_main:
            self.foreign_wait(im, 9)
        if wait_main:
            self.touch(im)
        if multi:
            self.depend(im, ib, ic, tp, 0)
        if shor:
            if sub:
                self.run(im, 1, timed)
            if big_sub:
                self.run(ib, 7, timed)
            self.run(ib, 7, timed)
            self.run(im, 2, timed)
            self.run(ic, 3, timed)
            self.run(ic, 8, timed)
            if multi:
                self.join_sides(ids, tp)
            self.run(im, 4, timed)
            self.run(im, 9, timed)
            self.run(im, 8, timed)
        else:
            assert not split or multi
            r4 = None
            if split:
                self.run(ic, 3, timed)
                self.run(ic, 2, timed)
                if tp:
                    r4 = self.mark(ic)
                    if not self.valid(r4):
                        r4 = None
                if r4 is None:
                    self.foreign_record(ic, 4)
            if sub:
                self.run(im, 1, timed)
            self.run(ib, 0, timed)
            if split:
                if r4 is not None:
                    self.wait(im, r4)
                else:
                    self.foreign_wait(im, 4)
            self.run(im, 2, timed)
            if not split:
                self.run(ic, 3, timed)
            if multi:
                self.join_sides(ids, tp)
            self.run(im, 4, timed)
            if with_aa:
                self.run(im, 5, timed)
        if multi and is_check:
            self.depend(im, S_MAIN, None, tp, 3)
        return self.nrec - rec0, self.nwait - wait0

    def check(self, harvest=False):
        """What a check puts on the main stream, the read and the swap of the pools; the older pool is drained first."""
        self.touch(S_MAIN)
        for cls in (10, 11, 12):
            self.timed_on(S_MAIN, cls)
        self.touch(S_MAIN)
        self.drain(self.cur ^ 1)
        self.swap()
        if harvest:
            self.touch(S_MAIN)
            self.timed_on(S_MAIN, 13)
            self.touch(S_MAIN)
            self.timed_on(S_MAIN, 14)
            self.touch(S_MAIN)


def solve_counts(merge, multi, iters, check_every, stride, split_intervals=0, split_solve=False, shor=False, accel=False, sub=True, big_sub=True):
    """(records, waits) the iterations of an eager solve enqueue.  With every interval sampled alike (check_every a multiple of stride) the sum
    depends on how many intervals ran split, not on which: the first `split_intervals` are taken."""
    d = Drive(4, merge)
    rec = waits = 0
    for it in range(1, iters + 1):
        is_check = it % check_every == 0
        interval = (it - 1) // check_every
        split = split_solve and not shor and interval < split_intervals
        r, w = d.iteration(multi, stride > 0 and it % stride == 0, split=split, shor=shor, with_aa=accel and not is_check and not shor,
                           is_check=is_check, wait_main=(it - 1) % check_every == 0, sub=sub, big_sub=big_sub)
        rec += r
        waits += w
        if is_check:
            d.check()
    return rec, waits
