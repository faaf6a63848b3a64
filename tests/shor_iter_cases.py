"""Cases of tests/test_shor_iter_cpu.py and tests/test_shor_iter.py: Shor-mode nodes whose state after a few iterations is pinned to
oracle/omc_oracle_shor.py.  gamma = 80, rank 1, the default Shor penalties, cold starts; instances from omc_oracle.make_instance(..., noise = 0.3)
with masks edited as described per case.  Every case states the structural conditions (on ShorStructure) that make it bite; `check_structure`
asserts them (the CPU test runs it for every case).

  A   8 x 10, three column types: columns 2, 5, 7 (0-based) fully observed; every minor (i1, i2, 3, 6) puts columns 2 and 5 wholly in C (type 2),
      six more minors share V1 / V2 keys (counts >= 4) and one coordinate lies in 7 minors or more
  B   A with depth-1 and depth-2 cut nodes (rows, NNQP, small cone, k_global's Shor flag)
  C   A with check_every = 2 and a penalty bump at the check of iteration 2: t = 3 is the first state behind k_shor_rescale
  D   12 x 14 with 255, 256, 257 and 513 minors: the one-lane-per-minor kernels at one, exactly one, two and three blocks
  E   8 x 10 degenerate lists: no minors; an explicit SOC list with every second outside entry; columns without a SOC row outside C (s = 0)
  F   257 x 260 and 4 x 257: the 256-strided loops of k_shor_cols / k_shor_reduce / k_shor_harvest wrap (rows in the first, columns in
      the second).  The engine and the reference require n <= m (OMC.jl:249-254), so the smallest shape whose row loop wraps has 257 columns or
      more: the big cone is of order 517 there and of order 261 in the second
  batch   on D's instance: A's list, the empty list and D's 257 minors as one batch through two slots
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import omc_oracle as orc            # noqa: E402
import omc_oracle_shor as sh        # noqa: E402
import omc_shor_iter_ref as ref     # noqa: E402

GAMMA = 80.0
A_EXTRA = [(1, 2, 8, 9), (1, 3, 1, 8), (2, 5, 4, 10), (1, 2, 3, 8), (1, 2, 3, 9), (1, 2, 3, 10)]
C_PARAMS = dict(check_every=2, bump_after=2, bump_window=1, bump_ratio=0.1, bump_max=1)


class Case:
    def __init__(self, name, A, mask, minors, soc, ts, cuts=(), params=None, soc_gpu=None, conditions=()):
        self.name, self.A, self.mask = name, A, mask
        self.n, self.m = A.shape
        self.inst = orc.Instance(A, mask, GAMMA, 1)
        self.minors = [tuple(int(v) for v in q) for q in minors]
        self.soc = list(soc)               # what the oracle takes: always explicit
        self.soc_gpu = soc_gpu             # what the engine takes: None = "every coordinate outside the minors"
        self.ts = tuple(ts)
        self.cuts = list(cuts)
        self.params = dict(params or {})
        self.conditions = tuple(conditions)
        self.structure = sh.ShorStructure(self.n, self.m, self.minors, self.soc, mask)


def _instance_A():
    A, mask = orc.make_instance(8, 10, 1, n_indices=45, seed=5, noise=0.3)
    mask = mask.copy(); mask[:, [2, 5, 7]] = True
    minors = [(i1, i2, 3, 6) for i1, i2 in itertools.combinations(range(1, 9), 2)] + A_EXTRA
    return A, mask, minors


def _complement(mask, minors):
    return sh.driver_shor_lists(mask, minors=list(minors))[1]


def _cut_nodes(inst):
    """depth-1 and depth-2 cut nodes as tests/test_gpu_shor.py builds them (left, then right)"""
    cuts = []; nodes = []
    for d in range(2):
        r0 = orc.sdp_relaxation(inst, cuts=cuts)
        x, _ = orc.breakpoint_vector(r0["Y"], r0["U"])
        cuts = cuts + [(x, r0["U"], ["left" if d % 2 == 0 else "right"])]
        nodes.append(list(cuts))
    return nodes


def _instance_D():
    A, mask = orc.make_instance(12, 14, 1, n_indices=90, seed=7, noise=0.3)
    mask = mask.copy(); mask[:, [0, 1, 4]] = True           # 0, 1: wholly in C through their pair list (type 2); 4: observed, partly in C (type 1)
    mask[11, [2, 3, 5, 6, 7, 8, 9]] = False                 # the other sub-grid columns keep an unobserved entry outside C (type 0)
    return A, mask


def _minors_D(count):
    """The full pair list of the fully observed columns 1, 2 (66 minors), then the first count - 66 tuples of a seeded permutation of the
    tuples over rows 1 .. 8 x columns 3 .. 10."""
    pairs = [(i1, i2, 1, 2) for i1, i2 in itertools.combinations(range(1, 13), 2)]
    grid = [(i1, i2, j1, j2) for i1, i2 in itertools.combinations(range(1, 9), 2) for j1, j2 in itertools.combinations(range(3, 11), 2)]
    perm = np.random.default_rng(77).permutation(len(grid))
    return pairs + [grid[p] for p in perm[:count - len(pairs)]]


def _instance_F(n, m):
    A, mask = orc.make_instance(n, m, 1, n_indices=int(0.55 * n * m), seed=11, noise=0.3)
    return A, mask.copy()


def _build():
    cases = {}
    A, mask, minors = _instance_A()
    socA = _complement(mask, minors)
    three = ("three_types", "shared_keys", "crowded_coordinate")
    cases["A"] = Case("A", A, mask, minors, socA, (1, 2, 3, 7, 26), conditions=three)
    for d, cuts in enumerate(_cut_nodes(cases["A"].inst), 1):
        cases["B-depth%d" % d] = Case("B-depth%d" % d, A, mask, minors, socA, (1, 3), cuts=cuts, conditions=three)
    cases["C"] = Case("C", A, mask, minors, socA, (2, 3, 4, 6), params=C_PARAMS, conditions=three + ("bump_at_2",))
    AD, maskD = _instance_D()
    for cnt in (255, 256, 257, 513):
        mi = _minors_D(cnt)
        cases["D-%d" % cnt] = Case("D-%d" % cnt, AD, maskD, mi, _complement(maskD, mi), (1, 3), conditions=("three_types", "count=%d" % cnt))
    allsoc = _complement(mask, [])
    cases["E-empty"] = Case("E-empty", A, mask, [], allsoc, (1, 3), conditions=("no_minors",))
    cases["E-half-soc"] = Case("E-half-soc", A, mask, minors, socA[::2], (1, 3), soc_gpu=socA[::2], conditions=three)
    soc0 = [(i, j) for (i, j) in socA if j not in (1, 8)]      # column 1 (type 0) and column 8 (type 1) keep no SOC row outside C
    cases["E-s0"] = Case("E-s0", A, mask, minors, soc0, (1, 3), soc_gpu=soc0, conditions=three + ("empty_paraboloid",))
    # F: the chain (i, i + 1, 1, 2), i odd, and (256, 257, 1, 2) put columns 1 and 2 of the tall shape wholly in C: a type-2 column of 257 rows
    # needs 129 minors; a dozen more on the other columns
    AF, maskF = _instance_F(257, 260)
    maskF[:, [0, 1]] = True
    tall = [(i, i + 1, 1, 2) for i in range(1, 256, 2)] + [(256, 257, 1, 2)]
    tall += [(1, 2, 3, 4), (3, 200, 3, 4), (255, 257, 3, 4), (100, 101, 2, 3), (5, 257, 1, 4), (17, 129, 3, 4), (64, 65, 3, 4), (128, 256, 3, 4),
             (2, 3, 3, 4), (250, 251, 3, 4), (30, 31, 2, 4), (254, 256, 3, 4)]
    cases["F-257x260"] = Case("F-257x260", AF, maskF, tall, _complement(maskF, tall), (1, 3), conditions=("has_type2", "last_row", "rows_wrap"))
    AF, maskF = _instance_F(4, 257)
    maskF[:, [0, 1]] = True
    wide = [(1, 2, 1, 2), (3, 4, 1, 2), (1, 2, 3, 257), (3, 4, 256, 257), (1, 4, 100, 200), (2, 3, 5, 6), (1, 3, 5, 7), (1, 2, 128, 129), (2, 4, 255, 256),
            (1, 2, 3, 4), (3, 4, 3, 257), (1, 4, 2, 257)]
    cases["F-4x257"] = Case("F-4x257", AF, maskF, wide, _complement(maskF, wide), (1, 3), conditions=("has_type2", "last_column", "columns_wrap"))
    return cases


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _build()
    return _cases


NAMES = ["A", "B-depth1", "B-depth2", "C", "D-255", "D-256", "D-257", "D-513", "E-empty", "E-half-soc", "E-s0", "F-257x260", "F-4x257"]
TS = {"A": (1, 2, 3, 7, 26), "B-depth1": (1, 3), "B-depth2": (1, 3), "C": (2, 3, 4, 6), "D-255": (1, 3), "D-256": (1, 3), "D-257": (1, 3), "D-513": (1, 3),
      "E-empty": (1, 3), "E-half-soc": (1, 3), "E-s0": (1, 3), "F-257x260": (1, 3), "F-4x257": (1, 3)}
RUNS = [(name, t) for name in NAMES for t in TS[name]]
BATCH_T = 3


def run_id(run):
    return "%s-t%d" % run


def batch_lists():
    """(instance case, [(minors, explicit soc)] of the three nodes): A's list, the empty list, D's 257 minors, all on D's instance."""
    D = cases()["D-257"]
    out = []
    for mi in (cases()["A"].minors, [], D.minors):
        out.append((list(mi), _complement(D.mask, mi)))
    return D, out


def check_structure(c):
    """The conditions that make the case bite; raises AssertionError naming the one that fails."""
    st = c.structure
    for cond in c.conditions:
        if cond == "three_types":
            assert set(np.unique(st.ctype)) == {0, 1, 2}, (c.name, cond, st.ctype)
        elif cond == "shared_keys":
            assert st.cnt1.max() >= 4 and st.cnt2.max() >= 4, (c.name, cond, st.cnt1.max(), st.cnt2.max())
        elif cond == "crowded_coordinate":
            assert st.cntC.max() >= 7, (c.name, cond, st.cntC.max())
        elif cond == "no_minors":
            assert st.nq == 0 and st.inS.all(), (c.name, cond)
        elif cond == "empty_paraboloid":
            empty = [j for j in range(c.m) if st.ctype[j] != 2 and not st.inS[:, j].any()]
            assert empty and {int(st.ctype[j]) for j in empty} == {0, 1}, (c.name, cond, empty)
        elif cond == "has_type2":
            assert (st.ctype == 2).any() and (st.ctype != 2).any(), (c.name, cond, st.ctype)
        elif cond == "last_row":
            assert st.inC[c.n - 1].any(), (c.name, cond)
        elif cond == "last_column":
            assert st.inC[:, c.m - 1].any(), (c.name, cond)
        elif cond == "rows_wrap":
            assert c.n > 256, (c.name, cond)
        elif cond == "columns_wrap":
            assert c.m > 256 and c.n + c.m == 261, (c.name, cond)
        elif cond.startswith("count="):
            assert st.nq == int(cond[6:]), (c.name, cond, st.nq)
        elif cond == "bump_at_2":
            r = reference(c.name, 3)
            assert r["n_bumps"] == 1 and r["rho"] == 4.0 * sh.ShorParams().rho and r["check_iters"] == [2, 3], (c.name, cond, r["n_bumps"], r["rho"])
            assert reference(c.name, 2)["n_bumps"] == 0      # the cap comes before the bump of the same check
        else:
            raise AssertionError("unknown condition " + cond)


_refs = {}
_erefs = {}


def reference(name, t):
    """the oracle's state of case `name` after t iterations: computed once, shared, never written to"""
    if (name, t) not in _refs:
        c = cases()[name]
        _refs[(name, t)] = ref.shor_state(c.inst, c.minors, c.soc, c.cuts, t, **c.params)
    return _refs[(name, t)]


def e_ref(name, t):
    """the reference's own error per array and scalar: the perturbation spread, and not below the rounding of the state to float64"""
    if (name, t) not in _erefs:
        c = cases()[name]
        r = reference(name, t)
        sp = ref.perturbation_spread(c.inst, c.minors, c.soc, c.cuts, t, ref=r, **c.params)
        fl = ref.representation_floor(r)
        _erefs[(name, t)] = {key: max(sp[key], fl[key]) for key in sp}
    return _erefs[(name, t)]
