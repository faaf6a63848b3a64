"""CPU tests of the boundary of appending Shor nodes: the three entry points are declared, exported and listed; NULL handles are
refused before any device call; the Python wrappers exist; the drivers' Shor keywords and their range checks; and the list bookkeeping
that bnb.branch_and_bound and bnb_stream.branch_and_bound_streaming share (shor_lists.ShorLists) gives, fed the same random stream, the
same child lists for a scripted sequence of splits."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["omc_relax_reserve_shor", "omc_relax_append_shor", "omc_relax_fetch_done_shor"]
SHOR_KEYWORDS = ["add_Shor_valid_inequalities", "Shor_valid_inequalities_noisy_rank1_num_entries_present", "add_Shor_valid_inequalities_fraction",
                 "add_Shor_valid_inequalities_iterative", "max_update_Shor_indices_probability", "min_update_Shor_indices_probability",
                 "update_Shor_indices_probability_decay_rate", "update_Shor_indices_n_minors", "shor_params", "shor_warm_start", "shor_warm_depth"]


def test_new_entry_points_are_declared_exported_and_listed(omc):
    hdr = open(os.path.join(ROOT, "include", "omc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(omc_[A-Za-z0-9_]+)\s*\(", hdr))
    lib = omc.load()
    for s in NEW:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in omc.EXPORTS, s


def test_null_handles_are_refused_before_any_device_call(omc):
    lib = omc.load()
    ptr = omc.pkg._lib.ptr
    one = np.ones(1, np.int64); L = np.zeros(1, np.int32); ids = np.zeros(1, np.int32)
    assert lib.omc_relax_reserve_shor(None, 1, 1) == -3
    assert lib.omc_relax_append_shor(None, 1, ptr(L), None, None, None, ptr(one), ptr(np.array([[1, 2, 1, 2]], np.int64)), ptr(-one), None, None, None) == -3
    assert lib.omc_relax_fetch_done_shor(None, 1, ptr(ids), None, None, None) == -3


def test_python_wrappers_exist(omc):
    for name in ("reserve_shor", "append_shor", "fetch_done_shor"):
        assert callable(getattr(omc.Engine, name)), name
    assert list(inspect.signature(omc.Engine.reserve_shor).parameters) == ["self", "nq_max", "extra_lists"]
    p = inspect.signature(omc.Engine.append_shor).parameters
    assert list(p) == ["self", "nodes", "shor_info", "disjunctive_cuts_type", "load_from", "save_to"]
    assert p["disjunctive_cuts_type"].default == "linear" and p["load_from"].default is None and p["save_to"].default is None
    p = inspect.signature(omc.Engine.fetch_done_shor).parameters
    assert list(p) == ["self", "ids", "want_W", "want_Theta"] and p["want_W"].default is False and p["want_Theta"].default is False


def test_streaming_driver_has_the_shor_keywords_of_the_round_based_one(omc):
    a = inspect.signature(omc.pkg.bnb.branch_and_bound).parameters
    b = inspect.signature(omc.pkg.bnb_stream.branch_and_bound_streaming).parameters
    for kw in SHOR_KEYWORDS:
        assert kw in b, kw
        assert b[kw].default == a[kw].default, kw


class _Stub:
    """What the drivers touch before their first device call, and a deterministic stand-in for the two list generators."""
    def __init__(self, n, m, k):
        self.n, self.m, self.k, self.gamma, self.device = n, m, k, 80.0, 0
        self.calls = []

    def generate_rank1_matrix_completion_Shor_constraints_indexes(self, classes):
        return np.array([(i1, i2, j1, j2) for i1 in range(1, 4) for i2 in range(i1 + 1, 5) for j1 in range(1, 3) for j2 in range(j1 + 1, 4)], np.int64)

    def generate_violated_Shor_minors(self, X3, classes, existing, n_minors):
        """n_minors tuples that are not in `existing`, chosen by X: first row index from the largest entry of X."""
        X = X3[0]; n, m = X.shape
        self.calls.append((len(existing), n_minors))
        i0 = int(np.argmax(np.abs(X).sum(1)))
        ex = set(existing); out = []
        for s in range(n):
            i1 = (i0 + s) % n
            for i2 in range(i1 + 1, n):
                for j1 in range(m):
                    for j2 in range(j1 + 1, m):
                        t = (i1 + 1, i2 + 1, j1 + 1, j2 + 1)
                        if t not in ex and len(out) < n_minors:
                            out.append((float(abs(X[i1, j1] * X[i2, j2] - X[i1, j2] * X[i2, j1])), t))
        return out


def test_range_checks_and_rank(omc):
    A = np.zeros((6, 8)); mask = np.ones((6, 8), bool)
    stream = omc.pkg.bnb_stream.branch_and_bound_streaming
    with pytest.raises(NotImplementedError):
        stream(_Stub(6, 8, 2), A, mask, add_Shor_valid_inequalities=True)
    bad = [dict(add_Shor_valid_inequalities_fraction=1.5),
           dict(add_Shor_valid_inequalities_iterative=True, max_update_Shor_indices_probability=1.5),
           dict(add_Shor_valid_inequalities_iterative=True, min_update_Shor_indices_probability=0.0),
           dict(add_Shor_valid_inequalities_iterative=True, update_Shor_indices_probability_decay_rate=1.0),
           dict(add_Shor_valid_inequalities_iterative=True, update_Shor_indices_n_minors=0)]
    for kw in bad:
        with pytest.raises(ValueError) as e1:
            stream(_Stub(6, 8, 1), A, mask, add_Shor_valid_inequalities=True, **kw)
        with pytest.raises(ValueError) as e2:
            omc.pkg.bnb.branch_and_bound(_Stub(6, 8, 1), A, mask, add_Shor_valid_inequalities=True, **kw)
        assert str(e1.value) == str(e2.value), kw


def test_both_drivers_build_the_same_child_lists(omc):
    """The helper both drivers import, driven as each of them drives it (bnb passes the solving handle and the X it already holds,
    bnb_stream the second handle and a fetch that runs only when the coin wins), on the same random stream and the same scripted splits:
    the same coins, the same scans, the same lists; every child list has its parent's as a prefix."""
    bnb, st = omc.pkg.bnb, omc.pkg.bnb_stream
    assert bnb.ShorLists is st.ShorLists is omc.pkg.shor_lists.ShorLists
    n, m = 6, 8
    xr = np.random.default_rng(3)
    script = [(d, xr.standard_normal((n, m))) for d in (0, 1, 1, 2, 5, 9, 30, 31, 40, 3)]      # (depth of the split node, its X)
    runs = []
    for how in ("bnb", "stream"):
        cls = bnb.ShorLists if how == "bnb" else st.ShorLists
        L = cls((4,), 1.0, True, 1.0, 0.1, 1.1, 5)
        eng = _Stub(n, m, 1); rng = np.random.default_rng(0); counters = {}; fetched = []
        cur = L.root(eng, rng)
        assert cur.shape == (0, 4)
        out = []
        for depth, X in script:
            if how == "bnb":
                child = L.child(eng, cur, depth, lambda: X, rng, 1, counters)
            else:
                def fetch():
                    fetched.append(depth)
                    return X
                child = L.child(eng, cur, depth, fetch, rng, 1, counters)
            assert len(child) >= len(cur) and np.array_equal(child[:len(cur)], cur)
            assert (child is cur) == (len(child) == len(cur))
            out.append(child); cur = child
        runs.append((out, eng.calls, counters, rng.random()))
        if how == "stream":
            assert len(fetched) == counters["shor_updates"] < len(script)      # X is fetched only for the nodes that won the coin
    (la, ca, na, ra), (lb, cb, nb, rb) = runs
    assert ca == cb and na == nb and ra == rb
    assert all(np.array_equal(x, y) for x, y in zip(la, lb))
    assert len(la[-1]) == 5 * na["shor_updates"] > 0
    # p(depth) of OMC.jl:956-967 and the static mode
    L = bnb.ShorLists((4,), 1.0, True, 1.0, 0.1, 1.1, 5)
    assert L.update_probability(0) == 1.0 and L.update_probability(3) == 1.0 / 1.1 ** 3 and L.update_probability(30) == 0.1
    S = bnb.ShorLists((4,), 0.5)
    r1 = S.root(_Stub(n, m, 1), np.random.default_rng(1)); r2 = S.root(_Stub(n, m, 1), np.random.default_rng(1))
    assert np.array_equal(r1, r2) and 0 < len(r1) < 18
    assert S.child(None, r1, 4, None, None) is r1 and S.pool_nq_max(r1, 32) == len(r1) and L.pool_nq_max(r1[:0], 3) == 15
