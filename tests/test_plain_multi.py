"""Separation, rounding and the left singular vectors on the multi-workgroup eigen-kernels (omc_launch_cone_plain_mw: k_mw_plain_fro,
k_mw_plain_prepare, k_mw_round at the threshold omc_plain_multi_tau(), k_mw_plain_norms, k_mw_plain_pick) against the references of
oracle/omc_plain_ref.py, with the bounds of tests/test_plain_ops.py (its docstring; its checkers are imported, tau = the library's).
Orders, reached with OMC_PLAIN_MULTI_MIN = 145 (tests/plain_multi_cases.py): 145 (smallest; 15 zero rows and columns inside a real block),
160 (no padding, nb = 10), 161 (NP = 176, Ncp = 192: 31 padding columns), 176 (a whole block of zero columns paired with real ones), 257
(several trips of every wave's row loop); and 1040 at the default knob (nb = 66), the order the default dispatch serves.
e_ref of every input is read from tests/golden/plain_multi_error_units.json (tools/record_plain_multi_error_units.py); the long-double
Rayleigh quotients are formed here for the extreme eigenvectors only (N^2 work), the rest of the spectrum, which enters through gaps
alone, is LAPACK's.

Measured on an MI355X, worst error over bound per order: MEASURED below (every run prints its own figures, one line per order)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import omc_plain_ref as R
import plain_multi_cases as PC
from test_plain_ops import _check_sep, _check_topk, _engine, _rb, _ratio, ERR_ARGUMENT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
KNOB = "OMC_PLAIN_MULTI_MIN"
MEASURED = """
worst over the cases of each order, product library, MI355X (sweeps: most of one call, separation / rounding / left singular vectors):
  order                eigenvalue error / e_ref  residual / rb  vector / (2 rb / gap)  eigenspace  weighted x  U'U - I / bound  sweeps
  145                  0.203   (bound 4)         0.027          0.014                  0.0099      0.0033      0.059            10 / 15 / 10
  160                  0.233                     0.022          0.0037                 0.010       0.0030      0.100            10 / 16 / -
  161                  0.216                     0.025          0.011                  0.012       0.0025      0.106            11 / 14 / 10
  176                  0.228                     0.036          0.018                  0.016       0.0037      0.201            11 / 15 / 11
  257                  0.253                     0.027          0.0088                 0.013       0.0036      0.110            11 / 13 / 12
  1040, default knob   0.190                     0.030          0.0013                 0.014       0.0045      0.0039           13 / 12 / -
  inside a solve (160 x 170): eigenvalue error 0.16 e_ref on the new path, 0.91 on the cold kernel; residual 0.018 / 0.069 of rb
  largest cosine between two returned columns: 0.50 tau (rounding, order 145, k = 8), 0.10 tau (left singular vectors, (145, 147))
  asynchronous arm of the solve: 6 asynchronous harvests, iterations 140, 200, 160, 200, 200, 200, 200; every output equal to the synchronous arm's
With Q applied as accumulated (the arithmetic of the clip path) the eigenvalue errors are 7.4 - 10.4 e_ref (the first case of each test) and
test_separation, test_order_1040_at_the_default_knob and test_inside_a_solve fail at every order; with c by division instead of rsqrt and Q
as accumulated, 5.4 - 6.4 e_ref and the same tests fail; with the division on top of the unit columns, the figures above to within 0.04."""


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    # the imported checkers state their bounds with tau = omc_plain_ref.TAU: they hold for this path only while it rotates to the same threshold
    assert omc.pkg.api.plain_multi_tau() == R.TAU
    return True


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(HERE, "golden", "plain_multi_error_units.json")) as f:
        return json.load(f)["cases"]


_refs = {}


def _ref(gold, key, M, M_ld):
    """Reference of one input, computed once: eigenvalues ascending (long-double Rayleigh quotients of LAPACK's vectors for the 3 smallest
    and the 9 largest, LAPACK's own values between them), LAPACK's vectors, e_ref from the golden file, ||M||_F."""
    if key not in _refs:
        w, V = np.linalg.eigh(M)
        N = M.shape[0]
        idx = np.r_[0:3, N - 9:N]
        Vl = np.asarray(V[:, idx], LD)
        lam = np.asarray(w, LD)
        lam[idx] = (Vl * (np.asarray(M_ld, LD) @ Vl)).sum(axis=0) / (Vl * Vl).sum(axis=0)
        f = R.fro(M)
        rec = gold[key]
        assert abs(f - rec["fro"]) <= 1e-9 * max(f, rec["fro"]), "%s: the recorded error units belong to another input" % key
        _refs[key] = dict(lam=lam, V=V, e=rec["units"] * R.U_RND * f, fro=f, M=M)
    return _refs[key]


def _multi_engine(omc, n, m, k, knob="145"):
    eng = _engine(omc, n, m, k)
    if knob is not None:
        eng.tuning_set(KNOB, knob)
    return eng


def _stats_ok(eng, B, stats):
    st = eng.plain_multi_stats()
    assert st["calls"] == B and st["exhausted"] == 0, st
    stats["sweeps"] = max(stats.get("sweeps", 0), st["max_sweeps"])
    return st


def _report(op, N, stats):
    print("plain_multi %s N=%d  " % (op, N) + "  ".join("%s=%.3g" % kv for kv in sorted(stats.items())))


# ---- 1. separation ------------------------------------------------------------------------------------------------------------------------
def _separation(omc, gold, eng, N, stats):
    cases = PC.sep_cases(N)
    ins = [R.sep_input(fam, N, R.SEP_K, seed) for _, fam, seed in cases]
    refs = [None if fam == "e" else _ref(gold, key, R.sep_matrix(Y, Uu), R.sep_matrix_ld(Y, Uu)) for (key, fam, _), (Y, Uu) in zip(cases, ins)]
    for rule in ("smallest_1_eigvec", "smallest_2_eigvec"):
        x, ev, fe = eng.breakpoint_vectors([Y for Y, _ in ins], [Uu for _, Uu in ins], rule)
        _stats_ok(eng, len(cases), stats)
        for b, (key, fam, _) in enumerate(cases):
            _check_sep(N, fam, rule, refs[b], ev[b], x[b], fe[b], stats)
            if fam != "e":      # feasible against the reference's sign of lambda_min + 1e-6
                assert bool(fe[b]) == (float(refs[b]["lam"][0]) - R.FEAS_TOL >= 0.0), (key, rule)


@pytest.mark.parametrize("N", PC.SMALL_ORDERS)
def test_separation(have_gpu, omc, gold, N):
    """Every family of R.SEP_FAMILIES (the exact zero matrix among them) under both breakpoint rules, one batch per rule."""
    assert [f for _, f, _ in PC.sep_cases(N)] == R.SEP_FAMILIES
    eng = _multi_engine(omc, N, N, R.SEP_K)
    stats = {}
    _separation(omc, gold, eng, N, stats)
    eng.close()
    _report("sep", N, stats)


# ---- 2. rounding and 3. left singular vectors -----------------------------------------------------------------------------------------
def _rounding(omc, gold, N, k, stats, knob):
    cases = PC.round_cases(N, k)
    Ys = [R.round_input(fam, N, k, seed) for _, fam, seed in cases]
    eng = _multi_engine(omc, N, N, k, knob)
    got = eng.round_Y(Ys)
    _stats_ok(eng, len(cases), stats)
    eng.close()
    for (key, fam, _), Y, Ug in zip(cases, Ys, got):
        if fam == "zero":      # finite orthonormal coordinate columns
            _check_topk(N, k, fam, None, None, None, Ug, stats, key)
            assert np.array_equal(np.sort(np.abs(Ug), axis=0)[-1], np.ones(k)) and np.count_nonzero(Ug) == k, key
            continue
        ref = _ref(gold, key, R.sym(Y), R.sym_ld(Y))
        _check_topk(N, k, fam, ref, np.asarray(ref["lam"], float)[::-1], ref["V"][:, ::-1], Ug, stats, key)


@pytest.mark.parametrize("N", PC.SMALL_ORDERS)
def test_rounding(have_gpu, omc, gold, N):
    """R.ROUND_FAMILIES at ranks 1 and 2, and 8 at orders 145 and 176."""
    stats = {}
    for k in PC.round_ranks(N):
        assert [f for _, f, _ in PC.round_cases(N, k)] == [f for f in R.ROUND_FAMILIES if f != "projector" or k == 2]
        _rounding(omc, gold, N, k, stats, "145")
    _report("round", N, stats)


@pytest.mark.parametrize("n,m", PC.SVD_SHAPES)
def test_left_singular_vectors(have_gpu, omc, gold, n, m):
    """The Gram product feeding the new path: families of R.SVD_FAMILIES, rank 2, against numpy's SVD of X itself."""
    k = PC.SVD_K
    cases = PC.svd_cases(n, m)
    assert [f for _, f, _ in cases] == R.SVD_FAMILIES
    Xs = [R.svd_input(fam, n, m, k, seed) for _, fam, seed in cases]
    eng = _multi_engine(omc, n, m, k)
    got = eng.left_singular(Xs)
    stats = {}
    _stats_ok(eng, len(cases), stats)
    eng.close()
    for (key, fam, _), X, Ug in zip(cases, Xs, got):
        if fam == "zero":
            _check_topk(n, k, fam, None, None, None, Ug, stats, key, R.TAU)
            continue
        ref = _ref(gold, key, X @ X.T, R.gram_ld(X))
        Uf, sv, _ = np.linalg.svd(X, full_matrices=True)
        s2 = np.zeros(n); s2[: sv.size] = sv ** 2
        _check_topk(n, k, fam, ref, s2, Uf, Ug, stats, key, R.TAU)
    _report("svd m=%d" % m, n, stats)


# ---- 4. order 1040 at the default knob ----------------------------------------------------------------------------------------------------
def test_order_1040_at_the_default_knob(have_gpu, omc, gold):
    """Families a, d (double eigenvalue), b_out, b_in, c_two under both rules with one long-lived engine, then `top` and `projector`
    of the rounding at rank 2: the default dispatch takes the new path here."""
    N = PC.BIG_ORDER
    assert omc.pkg.api.plain_multi_plan(N)["multi"] and omc.pkg.api.plain_multi_plan(N)["nb"] == 66
    assert [f for _, f, _ in PC.sep_cases(N)] == ["a", "b_out", "b_in", "c_two", "d"]
    eng = _engine(omc, N, N, R.SEP_K)
    stats = {}
    before = eng.cone_multi_stats()["calls"]
    _separation(omc, gold, eng, N, stats)
    assert eng.plain_multi_stats()["calls"] > 0
    assert eng.cone_multi_stats()["calls"] == before
    _report("sep", N, stats)
    eng.close()
    stats = {}
    assert [f for _, f, _ in PC.round_cases(N, PC.BIG_ROUND_K)] == PC.BIG_ROUND_FAMILIES
    _rounding(omc, gold, N, PC.BIG_ROUND_K, stats, None)
    _report("round", N, stats)


# ---- 5. dispatch, statistics, determinism ---------------------------------------------------------------------------------------------------
def test_dispatch_stats_and_determinism(have_gpu, omc, N=176):
    k = R.SEP_K
    eng = _engine(omc, N, N + 3, k)
    ins = [R.sep_input(f, N, k, 77 + i) for i, f in enumerate(["a", "g", "d"])]
    Ys, Us = [Y for Y, _ in ins], [Uu for _, Uu in ins]
    Yr = [R.round_input(f, N, k, 90 + i) for i, f in enumerate(["top", "projector", "top_small"])]
    Xs = [R.svd_input(f, N, N + 3, k, 60 + i) for i, f in enumerate(["product", "sparse", "product"])]
    cold = eng.breakpoint_vectors(Ys, Us)                      # the default knob: the cold kernel
    assert eng.plain_multi_stats() == dict(calls=0, max_sweeps=0, exhausted=0, device_us=0)
    eng.round_Y(Yr)
    assert eng.plain_multi_stats()["calls"] == 0
    clip_calls = eng.cone_multi_stats()["calls"]
    eng.tuning_set(KNOB, "145")
    for rule in ("smallest_1_eigvec", "smallest_2_eigvec"):
        got = eng.breakpoint_vectors(Ys, Us, rule)
        st = eng.plain_multi_stats()
        assert st["calls"] == 3 and st["exhausted"] == 0 and 1 < st["max_sweeps"] < R.MAX_SWEEPS and st["device_us"] > 0, st
        again = eng.breakpoint_vectors(Ys, Us, rule)
        assert all(np.array_equal(a, b) for a, b in zip(got, again))
        for i in range(3):      # slot independence: a batch of 3 against three batches of 1
            one = eng.breakpoint_vectors([Ys[i]], [Us[i]], rule)
            assert eng.plain_multi_stats()["calls"] == 1
            assert np.array_equal(one[0][0], got[0][i]) and np.array_equal(one[1][0], got[1][i]) and one[2][0] == got[2][i]
    assert not np.array_equal(cold[0], eng.breakpoint_vectors(Ys, Us)[0])      # the two paths are different arithmetic
    for call, arg in ((eng.round_Y, Yr), (eng.left_singular, Xs)):
        got = call(arg)
        st = eng.plain_multi_stats()
        assert st["calls"] == 3 and st["exhausted"] == 0, st
        again = call(arg)
        for i in range(3):
            assert np.array_equal(got[i], again[i]) and np.array_equal(call([arg[i]])[0], got[i])
    assert eng.cone_multi_stats()["calls"] == clip_calls       # counters of their own
    eng.tuning_set(KNOB, None)
    back = eng.breakpoint_vectors(Ys, Us)
    assert eng.plain_multi_stats()["calls"] == 0 and all(np.array_equal(a, b) for a, b in zip(cold, back))
    with pytest.raises(Exception):
        eng.tuning_set("OMC_PLAIN_MULTI_MINIMUM", "145")       # a misspelt knob is refused
    eng.close()


# ---- 6. inside a solve ------------------------------------------------------------------------------------------------------------------------
def _solve(omc, A, mask, nodes, knobs, **params):
    e = omc.Engine(A, mask, 80.0, 1)
    for name, val in knobs.items():
        e.tuning_set(name, val)
    P = omc.default_params(rho_scale=4.0, slots=2, breakpoints=omc.BREAKPOINTS["smallest_1_eigvec"], **(params or dict(max_iters=50)))
    out = e.matrix_completion_SDP_relaxation(nodes, "linear", params=P)
    st, mw = e.plain_multi_stats(), e.cone_multi_stats()
    st["async_harvests"] = e.host_phases()["async_harvests"]["count"]
    e.close()
    return out, st, mw


def _same_nodes(a, b, keys):
    for ra, rb_ in zip(a, b):
        for q in keys:
            assert np.array_equal(np.asarray(ra[q]), np.asarray(rb_[q])), q


def test_inside_a_solve(have_gpu, omc, orc):
    """160 x 170, rank 1, a root and its two children through 2 slots, 50 iterations each, no tracked block (sep_done is never set): the
    separation launch of the harvest on the new path (arm A) against the cold kernel (arm B).  Those three nodes all run to the cap, so a
    slot never finishes beside a live one and every harvest is synchronous.  The asynchronous harvest is therefore taken on seven nodes
    (with the four grandchildren) under eps_gap = 1e-4, checks every 10 iterations and a cap of 200: two nodes certify early (140 and 160
    iterations), the slots go out of step while nodes are pending, and with OMC_HARVEST_ASYNC_MIN_LIVE = 1 the plain launches of six
    harvests run beside the live slot's k_mw_round interval; the same solve with OMC_HARVEST_ASYNC = 0 is the synchronous arm."""
    n, m = 160, 170
    A, mask = orc.make_instance(n, m, 1, n_indices=int(0.2 * n * m), seed=0, noise=0.05)
    base = {"OMC_NO_SUBSPACE": "1", "OMC_CONE_MULTI_MIN": "145"}
    root = _solve(omc, A, mask, [[]], base)[0][0]
    nodes = [[]] + omc.pkg.bnb.make_children([], root, "linear", 1)
    assert len(nodes) == 3
    a, st_a, mw_a = _solve(omc, A, mask, nodes, dict(base, **{KNOB: "145"}))
    b, st_b, mw_b = _solve(omc, A, mask, nodes, base)
    print("plain_multi solve: arm A", st_a, "arm B", st_b, "iters", [r["iters"] for r in a])
    assert st_a["calls"] == 3 and st_a["exhausted"] == 0 and st_a["device_us"] == 0 and st_a["async_harvests"] == 0, st_a
    assert st_b["calls"] == 0, st_b
    assert mw_a["calls"] > 0 and mw_a["calls"] == mw_b["calls"], (mw_a, mw_b)
    _same_nodes(a, b, ("iters", "objective", "dual_bound", "X", "Y", "U"))
    stats = {}
    for q, (ra, rb_) in enumerate(zip(a, b)):
        M = R.sep_matrix(ra["Y"], ra["U"])
        lam, _ = R.rayleigh_eigvals(R.sep_matrix_ld(ra["Y"], ra["U"]))
        ref = dict(e=R.reference_error(M, lam)[0], fro=R.fro(M))
        for arm, r in (("A", ra), ("B", rb_)):
            ev, x = r["lambda_min"], r["breakpoint_vec"]
            d = max(abs(LD(ev[0]) - lam[0]), abs(LD(ev[1]) - lam[1]))
            res = float(np.linalg.norm(M @ x - ev[0] * x))
            stats["eig_" + arm] = max(stats.get("eig_" + arm, 0.0), _ratio(d, ref["e"]))
            stats["res_" + arm] = max(stats.get("res_" + arm, 0.0), res / _rb(n, ref))
            assert d <= 4.0 * ref["e"], (q, arm, float(d), ref["e"])
            assert res <= _rb(n, ref), (q, arm, res, _rb(n, ref))
            assert abs(np.linalg.norm(x) - 1.0) <= 8 * R.U_RND * math.sqrt(n), (q, arm)
    _report("solve", n, stats)
    mk = omc.pkg.bnb.make_children
    seven = nodes + mk(nodes[1], a[1], "linear", 1) + mk(nodes[2], a[2], "linear", 1)
    assert len(seven) == 7
    stagger = dict(max_iters=200, check_every=10, eps_gap=1e-4)
    c, st_c, _ = _solve(omc, A, mask, seven, dict(base, **{KNOB: "145", "OMC_HARVEST_ASYNC": "0"}), **stagger)
    d, st_d, _ = _solve(omc, A, mask, seven, dict(base, **{KNOB: "145", "OMC_HARVEST_ASYNC_MIN_LIVE": "1"}), **stagger)
    print("plain_multi solve: synchronous", st_c, "asynchronous", st_d, "iters", [r["iters"] for r in d])
    assert len({r["iters"] for r in c}) > 1, "the nodes finish in step: no slot is harvested beside a live one"
    assert st_c["calls"] == 7 and st_c["exhausted"] == 0 and st_c["async_harvests"] == 0, st_c
    assert st_d["calls"] == 7 and st_d["exhausted"] == 0 and st_d["async_harvests"] >= 1, st_d
    _same_nodes(c, d, ("iters", "status_code", "objective", "dual_bound", "X", "Y", "U", "lambda_min", "breakpoint_vec"))


# ---- 7. argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_with_the_knob_lowered(have_gpu, omc):
    n, m, k = 145, 147, 2
    eng = _multi_engine(omc, n, m, k)
    lib = omc.load()
    Y, Uu = R.sep_input("a", n, k, 5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    Yb = np.ascontiguousarray(Y.ravel(order="F")); Ub = np.ascontiguousarray(Uu.ravel(order="F")); Xb = np.zeros(n * m)
    ev = np.zeros(2); x = np.zeros(n); fe = np.zeros(1, np.int32); Uo = np.zeros(n * k)
    before = eng.breakpoint_vectors([Y], [Uu])
    assert eng.plain_multi_stats()["calls"] == 1
    for B in (0, -1):
        assert lib.omc_separation_batch(eng._h, B, 1, p(Yb), p(Ub), p(ev), p(x), p(fe)) == ERR_ARGUMENT
        assert lib.omc_round_Y_batch(eng._h, B, p(Yb), p(Uo)) == ERR_ARGUMENT
        assert lib.omc_left_singular_batch(eng._h, B, p(Xb), p(Uo)) == ERR_ARGUMENT
    assert lib.omc_separation_batch(eng._h, 1, 7, p(Yb), p(Ub), p(ev), p(x), p(fe)) == -1      # OMC_ERR_INVALID_ENUM
    after = eng.breakpoint_vectors([Y], [Uu])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert len(eng.round_Y([Y])) == 1 and len(eng.left_singular([np.ones((n, m))])) == 1
    eng.close()
