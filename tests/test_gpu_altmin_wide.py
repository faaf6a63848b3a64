"""GPU tests of alternating_minimization at ranks 5 - 8 (k_altmin_w) and of its time_limit, which all three altmin kernels enforce at
iteration granularity on the device's clock.  Run on the MI355X box: `pytest -m gpu`.

Instances: orc.make_instance(n, m, k, seed=70 + k, kind="lowrank", n_indices=int(frac n m)), gamma 80; (k, cut type, n, m, frac) =
(5, linear, 16, 22, 0.7), (6, linear2, 16, 22, 0.7), (8, linear3, 20, 26, 0.75): the smallest shapes with n_indices >= (n + m) k.  Node sets
and starts are those of test_altmin_rank_k_matches_oracle (no cut / one cut / two cuts with a perturbed start), max_iters = 12.

Tolerances are those of the rank <= 3 comparison with the numpy oracle (objectives rtol 1e-8, U V atol 1e-5, equal n_iters / converged):
perturbing the oracle's finite-difference step (1e-7 -> 1.7e-7) and the rounding of its row inverses moves its objectives by <= 2e-13
relative and U V by <= 3e-13 at these ranks, so the kernel's different summation orders (constraint values from the Gram matrix U'U,
right-looking Cholesky) are about five orders below them.  The oracle results are computed once per module and only read."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GAMMA = 80.0
CASES = [(5, "linear", 16, 22, 0.7), (6, "linear2", 16, 22, 0.7), (8, "linear3", 20, 26, 0.75)]
MAX_ITERS = 12
# eps of the convergence-branch test per rank, placed between two consecutive relative steps of the oracle's run with > 10 % to either
# (k = 5: 7.9e-2 | 4.27e-2 at iteration 6; k = 6: 6.3e-2 | 4.52e-2 at iteration 7; k = 8: 3.46e-2 | 2.66e-2 at iteration 11)
EPS_LOOSE = {5: 5e-2, 6: 5.4e-2, 8: 3.0e-2}


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


class Case:
    pass


_cases = {}


def _case(orc, k):
    """instance, starts and node sets of one rank; oracle runs are added by _oracle and kept"""
    if k in _cases:
        return _cases[k]
    _, cut_type, n, m, frac = next(c for c in CASES if c[0] == k)
    c = Case()
    c.k, c.cut_type, c.n, c.m = k, cut_type, n, m
    c.A, c.mask = orc.make_instance(n, m, k, seed=70 + k, kind="lowrank", n_indices=int(frac * n * m))
    c.inst = orc.Instance(c.A, c.mask, GAMMA, k)
    c.U0 = orc.svd_rounding(np.where(c.mask, c.A, 0.0), k)
    rng = np.random.default_rng(2)
    dirs = orc.child_directions(cut_type, k)
    x1 = np.linalg.qr(rng.standard_normal((n, 1)))[0][:, 0]; x2 = np.linalg.qr(rng.standard_normal((n, 1)))[0][:, 0]
    c.node_sets = [[], [(x1, c.U0 * 0.6, list(dirs[1]))], [(x1, c.U0 * 0.6, list(dirs[-1])), (x2, -c.U0 * 0.3, list(dirs[0]))]]
    c.starts = [c.U0, c.U0, c.U0 + 0.05 * rng.standard_normal((n, k))]
    c.oracle = {}
    _cases[k] = c
    return c


def _oracle(orc, c, node, max_iters=MAX_ITERS, eps=1e-5):
    key = (node, max_iters, eps)
    if key not in c.oracle:
        c.oracle[key] = orc.alternating_minimization(c.inst, c.starts[node], c.node_sets[node], c.cut_type, eps=eps, max_iters=max_iters)
    return c.oracle[key]


def _assert_matches(orc, c, g, r):
    """the comparison of test_altmin_rank_k_matches_oracle, plus the master objective from the factors"""
    n, k = c.n, c.k
    W, rad = orc.quadratic_constraint_vectors(k)
    assert g["converged"] == r["converged"] and g["n_iters"] == r["n_iters"]
    assert len(g["objectives"]) == len(r["objectives"])
    assert np.allclose(g["objectives"], r["objectives"], rtol=1e-8, atol=0.0)
    assert np.allclose(g["U"] @ g["V"], r["U"] @ r["V"], atol=1e-5, rtol=0.0)
    assert (((g["U"] @ W.T) ** 2).sum(0) - rad).max() <= 1e-9                       # balls and pair cones (OMC.jl:2029-2045, 2164-2171)
    for j in range(k):
        assert (g["U"][n - k + j:, j] >= -1e-10).all()                               # symmetry breaking (OMC.jl:1989-1996)
    assert g["master_objective"] == pytest.approx(orc.evaluate_objective(g["U"] @ g["V"], c.A, c.mask, GAMMA), rel=1e-10)


@pytest.mark.parametrize("k", [5, 6, 8])
def test_wide_rank_matches_oracle(have_gpu, omc, orc, k):
    """k_altmin_w against the oracle's alternating_minimization: 3 - 10 quadratic constraints and 8 - 29 linear rows are active in these
    cases (Newton and NNQP both work, below the 64-row cap), and the iteration cap binds (12 iterations)."""
    c = _case(orc, k)
    eng = omc.Engine(c.A, c.mask, GAMMA, k)
    got = eng.alternating_minimization(c.starts, c.node_sets, c.cut_type, max_iters=MAX_ITERS)
    eng.close()
    for node, g in enumerate(got):
        r = _oracle(orc, c, node)
        print("k", k, "node", node, "n_iters", g["n_iters"], r["n_iters"], "objective", g["objectives"][-1:], r["objectives"][-1:],
              "max|UV - UV_oracle|", float(np.abs(g["U"] @ g["V"] - r["U"] @ r["V"]).max()))
        _assert_matches(orc, c, g, r)


@pytest.mark.parametrize("k", [5, 6, 8])
def test_wide_rank_convergence_branch(have_gpu, omc, orc, k):
    """a loose eps on the no-cut cases: the oracle's relative steps fall to 1.0e-2 .. 2.0e-2 by iteration 12, so the eps rule (OMC.jl:2235)
    ends each run inside the cap with converged = true; the relative steps at and before the stopping iteration are printed and must not
    sit within 10 % of eps (a rounding difference could otherwise flip the stop)."""
    c = _case(orc, k)
    eps = EPS_LOOSE[k]
    r = _oracle(orc, c, 0, eps=eps)
    o = r["objectives"]
    step = abs((o[-1] - o[-2]) / o[-2])
    prev = abs((o[-2] - o[-3]) / o[-3])
    print("k", k, "eps", eps, "oracle stops at", r["n_iters"], "relative step", step, "the one before", prev)
    assert r["converged"] and 3 <= r["n_iters"] < MAX_ITERS and step < 0.9 * eps and prev > 1.1 * eps
    eng = omc.Engine(c.A, c.mask, GAMMA, k)
    g = eng.alternating_minimization([c.starts[0]], [[]], c.cut_type, eps=eps, max_iters=MAX_ITERS)[0]
    eng.close()
    assert g["converged"] is True
    _assert_matches(orc, c, g, r)


def test_wide_rank_failure_branch(have_gpu, omc, orc):
    """contradictory cut bounds at k = 5: model_U has no solution, the loop ends in its first iteration with converged = false and no
    objective (OMC.jl:2231, 2263-2265); the same start without cuts runs as the oracle does"""
    k, n, m = 5, 16, 22
    A, mask = orc.make_instance(n, m, k, seed=75, kind="lowrank", n_indices=int(0.7 * n * m))
    inst = orc.Instance(A, mask, GAMMA, k)
    U0 = orc.svd_rounding(np.where(mask, A, 0.0), k)
    x = np.zeros(n); x[0] = 1.0
    Uh = np.zeros((n, k)); Uh[0, :] = 0.5
    cuts = [(x, Uh, ["right"] * k), (x, -Uh, ["left"] * k)]
    eng = omc.Engine(A, mask, GAMMA, k)
    got = eng.alternating_minimization([U0, U0], [cuts, []], "linear", max_iters=MAX_ITERS)
    eng.close()
    r = orc.alternating_minimization(inst, U0, cuts, "linear", max_iters=MAX_ITERS)
    assert (r["converged"], r["n_iters"], len(r["objectives"])) == (False, 1, 0)
    assert (got[0]["converged"], got[0]["n_iters"], len(got[0]["objectives"])) == (False, 1, 0)
    r = orc.alternating_minimization(inst, U0, [], "linear", max_iters=MAX_ITERS)
    assert got[1]["converged"] == r["converged"] and got[1]["n_iters"] == r["n_iters"]
    assert np.allclose(got[1]["objectives"], r["objectives"], rtol=1e-8, atol=0.0)


def test_wide_rank_lds_and_slab_variants_agree(have_gpu, omc, orc):
    """the k = 5 case in dynamic LDS and on the per-problem global slab (OMC_ALTMIN_NOLDS): the same code on another address space, bit-identical"""
    c = _case(orc, 5)
    eng = omc.Engine(c.A, c.mask, GAMMA, 5)
    assert eng.altmin_plan(max_cuts=2)["lds_bytes"] > 0 and eng.altmin_plan(max_cuts=2, nolds=True)["slab_bytes"] > 0
    a = eng.alternating_minimization(c.starts, c.node_sets, c.cut_type, max_iters=MAX_ITERS)
    eng.tuning_set("OMC_ALTMIN_NOLDS", "1")
    try:
        b = eng.alternating_minimization(c.starts, c.node_sets, c.cut_type, max_iters=MAX_ITERS)
    finally:
        eng.tuning_set("OMC_ALTMIN_NOLDS", None)
    eng.close()
    for g, h in zip(a, b):
        assert g["n_iters"] == h["n_iters"] and g["converged"] == h["converged"] and g["n_iters"] == MAX_ITERS
        assert np.array_equal(g["objectives"], h["objectives"]) and g["master_objective"] == h["master_objective"]
        assert np.array_equal(g["U"], h["U"]) and np.array_equal(g["V"], h["V"])


def _assert_prefix(g, full, max_iters):
    """a run the clock stopped is the unlimited run of the same kernel, cut after n_iters iterations"""
    ni = g["n_iters"]
    assert 1 <= ni <= max_iters
    assert len(g["objectives"]) == ni or (ni == full["n_iters"] and len(g["objectives"]) == len(full["objectives"]))
    assert np.allclose(g["objectives"], full["objectives"][:len(g["objectives"])], rtol=1e-12, atol=0.0)
    if ni < full["n_iters"]:
        assert g["converged"] is False


def test_time_limit_rank8(have_gpu, omc, orc):
    """time_limit inside the launch (OMC.jl:2186-2189).  (a) 1 us: the stamp is taken right before the first check, so the first iteration
    runs, and one iteration (dozens of workgroup barriers and dependent memory round trips) is far above a microsecond: exactly one
    iteration, equal to the oracle's max_iters = 1.  (b) a quarter of the unlimited call's solve_time: wherever the clock cuts, the run is
    a prefix of the unlimited one and its factors are the oracle's after the same number of iterations."""
    c = _case(orc, 8)
    eng = omc.Engine(c.A, c.mask, GAMMA, 8)
    full = eng.alternating_minimization([c.starts[0]], [[]], c.cut_type, max_iters=40)[0]
    one = eng.alternating_minimization([c.starts[0]], [[]], c.cut_type, max_iters=40, time_limit=1e-6)[0]
    part = eng.alternating_minimization([c.starts[0]], [[]], c.cut_type, max_iters=40, time_limit=0.25 * full["solve_time"])[0]
    eng.close()
    print("unlimited: n_iters", full["n_iters"], "solve_time", full["solve_time"], "; quarter of it: n_iters", part["n_iters"])
    assert one["n_iters"] == 1 and one["converged"] is False and len(one["objectives"]) == 1
    r1 = _oracle(orc, c, 0, max_iters=1)
    assert len(r1["objectives"]) == 1 and r1["converged"] is False
    _assert_matches(orc, c, one, r1)
    _assert_prefix(one, full, 40)
    _assert_prefix(part, full, 40)
    rp = _oracle(orc, c, 0, max_iters=part["n_iters"])
    assert np.allclose(part["U"] @ part["V"], rp["U"] @ rp["V"], atol=1e-5, rtol=0.0)
    assert part["master_objective"] == pytest.approx(orc.evaluate_objective(part["U"] @ part["V"], c.A, c.mask, GAMMA), rel=1e-10)


@pytest.mark.parametrize("k,n,m", [(1, 30, 40), (2, 16, 22)])
def test_time_limit_reaches_the_narrow_kernels(have_gpu, omc, orc, k, n, m):
    """the same two properties through k_altmin (k = 1) and k_altmin_k (k = 2)"""
    A, mask = orc.make_instance(n, m, k, seed=90 + k, kind="lowrank", n_indices=int(0.5 * n * m))
    inst = orc.Instance(A, mask, GAMMA, k)
    U0 = orc.svd_rounding(np.where(mask, A, 0.0), k)
    eng = omc.Engine(A, mask, GAMMA, k)
    full = eng.alternating_minimization([U0], [[]], "linear", max_iters=40)[0]
    one = eng.alternating_minimization([U0], [[]], "linear", max_iters=40, time_limit=1e-6)[0]
    part = eng.alternating_minimization([U0], [[]], "linear", max_iters=40, time_limit=0.25 * full["solve_time"])[0]
    eng.close()
    print("k", k, "unlimited n_iters", full["n_iters"], "solve_time", full["solve_time"], "quarter:", part["n_iters"])
    assert full["n_iters"] > 1
    assert one["n_iters"] == 1 and one["converged"] is False and len(one["objectives"]) == 1
    for g in (one, part):
        _assert_prefix(g, full, 40)
        r = orc.alternating_minimization(inst, U0, [], "linear", max_iters=g["n_iters"])
        assert np.allclose(g["U"] @ g["V"], r["U"] @ r["V"], atol=1e-5, rtol=0.0)
        assert g["master_objective"] == pytest.approx(orc.evaluate_objective(g["U"] @ g["V"], A, mask, GAMMA), rel=1e-10)


def test_driver_runs_at_rank_5(have_gpu, omc, orc):
    """bnb.branch_and_bound with altmin at k = 5 (root only): the incumbent is evaluate_objective of a rank-5 X"""
    c = _case(orc, 5)
    eng = omc.Engine(c.A, c.mask, GAMMA, 5)
    sol, inst = omc.pkg.bnb.branch_and_bound(eng, c.A, c.mask, root_only=True, altmin_flag=True)
    eng.close()
    assert sol["objective"] == pytest.approx(orc.evaluate_objective(sol["X"], c.A, c.mask, GAMMA), rel=1e-10)
    assert np.linalg.matrix_rank(sol["X"], tol=1e-8) <= 5
