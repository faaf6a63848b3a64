"""k_global's schedule (packed-triangle target assembly four entries at a time, weight division inside the Lambda Lambda' tile store, two
tiles per wave, the row projection's Gram matrix staged in LDS, the mu != 0 row lists) changes no arithmetic and no order of a sum.  So
objective, dual bound, iterations, status, Y and U are equal -- np.array_equal, tolerance zero -- between the LDS arm and the
OMC_GLOBAL_NOLDS=1 arm of the kernel, with OMC_DENSE_PROJ on and off, and across two runs, on shapes that stress the index walks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


def _run(eng, nodes, P, env, **kw):
    for k_, v in env.items():
        eng.tuning_set(k_, v)
    try:
        out = eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False, **kw)
        return out, eng.solver_info()["global_lds"]
    finally:
        for k_ in env:
            eng.tuning_set(k_, None)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x["objective"], x["dual_bound"], x["iters"], x["status_code"]) == (y["objective"], y["dual_bound"], y["iters"], y["status_code"])
        assert np.array_equal(x["Y"], y["Y"]) and np.array_equal(x["U"], y["U"])


def _all_arms(eng, nodes, P, **kw):
    """LDS arm, its repeat, OMC_DENSE_PROJ=1, OMC_GLOBAL_NOLDS=1 (and both): all equal.  Returns the LDS arm's results."""
    a, lds = _run(eng, nodes, P, {}, **kw)
    assert lds
    b, lds = _run(eng, nodes, P, {}, **kw)
    assert lds
    _same(a, b)
    d, lds = _run(eng, nodes, P, {"OMC_DENSE_PROJ": "1"}, **kw)
    assert lds
    _same(a, d)
    g, lds = _run(eng, nodes, P, {"OMC_GLOBAL_NOLDS": "1"}, **kw)
    assert not lds
    _same(a, g)
    gd, lds = _run(eng, nodes, P, {"OMC_GLOBAL_NOLDS": "1", "OMC_DENSE_PROJ": "1"}, **kw)
    assert not lds
    _same(a, gd)
    return a


def _root_and_children(omc, n, m, seed):
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, n, m, int(0.35 * n * m), seed=seed)
    eng = omc.Engine(A, mask, GAMMA, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    root = _all_arms(eng, [[]], P)
    kids = omc.pkg.bnb.make_children([], root[0], "linear", 1)
    out = _all_arms(eng, kids, P)
    assert all(o["iters"] > 0 for o in out)
    eng.close()


def test_order_32_three_tiles_and_a_triangle_below_one_trip(have_gpu, omc):
    """n = 32: a multiple of 16, 3 Lambda Lambda' tiles (odd: the one-tile remainder on every wave that works), 528 triangle entries
    < 4 x 512 (most of the four entries of a thread are out of range)."""
    _root_and_children(omc, 32, 40, seed=5)


def test_order_70_fifteen_tiles_with_a_ragged_edge(have_gpu, omc):
    """n = 70: not a multiple of 16, 15 tiles over 8 waves (seven pairs and one single), 2485 entries (a partial second trip)."""
    _root_and_children(omc, 70, 80, seed=6)


def test_config2_depth3_frontier_and_warm_children(have_gpu, omc):
    """n = 100 (28 tiles: a pair and a single on half the waves), nodes with three cuts, then their children warm-started from the state pool."""
    A, mask, gamma, _ = omc.pkg.data.config_instance(2, seed=0)
    eng = omc.Engine(A, mask, gamma, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    nodes, _ = omc.pkg.bnb.expand_frontier(eng, 3, "linear", params=omc.default_params(rho_scale=4.0))
    assert nodes and all(len(c) == 3 for c in nodes)
    a = _all_arms(eng, nodes, P)
    Pw = omc.default_params(rho_scale=4.0)
    eng.state_pool_create(len(nodes))
    _run(eng, nodes, Pw, {}, save_to=list(range(len(nodes))))
    kids, lf = [], []
    for i, (cuts, o) in enumerate(zip(nodes, a)):
        for c in omc.pkg.bnb.make_children(cuts, o, "linear", 1):
            kids.append(c); lf.append(i)
    assert kids and all(len(c) == 4 for c in kids)
    _all_arms(eng, kids, Pw, load_from=lf)
    eng.close()


def test_order_20_deep_node_keeps_the_gram_matrix_in_global_memory(have_gpu, omc):
    """n = 20, k = 1, seven cuts: Rmax = 2 + 3 x 7 = 23 rows, 23^2 = 529 > GL_XS n = 320, so the row projection reads the Gram matrix from
    global memory; the children of the root (Rmax^2 = 25 <= 320 when staged alone) take the staged copy."""
    n, m = 20, 24
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, n, m, int(0.4 * n * m), seed=7)
    eng = omc.Engine(A, mask, GAMMA, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    root = _all_arms(eng, [[]], P)[0]
    rng = np.random.default_rng(13)
    U = np.array(root["U"])
    deep = []
    for s in range(2):
        cuts = []
        for t in range(7):
            x = rng.standard_normal(n); x /= np.linalg.norm(x)
            cuts.append((x, U, ["left" if (t + s) % 2 else "right"]))
        deep.append(cuts)
    assert (2 + 3 * 7) ** 2 > 16 * n
    out = _all_arms(eng, deep, P)
    assert all(o["iters"] > 0 for o in out)
    _all_arms(eng, omc.pkg.bnb.make_children([], root, "linear", 1), P)
    eng.close()


def test_small_shor_root_keeps_its_division_pass(have_gpu, omc, orc):
    """Shor mode has no Lambda Lambda' term: the target is divided by the weights in a pass over the packed triangle."""
    A, mask = orc.make_instance(10, 12, 1, n_indices=60, seed=1, noise=0.3, kind="lowrank")
    eng = omc.Engine(A, mask, GAMMA, 1)
    P = omc.default_params(eps_gap=1e-6)
    out = _all_arms(eng, [[]], P, add_Shor_valid_inequalities=True, shor_info=[([], None)])
    assert out[0]["status_code"] == 0
    eng.close()
