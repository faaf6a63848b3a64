"""k_cone_sub after the residency bound and the shorter per-call chain: two workgroups per CU as the runtime reports them, and the
tile shapes at which the kernel's index walks change (three row tiles: wave 3 owns none; five: only wave 0 holds a second tile, ragged
padding rows; seven: config 2; ten: the third accumulator, nt > 8, beside the L2-resident full kernel).  The power steps of a chunk
alternate between the X and the Z block with the rescale in the tile store, so the accepted path, the fail / back-off path
(OMC_SUB_QMAX=2) and the separation vector from the block (k_cone_sub<2>) are each run at such a shape.

Seeds: the four shapes are seed 0 of the instance generator, the separation instance seed 3 as in its model in test_gpu_parity.py; no
other seed was tried.  The parent library was run on the same instances with the same nodes (both libraries in child processes of their
own, profiles/r11_cone_sub_chain.txt section 3): its calls / fall-backs are recorded in the tests' docstrings, well inside the cap of
one half, and every array of every arm was np.array_equal between the two libraries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0
# (n, m, observed cells); np16 = 48, 80, 112, 160.  n = 100 is config 2 (20 % observed).
SHAPES = {48: (48, 52, 874), 70: (70, 72, 1512), 100: (100, 100, 2000), 150: (150, 150, 3375)}
DENSE = {"OMC_DENSE_PROJ": "1"}
FULL = {"OMC_NO_SUBSPACE": "1"}


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
        return eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False, **kw)
    finally:
        for k_ in env:
            eng.tuning_set(k_, None)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x["objective"], x["dual_bound"], x["iters"], x["status_code"]) == (y["objective"], y["dual_bound"], y["iters"], y["status_code"])
        assert np.array_equal(x["Y"], y["Y"]) and np.array_equal(x["U"], y["U"])


def _family(omc, n):
    """Engine, the root and its two children, all three warm-started from the root's final state in the pool."""
    n_, m, nidx = SHAPES[n]
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, n_, m, nidx, seed=0)
    eng = omc.Engine(A, mask, GAMMA, 1)
    eng.state_pool_create(1)
    root = _run(eng, [[]], omc.default_params(rho_scale=4.0, max_iters=1500), {}, save_to=[0])[0]
    nodes = [[]] + omc.pkg.bnb.make_children([], root, "linear", 1)
    return eng, nodes, [0] * len(nodes)


def test_residency_two_workgroups_per_cu(have_gpu, omc):
    """What the HIP runtime grants at config 2's geometry, dynamic LDS included: k_cone_sub lost its second workgroup once without a
    test noticing (the compiler took the 512-register budget of one wave per SIMD)."""
    A, mask, gamma, _ = omc.pkg.data.config_instance(2, seed=0)
    eng = omc.Engine(A, mask, gamma, 1)
    with pytest.raises(omc.OmcError):
        eng.kernel_residency()                                  # the geometry is planned when a batch is staged
    _run(eng, [[]], omc.default_params(rho_scale=4.0, max_iters=25), {})
    res = eng.kernel_residency()
    print("residency", res)
    for name in ("k_cone_sub<0>", "k_cone_sub<1>", "k_cone_sub<2>", "k_global", "k_small", "k_colprox_pair", "k_colprox_wide", "k_colprox", "k_cone_ws", "k_cone"):
        assert name in res
    assert res["k_cone_sub<0>"] >= 2 and res["k_cone_sub<1>"] >= 2 and res["k_cone_sub<2>"] >= 2
    assert res["k_global"] >= 2
    assert res["k_small"] >= 1 and res["k_colprox_pair"] >= 1 and res["k_cone_ws"] >= 1
    info = eng.solver_info()                                    # unchanged shape: bench.py reads it
    assert set(info) == {"solve_seconds", "jacobi_sweeps", "rho", "r_max", "cone_lds", "global_lds", "small_lds", "R_max"}
    eng.close()


@pytest.mark.parametrize("n", [48, 70, 100, 150])
def test_tile_shapes(have_gpu, omc, n):
    """Default arm = its repeat = OMC_DENSE_PROJ=1 bit for bit at 300 iterations; against the full decomposition every iteration
    (OMC_NO_SUBSPACE=1) the certified solves bracket each other: a dual bound is a lower bound of the node's optimum and a certified
    objective is within eps_gap of it, so neither arm's bound may exceed the other's objective by more than that slack (the form and
    the 1e-6 = eps_gap of test_order_200_l2_resident_variants_agree in test_gpu_parity.py).
    Parent library, default arm, calls / fall-backs: n = 48: 745 / 2, n = 70: 660 / 2, n = 100: 823 / 1, n = 150: 825 / 0; all three nodes
    certified in both arms at every shape."""
    eng, nodes, lf = _family(omc, n)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    a = _run(eng, nodes, P, {}, load_from=lf)
    st = eng.subspace_stats()
    print("n", n, "iters", [o["iters"] for o in a], "subspace", st)
    assert st["calls"] > 0
    assert 2 * st["fallbacks"] < st["calls"], st
    _same(a, _run(eng, nodes, P, {}, load_from=lf))
    _same(a, _run(eng, nodes, P, DENSE, load_from=lf))
    Pc = omc.default_params(rho_scale=4.0)
    blk = _run(eng, nodes, Pc, {}, load_from=lf)
    full = _run(eng, nodes, Pc, FULL, load_from=lf)
    assert eng.subspace_stats()["calls"] == 0                   # the full arm really ran without the block
    print("n", n, "block", [(o["status_code"], o["iters"], o["objective"], o["dual_bound"]) for o in blk])
    print("n", n, "full ", [(o["status_code"], o["iters"], o["objective"], o["dual_bound"]) for o in full])
    pairs = 0
    for x, y in zip(blk, full):
        if x["status_code"] == 0 and y["status_code"] == 0:
            pairs += 1
            assert x["dual_bound"] <= y["objective"] * (1 + 1e-6)
            assert y["dual_bound"] <= x["objective"] * (1 + 1e-6)
    assert pairs >= 1
    eng.close()


def test_fail_and_back_off_under_the_new_buffer_roles(have_gpu, omc):
    """A step cap of 2 at n = 70 (five row tiles): calls fail on the cap, back off and are re-seeded by the full kernel, in the same
    launches as accepted ones; the factored and the dense arm and a repeat stay bit-identical.  Parent library, seed 0: 603 calls, 8 of them
    failed on the cap, 65 seedings by the full kernel."""
    eng, nodes, lf = _family(omc, 70)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    env = {"OMC_SUB_QMAX": "2"}
    a = _run(eng, nodes, P, env, load_from=lf)
    st = eng.subspace_stats()
    print("qmax 2:", st)
    assert st["calls"] > 0 and st["fail_steps"] > 0 and st["seeds"] > 0 and st["fallbacks"] < st["calls"], st
    _same(a, _run(eng, nodes, P, {**env, **DENSE}, load_from=lf))
    _same(a, _run(eng, nodes, P, env, load_from=lf))
    eng.close()


def test_separation_from_the_block_at_five_tiles(have_gpu, omc, orc):
    """k_cone_sub<2> at n = 70: the separation vector of every feasible node of a depth-3 frontier against omc_separation_batch (cold
    eigendecomposition of the returned (Y, U)): same lambda_min, same vector up to the eigen-gap, the same master-feasibility verdict."""
    A, mask = orc.make_instance(70, 72, 1, n_indices=1512, seed=3, noise=0.1, kind="lowrank")
    eng = omc.Engine(A, mask, GAMMA, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=1500)
    nodes, _ = omc.pkg.bnb.expand_frontier(eng, 3, "linear", params=P)
    out = eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False)
    st = eng.subspace_stats()
    assert st["calls"] > 0 and 2 * st["fallbacks"] < st["calls"], st          # the slots follow the block when they are harvested
    ok = [o for o in out if o["feasible"]]
    assert len(ok) >= len(nodes) // 2
    xs, lam, _ = eng.breakpoint_vectors([o["Y"] for o in ok], [o["U"] for o in ok])
    for o, xc, lc in zip(ok, xs, lam):
        assert o["lambda_min"][0] == pytest.approx(lc[0], abs=1e-7)
        assert (o["lambda_min"][0] >= -1e-6) == (lc[0] >= -1e-6)
        if lc[1] - lc[0] > 1e-4:
            assert np.allclose(o["breakpoint_vec"], xc, atol=1e-5)
    eng.close()
