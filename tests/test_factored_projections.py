"""Factored W1: after an accepted k_cone_sub<0> call, k_global forms the entries of W1 = clip(Y - D1, 0, 1) from the call's Ritz pairs
instead of reading a dense W1, and no longer stores Yp.  It repeats the dense rebuild's arithmetic, so every result is bit-identical with
the factored path on and off (OMC_DENSE_PROJ=1: dense W1 and the Yp store), and across repeated runs."""
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
        return eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False, **kw)
    finally:
        for k_ in env:
            eng.tuning_set(k_, None)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x["objective"], x["dual_bound"], x["iters"], x["status_code"]) == (y["objective"], y["dual_bound"], y["iters"], y["status_code"])
        assert np.array_equal(x["Y"], y["Y"]) and np.array_equal(x["U"], y["U"])


DENSE = {"OMC_DENSE_PROJ": "1"}


def test_config2_frontier_cold_and_warm(have_gpu, omc):
    A, mask, gamma, _ = omc.pkg.data.config_instance(2, seed=0)
    eng = omc.Engine(A, mask, gamma, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    nodes, _ = omc.pkg.bnb.expand_frontier(eng, 3, "linear", params=omc.default_params(rho_scale=4.0))
    a = _run(eng, nodes, P, {})
    _same(a, _run(eng, nodes, P, DENSE))
    _same(a, _run(eng, nodes, P, {}))
    # warm-started from the parents' final states (state pool)
    Pw = omc.default_params(rho_scale=4.0)
    eng.state_pool_create(len(nodes))
    _run(eng, nodes, Pw, {}, save_to=list(range(len(nodes))))
    kids, lf = [], []
    for i, (cuts, o) in enumerate(zip(nodes, a)):
        for c in omc.pkg.bnb.make_children(cuts, o, "linear", 1):
            kids.append(c); lf.append(i)
    w = _run(eng, kids, Pw, {}, load_from=lf)
    _same(w, _run(eng, kids, Pw, DENSE, load_from=lf))
    _same(w, _run(eng, kids, Pw, {}, load_from=lf))
    eng.close()


def test_slots_switch_between_block_and_full_kernel(have_gpu, omc):
    """A step cap of 2 makes many k_cone_sub calls fail: those slots take the full kernel (dense W1) in the same launches as the
    accepted ones (factored W1)."""
    A, mask, gamma, _ = omc.pkg.data.config_instance(2, seed=0)
    eng = omc.Engine(A, mask, gamma, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=400, eps_gap=1e-14)
    nodes, _ = omc.pkg.bnb.expand_frontier(eng, 2, "linear", params=omc.default_params(rho_scale=4.0))
    env = {"OMC_SUB_QMAX": "2"}
    a = _run(eng, nodes, P, env)
    _same(a, _run(eng, nodes, P, {**env, **DENSE}))
    _same(a, _run(eng, nodes, P, env))
    eng.close()


def test_nodes_beyond_16_row_functionals(have_gpu, omc):
    """Nodes with 20 cuts (r = 20 row functionals: k_small's scalar path) beside nodes with one cut in the same batch."""
    A, mask, gamma, _ = omc.pkg.data.config_instance(2, seed=0)
    n = A.shape[0]
    eng = omc.Engine(A, mask, gamma, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=200, eps_gap=1e-14)
    root = eng.matrix_completion_SDP_relaxation([[]], "linear", params=omc.default_params(rho_scale=4.0))[0]
    rng = np.random.default_rng(11)
    U = np.array(root["U"])
    deep = []
    for s in range(3):
        cuts = []
        for t in range(20):
            x = rng.standard_normal(n); x /= np.linalg.norm(x)
            cuts.append((x, U, ["left" if (t + s) % 2 else "right"]))
        deep.append(cuts)
    nodes = deep + omc.pkg.bnb.make_children([], root, "linear", 1)
    a = _run(eng, nodes, P, {})
    _same(a, _run(eng, nodes, P, DENSE))
    _same(a, _run(eng, nodes, P, {}))
    eng.close()


def test_rank2_instance_and_oracle(have_gpu, omc, orc):
    n, m, k = 60, 70, 2
    A, mask = omc.pkg.data.generate_matrix_completion_data(k, n, m, int(0.35 * n * m), seed=4)
    eng = omc.Engine(A, mask, GAMMA, k)
    inst = orc.Instance(A, mask, GAMMA, k)
    P = omc.default_params(rho_scale=4.0)
    got = _run(eng, [[]], P, {})
    ref = orc.sdp_relaxation(inst, [], "linear", params=orc.RelaxParams(rho_scale=4.0), want_certificate=False)
    assert got[0]["objective"] == pytest.approx(ref["objective"], rel=2e-6)
    _same(got, _run(eng, [[]], P, DENSE))
    kids = omc.pkg.bnb.make_children([], got[0], "linear", k)
    Pf = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    a = _run(eng, kids, Pf, {})
    _same(a, _run(eng, kids, Pf, DENSE))
    _same(a, _run(eng, kids, Pf, {}))
    eng.close()
