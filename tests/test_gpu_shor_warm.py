"""GPU tests of the warm start of Shor-mode relaxations from a pool entry (omc_state_pool_reserve_shor, omc_relax_set_warm before
omc_relax_stage_shor).  Run on the MI355X box: `pytest -m gpu`.

Instance: 10 x 12 rank 1, 60 observed entries, seed 2, noise 0.1, gamma 80, the static class-4 list (208 minors); eps_gap 1e-5, at most
6000 iterations, rho_scale 1.  The cuts come from the oracle's Shor root and from the oracle's solution of `left`.  Every node the tests
require to certify is one the oracle alone certifies inside that cap (root 600 iterations, left 625, right 975, left.left 4100, the root
with the first 104 minors 3200, root / left at rho_scale 2: 1200 / 1250).

The Shor oracle has no warm start.  The tests rest on the uniqueness of the optimum value: two results that both carry the two-sided 1e-5
certificate of the same program differ by at most 2e-5 max(1, |objective|) (the project's "twice the certified gap" rule).  Every warm
result must also be certified (status 0, dual_bound <= objective (1 + 1e-5)) and its point must pass shor_primal_residuals at 1e-5, the
level test_gpu_shor.py uses at 1e-6 for the 1e-6 class.  Cold GPU solves are the unchanged path and the reference where the oracle
would need seconds of CPU (left.left, the penalty-2 solves).  No iteration ratio is fixed in advance (nobody had measured one): the
counts are printed and go into the failure messages; "strictly fewer" is what the tests ask."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GAMMA = 80.0
TOL = 2e-5
NQ = 208
E_ROOT, E_LEFT, E_HALF, E_BASE, E_NEVER = 0, 1, 2, 3, 5


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


@pytest.fixture(scope="module")
def sh():
    import omc_oracle_shor
    return omc_oracle_shor


def _close(a, b):
    return abs(a - b) <= TOL * max(1.0, abs(b))


def _same(a, b):
    return a["objective"] == b["objective"] and a["iters"] == b["iters"] and np.array_equal(a["X"], b["X"])


class Env:
    pass


def _solve(env, nodes, lists, load_from=None, save_to=None, params=None, want_V=False, eng=None):
    eng = eng or env.eng
    return eng.matrix_completion_SDP_relaxation(nodes, "linear", params or env.P, add_Shor_valid_inequalities=True,
                                                shor_info=[(l, None) for l in lists], want_Theta=True, want_V=want_V,
                                                load_from=load_from, save_to=save_to)


def _certified(env, r, minors, cuts, name):
    assert r["status_code"] == 0, (name, r["iters"], r["objective"], r["dual_bound"])
    assert r["dual_bound"] <= r["objective"] * (1 + 1e-5), (name, r["objective"], r["dual_bound"])
    if "V" in r:
        orc, sh = env.orc, env.sh
        st = sh.ShorStructure(env.inst.n, env.inst.m, minors, sh.driver_shor_lists(env.mask, minors=minors)[1], env.inst.indices)
        rows = orc.build_rows(env.inst, cuts, "linear")
        V = r["V"]; V1 = np.zeros(st.nv1); V2 = np.zeros(st.nv2)
        V1[st.k12] = V[:, 0]; V1[st.k34] = V[:, 1]; V2[st.k13] = V[:, 2]; V2[st.k24] = V[:, 3]
        res = sh.shor_primal_residuals(env.inst, st, rows, r["X"], r["W"], V1, V2, V[:, 4].copy(), r["Theta"], r["Y"], r["U"])
        print(f"  residuals {name}: max {res['max']:.3e}")
        assert res["max"] <= 1e-5, (name, res)


@pytest.fixture(scope="module")
def env(have_gpu, omc, orc, sh):
    """The oracle's root and `left` (computed once), the cuts, one engine whose pool holds: entry 0 the Shor root, entry 2 the root of the
    first 104 minors, entry 3 a base-mode root, entry 5 nothing; and the cold solves the tests compare against.  Tests only read these
    entries (test 1 writes entry 1)."""
    e = Env()
    e.omc, e.orc, e.sh = omc, orc, sh
    e.A, e.mask = orc.make_instance(10, 12, 1, n_indices=60, seed=2, noise=0.1)
    e.inst = orc.Instance(e.A, e.mask, GAMMA, 1)
    e.minors, e.soc = sh.driver_shor_lists(e.mask, (4,))
    assert len(e.minors) == NQ
    e.P = omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0)
    e.P2 = omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=2.0)
    op = sh.ShorParams(eps_gap=1e-5, max_iters=6000)
    e.o_root = sh.sdp_relaxation_shor(e.inst, e.minors, e.soc, params=op)
    x = orc.breakpoint_vector(e.o_root["Y"], e.o_root["U"])[0]
    e.left = [(x, e.o_root["U"], ["left"])]; e.right = [(x, e.o_root["U"], ["right"])]
    e.o_left = sh.sdp_relaxation_shor(e.inst, e.minors, e.soc, cuts=e.left, params=op)
    assert e.o_root["termination_status"] == 0 and e.o_left["termination_status"] == 0
    x2 = orc.breakpoint_vector(e.o_left["Y"], e.o_left["U"])[0]
    e.leftleft = e.left + [(x2, e.o_left["U"], ["left"])]
    e.eng = omc.Engine(e.A, e.mask, GAMMA, 1)
    e.eng.state_pool_create(6)
    e.eng.state_pool_reserve_shor(NQ)
    # cold references (no indices: the unchanged path)
    e.c_root, e.c_left, e.c_ll, e.c_right = _solve(e, [[], e.left, e.leftleft, e.right], [e.minors] * 4, want_V=True)
    e.stats_cold = e.eng.shor_warm_stats()
    # entry 0: the root, saved; the solve itself is the cold one
    e.s_root = _solve(e, [[]], [e.minors], save_to=[E_ROOT], want_V=True)[0]
    e.stats_save = e.eng.shor_warm_stats()
    e.V_root = e.s_root["V"]
    # entry 2: the root of the first 104 minors; entry 3: a base-mode root
    e.s_half = _solve(e, [[]], [e.minors[:104]], save_to=[E_HALF])[0]
    e.Pb = omc.default_params(rho_scale=4.0)
    e.b_root = e.eng.matrix_completion_SDP_relaxation([[]], "linear", e.Pb, save_to=[E_BASE])[0]
    yield e
    e.eng.close()


def test_restart_and_path(env):
    """Root restarted from its own final state; left from the root's; left.left from left's.  Each agrees with its cold twin (root and
    left also with the oracle), the restart and the warm path need strictly fewer iterations than the cold ones."""
    e = env
    assert e.stats_cold == dict(loaded_identical=0, loaded_prefix=0, refused=0, saved=0)
    assert e.stats_save == dict(loaded_identical=0, loaded_prefix=0, refused=0, saved=1)
    assert _same(e.s_root, e.c_root)                                   # saving does not change the solve
    w_root = _solve(e, [[]], [e.minors], load_from=[E_ROOT], want_V=True)[0]
    assert e.eng.shor_warm_stats() == dict(loaded_identical=1, loaded_prefix=0, refused=0, saved=0)
    w_left = _solve(e, [e.left], [e.minors], load_from=[E_ROOT], save_to=[E_LEFT], want_V=True)[0]
    assert e.eng.shor_warm_stats() == dict(loaded_identical=1, loaded_prefix=0, refused=0, saved=1)
    w_ll = _solve(e, [e.leftleft], [e.minors], load_from=[E_LEFT], want_V=True)[0]
    assert e.eng.shor_warm_stats() == dict(loaded_identical=1, loaded_prefix=0, refused=0, saved=0)
    counts = dict(root=(e.c_root["iters"], w_root["iters"]), left=(e.c_left["iters"], w_left["iters"]), leftleft=(e.c_ll["iters"], w_ll["iters"]))
    print("  iterations (cold, warm):", counts)
    for name, w, c, cuts in (("root", w_root, e.c_root, []), ("left", w_left, e.c_left, e.left), ("left.left", w_ll, e.c_ll, e.leftleft)):
        _certified(e, c, e.minors, cuts, name + " cold")
        _certified(e, w, e.minors, cuts, name + " warm")
        assert _close(w["objective"], c["objective"]), (name, w["objective"], c["objective"], counts)
    assert _close(w_root["objective"], e.o_root["objective"]) and _close(e.c_root["objective"], e.o_root["objective"]), counts
    assert _close(w_left["objective"], e.o_left["objective"]) and _close(e.c_left["objective"], e.o_left["objective"]), counts
    assert w_root["iters"] < e.c_root["iters"], counts
    assert w_left["iters"] + w_ll["iters"] < e.c_left["iters"] + e.c_ll["iters"], counts


def test_different_penalty(env):
    """The root saved at rho_scale 1 starts the root and left at rho_scale 2: the saved scaled duals are multiplied by 1/2."""
    e = env
    c = _solve(e, [[], e.left], [e.minors] * 2, params=e.P2)
    w = _solve(e, [[], e.left], [e.minors] * 2, load_from=[E_ROOT, E_ROOT], params=e.P2, want_V=True)
    assert e.eng.shor_warm_stats()["loaded_identical"] == 2
    counts = [(cc["iters"], ww["iters"]) for cc, ww in zip(c, w)]
    print("  rho_scale 2, iterations (cold, warm) of root, left:", counts)
    for name, cc, ww, cuts in (("root", c[0], w[0], []), ("left", c[1], w[1], e.left)):
        assert cc["status_code"] == 0, (name, cc["iters"])
        _certified(e, ww, e.minors, cuts, name + " warm at rho_scale 2")
        assert _close(ww["objective"], cc["objective"]), (name, ww["objective"], cc["objective"], counts)
        assert ww["iters"] < cc["iters"], (name, counts)


def test_prefix_list(env):
    """Parent: the root with the first 104 minors.  Child: the root with all 208.  One prefix load; the value is the full root's.
    Iterations are recorded, not asserted: a converged half-list state need not beat a 600-iteration cold solve."""
    e = env
    assert e.s_half["status_code"] == 0, e.s_half["iters"]
    w = _solve(e, [[]], [e.minors], load_from=[E_HALF], want_V=True)[0]
    assert e.eng.shor_warm_stats() == dict(loaded_identical=0, loaded_prefix=1, refused=0, saved=0)
    print("  prefix 104 -> 208: iterations cold", e.c_root["iters"], "warm", w["iters"], "(parent", e.s_half["iters"], ")")
    _certified(e, w, e.minors, [], "prefix child")
    assert _close(w["objective"], e.c_root["objective"]), (w["objective"], e.c_root["objective"])
    assert _close(w["objective"], e.o_root["objective"]), (w["objective"], e.o_root["objective"])


def test_refusals(env, omc):
    e = env
    sub = e.minors[50:150]
    c_sub = _solve(e, [[]], [sub])[0]
    r = _solve(e, [[]], [sub], load_from=[E_HALF])[0]                  # neither identical nor a prefix
    assert e.eng.shor_warm_stats()["refused"] == 1 and _same(r, c_sub)
    r = _solve(e, [[]], [e.minors], load_from=[E_NEVER])[0]            # never saved
    assert e.eng.shor_warm_stats()["refused"] == 1 and _same(r, e.c_root)
    r = _solve(e, [[]], [e.minors], load_from=[E_BASE])[0]             # saved by a base-mode stage
    assert e.eng.shor_warm_stats()["refused"] == 1 and _same(r, e.c_root)
    assert e.eng.shor_warm_stats()["loaded_identical"] == 0
    # the base engine refuses a Shor-mode entry in the same way
    rb = e.eng.matrix_completion_SDP_relaxation([[]], "linear", e.Pb, load_from=[E_ROOT])[0]
    assert _same(rb, e.b_root)
    # without the reservation the indices are ignored exactly as before
    eng2 = omc.Engine(e.A, e.mask, GAMMA, 1)
    with pytest.raises(omc.OmcError) as err:
        eng2.state_pool_reserve_shor(NQ)                               # no pool
    assert err.value.code == -3
    eng2.state_pool_create(2)
    with pytest.raises(omc.OmcError) as err:
        eng2.state_pool_reserve_shor(-1)
    assert err.value.code == -3
    plain = _solve(e, [[]], [e.minors], eng=eng2)[0]
    a = _solve(e, [[]], [e.minors], save_to=[0], eng=eng2)[0]
    b = _solve(e, [[]], [e.minors], load_from=[0], eng=eng2)[0]
    assert _same(a, plain) and _same(b, plain) and _same(plain, e.c_root)
    assert eng2.shor_warm_stats() == dict(loaded_identical=0, loaded_prefix=0, refused=0, saved=0)
    with pytest.raises(omc.OmcError) as err:
        eng2.state_pool_fetch_shor(0)
    assert err.value.code == -3
    eng2.close()


def test_slots(env):
    """Six nodes through two slots, three of them warm from entry 0: every node's result is that of the same node solved alone with the
    same entry -- a relaxation does not depend on its slot or on the moment it starts."""
    e = env
    nodes = [e.left, e.right, [], e.left, e.right, []]
    lf = [E_ROOT, E_ROOT, E_ROOT, -1, -1, -1]
    p2 = e.omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0, slots=2)
    out = _solve(e, nodes, [e.minors] * 6, load_from=lf, params=p2)
    assert e.eng.shor_warm_stats() == dict(loaded_identical=3, loaded_prefix=0, refused=0, saved=0)
    for i, (nd, l) in enumerate(zip(nodes, lf)):
        alone = _solve(e, [nd], [e.minors], load_from=[l])[0]
        assert _same(out[i], alone), (i, out[i]["iters"], alone["iters"], out[i]["objective"], alone["objective"])
    assert _same(out[3], e.c_left) and _same(out[4], e.c_right) and _same(out[5], e.c_root)


def test_saved_point_is_the_returned_point(env):
    e = env
    f = e.eng.state_pool_fetch_shor(E_ROOT)
    assert f["nq"] == NQ
    for got, want in ((f["X"], e.s_root["X"]), (f["Theta"], e.s_root["Theta"]), (f["V"], e.V_root)):
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert e.eng.state_pool_fetch_shor(E_HALF)["nq"] == 104
    for entry in (E_BASE, E_NEVER):
        with pytest.raises(e.omc.OmcError) as err:
            e.eng.state_pool_fetch_shor(entry)
        assert err.value.code == -3


def test_driver_with_shor_warm_start(have_gpu, omc, orc):
    """branch_and_bound with shor_warm_start on the 12 x 14 instance of test_branch_and_bound_with_shor_inequalities, static and iterative:
    the invariants that test checks, at least one accepted load whenever a node below the root was relaxed, and the root bound of the
    run without warm starts."""
    A, mask = orc.make_instance(12, 14, 1, n_indices=70, seed=2, noise=0.1)
    eng = omc.Engine(A, mask, GAMMA, 1)
    bnb = omc.pkg.bnb
    sp = omc.default_params(rho_scale=1.0, eps_gap=1e-5, max_iters=4000)
    for kw in (dict(add_Shor_valid_inequalities_iterative=False), dict(add_Shor_valid_inequalities_iterative=True, update_Shor_indices_n_minors=20)):
        runs = {}
        for warm in (False, True):
            sol, inst = bnb.branch_and_bound(eng, A, mask, gap=1e-3, time_limit=120.0, batch=4, use_max_steps=True, max_steps=12,
                                             add_Shor_valid_inequalities=True, Shor_valid_inequalities_noisy_rank1_num_entries_present=[4],
                                             shor_params=sp, shor_warm_start=warm, **kw)
            runs[warm] = (sol, inst)
            log = inst["run_log"]; c = inst["run_details"]
            lbs = [row[3] for row in log]
            assert all(b2 >= b1 - 1e-12 for b1, b2 in zip(lbs, lbs[1:]))
            assert sol["lower_bound"] <= sol["objective"] * (1 + 1e-6)
            assert c["nodes_dominated"] + c["nodes_relax_infeasible"] + c["nodes_relax_feasible"] == c["nodes_explored"]
            if warm:
                print("  driver", kw, {k_: c.get(k_) for k_ in ("nodes_explored", "warm_started", "shor_warm_refused", "shor_warm_outgrown", "shor_updates")})
                if c["nodes_relax_infeasible"] + c["nodes_relax_feasible"] > 1:      # a node below the root was relaxed
                    assert c.get("warm_started", 0) >= 1, c
            else:
                assert "warm_started" not in c
        lb0 = [runs[w][1]["run_log"][0][3] for w in (False, True)]
        assert abs(lb0[0] - lb0[1]) <= TOL * max(1.0, abs(lb0[0])), lb0
    eng.close()
