"""GPU tests of the objective cutoff (Engine.set_cutoff, status 4 = OBJECTIVE_LIMIT; run on the MI355X box: `pytest -m gpu`).

Instances, paths and the oracle's recorded objectives are those of tests/test_gpu_certificate.py (tests/golden/certificate_paths.json, read
only).  Tolerances are that file's: OBJ_REL = 2e-6 between a valid bound and the oracle's certified objective, REPRO = 1e-7 between the
sanitised numpy bound and the reported one.  early_stop_factor = 0 throughout, so that max_iters has no influence on a trajectory before
its cap: a node stopped by the cutoff at iteration t is then the same node as one capped at t (runs D) and one check earlier its bound
was not above the cutoff (runs E)."""
import math
import time

import numpy as np
import pytest

from test_gpu_certificate import Case, GAMMA, OBJ_REL, REPRO, SHAPES

pytestmark = pytest.mark.gpu
KEYS = ("objective", "dual_bound", "iters", "status_code")
OBJ0 = 2.913745664          # the oracle's objective at all three nodes of shape 0
CUTOFFS = {0: 0.99 * OBJ0, 1: 3.3, 2: 3.5}


@pytest.fixture(scope="module")
def have_gpu(omc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


@pytest.fixture(scope="module")
def cases(have_gpu, omc, orc):
    return [Case(omc, orc, s) for s in range(len(SHAPES))]


@pytest.fixture(scope="module")
def uncut(cases):
    """Every shape's nodes in one batch on a fresh engine that has never been given a cutoff: solved once, shared, not modified."""
    done = {}

    def get(s):
        if s not in done:
            done[s] = solve(cases[s], cases[s].nodes)
        return done[s]
    return get


def params(cs, **kw):
    return cs.params(early_stop_factor=0.0, **kw)


def solve(cs, nodes, cutoff=None, eng=None, **kw):
    own = eng is None
    if own:
        eng = cs.omc.Engine(cs.A, cs.mask, GAMMA, cs.k)
    if cutoff is not None:
        eng.set_cutoff(cutoff)
    out = eng.matrix_completion_SDP_relaxation(nodes, cs.cut_type, params=params(cs, **kw), want_X=False)
    stats = eng.cutoff_stats()
    if own:
        eng.close()
    for o in out:
        o["cutoff_stats"] = stats
    return out


def same(a, b, arrays=("Y", "U")):
    return all(a[q] == b[q] for q in KEYS) and all(np.array_equal(a[q], b[q]) for q in arrays)


# ---- 1. off is off ------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(cases, uncut):
    cs = cases[0]
    runs = [uncut(0), solve(cs, cs.nodes, cutoff=math.inf), solve(cs, cs.nodes, cutoff=1.01 * OBJ0)]
    for r in runs:
        assert [o["status_code"] for o in r].count(4) == 0 and r[0]["cutoff_stats"][0] == 0
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert same(a, b)


# ---- 2. it cuts, at the right check, without touching the trajectory -------------------------------------------------------------------------
@pytest.mark.parametrize("s", range(len(SHAPES)))
def test_cuts_at_the_right_check_on_the_same_trajectory(cases, uncut, s):
    cs = cases[s]; c = CUTOFFS[s]; U = uncut(s)
    every = params(cs).check_every
    C = solve(cs, cs.nodes, cutoff=c)
    eng = cs.omc.Engine(cs.A, cs.mask, GAMMA, cs.k)          # runs D and E: one engine without a cutoff, node after node
    for d, (u, o, node) in enumerate(zip(U, C, cs.nodes)):
        print(f"shape {s} node {d}: cutoff {c!r} | uncut status {u['status_code']} iters {u['iters']} dual_bound {u['dual_bound']!r} objective {u['objective']!r}"
              f" | cut status {o['status_code']} iters {o['iters']} dual_bound {o['dual_bound']!r}")
        if o["status_code"] == 4:
            assert o["dual_bound"] > c
            assert o["iters"] % every == 0
            D = solve(cs, [node], eng=eng, max_iters=o["iters"])[0]
            assert D["iters"] == o["iters"] and all(np.array_equal(D[q], o[q]) for q in ("dual_bound", "objective", "Y", "U"))
            if o["iters"] - every > 0:
                E = solve(cs, [node], eng=eng, max_iters=o["iters"] - every)[0]
                print(f"    one check earlier: iters {E['iters']} dual_bound {E['dual_bound']!r}")
                assert E["dual_bound"] <= c
        if cs.ref_status[d] == 0:
            ref = float(cs.ref_objective[d])
            assert o["dual_bound"] <= ref + OBJ_REL * max(1.0, abs(ref))
            if ref < c:
                assert o["status_code"] != 4 and same(u, o)
    eng.close()
    assert C[0]["cutoff_stats"][0] == [o["status_code"] for o in C].count(4)
    assert C[0]["cutoff_stats"][1] == sum(o["iters"] for o in C if o["status_code"] == 4)
    if s == 0:
        for u, o in zip(U, C):
            assert o["status_code"] == 4 and o["iters"] < u["iters"]
    if s == 1:
        assert C[0]["status_code"] != 4 and same(U[0], C[0])
        for u, o in zip(U[1:], C[1:]):
            if u["dual_bound"] > c:
                assert o["status_code"] == 4
    if s == 2:
        for o in C[2:]:
            assert o["status_code"] in (3, 4)


# ---- 3. the prune is re-verifiable -----------------------------------------------------------------------------------------------------------
def test_cut_off_nodes_export_the_certificate_of_the_prune(cases):
    cs = cases[0]; c = CUTOFFS[0]
    eng = cs.omc.Engine(cs.A, cs.mask, GAMMA, cs.k)
    eng.keep_certificates(True)
    out = solve(cs, cs.nodes, cutoff=c, eng=eng)
    certs = eng.fetch_certificate(range(len(cs.nodes)))
    eng.close()
    assert [o["status_code"] for o in out] == [4, 4, 4]
    for o, ce, node in zip(out, certs, cs.nodes):
        val, df = cs.numpy_bound(node, ce)
        print(f"dual_bound {o['dual_bound']!r} numpy {val!r} shortfall {o['dual_bound'] - val:.3e} defects {df}")
        assert ce.bound == o["dual_bound"]
        assert o["dual_bound"] - val <= REPRO * max(1.0, abs(o["dual_bound"]))
        assert val > c - REPRO * max(1.0, abs(c))


# ---- 4. live update --------------------------------------------------------------------------------------------------------------------------
def test_cutoff_set_while_the_solve_runs(cases):
    """Nodes that cannot end by themselves (eps_gap = 0, no stall rule, a million iterations) in a held solve; the cutoff arrives once a check
    has passed.  A build in which it has no effect lets the solve run into its own 20 s limit, and the test fails."""
    cs = cases[0]
    eng = cs.omc.Engine(cs.A, cs.mask, GAMMA, cs.k)
    eng.stage(cs.nodes, cs.cut_type, params(cs, eps_gap=0.0, stall_checks=10**6, max_iters=10**6, time_limit=20.0, slots=2))
    eng.hold(True)
    eng.submit()
    deadline = time.time() + 10.0
    checks = 0
    while time.time() < deadline:
        assert eng.poll()["running"]
        checks = eng.host_phases()["check_wait"]["count"]
        if checks >= 1:
            break
        time.sleep(0.001)
    assert checks >= 1
    t0 = time.time()
    eng.set_cutoff(-math.inf)
    eng.hold(False)
    eng.wait()
    dt = time.time() - t0
    out = eng.fetch(want_X=False)
    stats = eng.cutoff_stats()
    assert eng.get_cutoff() == -math.inf
    eng.close()
    print(f"checks before the call {checks}, {dt:.3f} s from set_cutoff to the end, iterations {[o['iters'] for o in out]}, stats {stats}")
    assert [o["status_code"] for o in out] == [4, 4, 4] and all(o["iters"] < 10**6 for o in out)
    assert stats[0] == 3 and stats[1] == sum(o["iters"] for o in out) and stats[2] >= 1 and stats[3] == 0
    assert dt < 10.0


# ---- 5. Shor mode ----------------------------------------------------------------------------------------------------------------------------
def test_shor_mode(have_gpu, omc, orc):
    """12 x 14 with its 152 class-4 minors (tests/test_gpu_shor.py), the root and its first child.  Shor mode checks at a node's own cap, so
    run D is exact there too."""
    import omc_oracle_shor as sh
    A, mask = orc.make_instance(12, 14, 1, n_indices=70, seed=2, noise=0.1, kind="lowrank")
    minors, _ = sh.driver_shor_lists(mask, (4,))
    assert len(minors) == 152
    eng = omc.Engine(A, mask, GAMMA, 1)
    root = eng.matrix_completion_SDP_relaxation([[]], "linear", params=omc.default_params(rho_scale=4.0))[0]
    nodes = [[], omc.pkg.bnb.make_children([], root, "linear", 1)[0]]

    def run(nd, max_iters=6000):
        P = omc.default_params(eps_gap=1e-6, max_iters=max_iters, early_stop_factor=0.0)
        return eng.matrix_completion_SDP_relaxation(nd, "linear", P, add_Shor_valid_inequalities=True, shor_info=[(minors, None)] * len(nd), want_Theta=True)

    U = run(nodes)
    c = 0.98 * U[0]["objective"]
    every = omc.default_params().check_every
    eng.set_cutoff(c)
    C = run(nodes)
    assert eng.cutoff_stats()[0] == 2
    eng.set_cutoff(math.inf)
    for d, (u, o, node) in enumerate(zip(U, C, nodes)):
        print(f"node {d}: cutoff {c!r} | uncut status {u['status_code']} iters {u['iters']} objective {u['objective']!r} | cut status {o['status_code']} iters {o['iters']} dual_bound {o['dual_bound']!r}")
        assert o["status_code"] == 4 and o["iters"] < u["iters"] and o["dual_bound"] > c
        D = run([node], max_iters=o["iters"])[0]
        assert D["iters"] == o["iters"] and all(np.array_equal(D[q], o[q]) for q in ("objective", "dual_bound", "X", "W", "Theta"))
        if o["iters"] - every > 0:
            E = run([node], max_iters=o["iters"] - every)[0]
            print(f"    one check earlier: iters {E['iters']} dual_bound {E['dual_bound']!r}")
            assert E["dual_bound"] <= c
    eng.close()


# ---- 6. drivers ------------------------------------------------------------------------------------------------------------------------------
DRIVER_GAP = 0.25


def test_drivers(have_gpu, omc, orc):
    """The 14 x 18 instance of test_streaming_branch_and_bound_against_the_round_based_driver.  Its tree does not close to 1e-4 in any time a
    test may take (measured on the MI355X: gap 0.199 after 60 s and 45 000 nodes, with and without the cutoff), so both drivers run to
    gap = 0.25, which the round-based driver reaches after about 800 nodes and 2 s, the queue-driven one after about 1100 nodes and
    1.4 s, each with pruned nodes on the way (the first within the first 30 relaxations).  Ending by the gap, never by the clock, is
    what makes the round-based runs comparable node for node: that driver is deterministic, and with the cutoff it must grow the same
    tree with no more iterations.  The queue-driven driver depends on timing (which nodes are in flight when, hence which split nodes feed
    the alternating minimisation): its two runs are not comparable bit for bit, with or without the cutoff.  It must reach the same
    incumbent to the tolerance that routine converges to and close the same gap."""
    A, mask = orc.make_instance(14, 18, 1, seed=5, kind="lowrank", n_indices=int(0.35 * 14 * 18), noise=0.15)
    runs = {}
    for on in (False, True):
        eng = omc.Engine(A, mask, GAMMA, 1)
        runs[on] = omc.pkg.bnb.branch_and_bound(eng, A, mask, gap=DRIVER_GAP, time_limit=120.0, batch=64, rho_scale=8.0, seed=0, use_certified_bound=True,
                                                objective_cutoff=on)
        assert eng.get_cutoff() == math.inf
        eng.close()
    (a, ia), (b, ib) = runs[False], runs[True]
    ca, cb = ia["run_details"], ib["run_details"]
    la, lb_ = ia["relax_log"], ib["relax_log"]
    ended = lambda log: {e[0] for e in log if e[3] in ("infeasible", "pruned", "cutoff")}      # noqa: E731
    ita, itb = sum(e[2] for e in la), sum(e[2] for e in lb_)
    print(f"round-based off: {len(la)} nodes, pruned {ca['nodes_relax_feasible_pruned']} infeasible {ca['nodes_relax_infeasible']}, iterations {ita}, lower {a['lower_bound']!r} upper {a['objective']!r}, {ca['time_taken']:.2f} s")
    print(f"round-based on : {len(lb_)} nodes, pruned {cb['nodes_relax_feasible_pruned']} (cutoff {cb['nodes_relax_cutoff']}) infeasible {cb['nodes_relax_infeasible']}, iterations {itb}, lower {b['lower_bound']!r} upper {b['objective']!r}, {cb['time_taken']:.2f} s")
    assert a["gap"] <= DRIVER_GAP and b["gap"] <= DRIVER_GAP          # both runs ended by the gap, not by the time limit
    assert "nodes_relax_cutoff" not in ca
    assert [e[0] for e in la] == [e[0] for e in lb_]
    assert a["lower_bound"] == b["lower_bound"] and a["objective"] == b["objective"] and np.array_equal(a["X"], b["X"])
    assert ended(la) == ended(lb_)
    assert cb["nodes_relax_cutoff"] <= cb["nodes_relax_feasible_pruned"]
    assert itb <= ita
    if ca["nodes_relax_feasible_pruned"] + ca["nodes_relax_infeasible"] > 0:
        assert cb["nodes_relax_cutoff"] > 0 and itb < ita
    st = {}
    for on in (False, True):
        eng = omc.Engine(A, mask, GAMMA, 1)
        st[on] = omc.pkg.bnb_stream.branch_and_bound_streaming(eng, A, mask, gap=DRIVER_GAP, time_limit=120.0, slots=64, rho_scale=8.0, objective_cutoff=on)
        assert eng.get_cutoff() == math.inf
        eng.close()
    (p, ip), (q, iq) = st[False], st[True]
    print(f"queue-driven off: {len(ip['relax_log'])} nodes, iterations {sum(e[2] for e in ip['relax_log'])}, lower {p['lower_bound']!r} upper {p['objective']!r}, {ip['run_details']['time_taken']:.2f} s")
    print(f"queue-driven on : {len(iq['relax_log'])} nodes (cutoff {iq['run_details']['nodes_relax_cutoff']}), iterations {sum(e[2] for e in iq['relax_log'])}, lower {q['lower_bound']!r} upper {q['objective']!r}, {iq['run_details']['time_taken']:.2f} s")
    # the same incumbent: both are alternating-minimisation points of one local optimum, each converged to that routine's eps = 1e-5, and which
    # split nodes feed it depends on the order in which nodes finish (measured: 1.5944157611 off, 1.5944161061 on, 1.5944151637 round-based)
    assert abs(q["objective"] - p["objective"]) <= 1e-5 * max(1.0, abs(p["objective"]))
    assert p["gap"] <= DRIVER_GAP and q["gap"] <= DRIVER_GAP and q["lower_bound"] <= q["objective"] * (1 + 1e-9)
    assert iq["run_details"]["nodes_relax_cutoff"] <= iq["run_details"]["nodes_relax_feasible_pruned"]
