"""The solve loop (csrc/omc_relax_solve.cpp over the slot bookkeeping of csrc/omc_slots.h) through every path it has: graph replay and
eager enqueue, synchronous and asynchronous harvests, one stream, nodes appended to a solve that has run dry, the time limit, a
first_wins race, Shor mode.  Within the build a node's relaxation does not depend on the path: scenarios A to D and the same nodes with
one slot each agree bit for bit.  With OMC_PARENT_LIB naming another build of the library (the parent commit's), every scenario also runs
there in a child process, and every scalar and array, the launches and units of every kernel class and the counts of every host phase
must be equal.

Shapes: the 24 x 30 rank-1 instance of smoke(), nodes from its depth-6 frontier and their prefixes (tests/test_between_iterations.py); the 10 x 12 Shor
instance of tests/test_gpu_shor_append.py.  A node costs milliseconds."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0
HERE = os.path.dirname(os.path.abspath(__file__))
NO_GRAPH = {"OMC_GRAPH_MAX": "0"}
# cuts kept of the twelve depth-6 nodes: the shallow ones certify after a few hundred iterations, the deep ones run to the cap of 400, so
# the four slots finish at different checks and a harvest finds live slots beside the finished ones
CUTS = [0, 6, 2, 6, 6, 1, 6, 3, 2, 6, 0, 6]


def _run(eng, nodes, P, env, **kw):
    for k_, v in env.items():
        eng.tuning_set(k_, v)
    try:
        return eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False, **kw)
    finally:
        for k_ in env:
            eng.tuning_set(k_, None)


def _compared(key, v):
    """Every number and array of a result but the wall-clock time of its solve."""
    return key != "solve_time" and isinstance(v, (bool, int, float, np.ndarray, np.generic))


def _counts(eng):
    """Launches and units of every kernel class, counts of every host phase, of the engine's last solve."""
    c = {"kernel/%s/%s" % (cls, f): v[f] for cls, v in eng.kernel_stats().items() for f in ("launches", "units")}
    c.update({"host/%s" % name: v["count"] for name, v in eng.host_phases().items()})
    return c


def _appended_to_a_dry_solve(eng, nodes, P):
    """Two nodes staged into four slots and held; once both are harvested the loop has run dry and waits; eight more arrive in one call and
    take the idle slots, then harvested ones.  (The loop re-reads the number of staged nodes at a check and when it is dry, and it counts
    a node as done after that check's read: nodes appended when both are done are always found by the dry loop, so the enqueue order and
    the counts do not depend on when the call lands.)"""
    eng.reserve(len(nodes) - 2, 6)
    eng.stage(nodes[:2], "linear", P)
    eng.hold(True)
    eng.submit()
    t0 = time.monotonic()
    while eng.poll()["nodes_done"] < 2:
        assert time.monotonic() - t0 < 60.0
        time.sleep(0.0005)
    eng.append(nodes[2:], "linear")
    eng.hold(False)
    eng.wait()
    return eng.fetch(want_X=False)


def _scenarios(omc, orc):
    """name -> (results, counts) of every scenario, on the library the process has loaded."""
    out = {}
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, 24, 30, int(0.35 * 24 * 30), seed=3)
    eng = omc.Engine(A, mask, GAMMA, 1)
    n6, _ = omc.pkg.bnb.expand_frontier(eng, 6, "linear", params=omc.default_params(rho_scale=4.0, max_iters=400))
    assert len(n6) >= 12 and all(len(c) == 6 for c in n6)
    nodes = [n6[i][:c] for i, c in enumerate(CUTS)]
    P4 = omc.default_params(rho_scale=4.0, max_iters=400, slots=4)
    for name, env in (("A", {}), ("B", NO_GRAPH), ("C", dict(NO_GRAPH, OMC_HARVEST_ASYNC_MIN_LIVE="1")), ("D", {"OMC_STREAMS": "1"})):
        out[name] = (_run(eng, nodes, P4, env), _counts(eng))
    out["solo"] = (_run(eng, nodes, omc.default_params(rho_scale=4.0, max_iters=400), {}), _counts(eng))
    out["E"] = (_appended_to_a_dry_solve(eng, nodes[:10], P4), _counts(eng))
    out["F"] = (_run(eng, n6[:6], omc.default_params(rho_scale=4.0, max_iters=300, slots=2, time_limit=1e-9), {}), _counts(eng))
    out["G"] = (_run(eng, [[], [], []], omc.default_params(rho_scale=1.0, first_wins=1), {}, rho_scales=[0.05, 4.0, 300.0]), _counts(eng))
    eng.close()
    # Shor mode: root and two children under the static class-4 list (208 minors) and under its first half, six nodes through two slots
    import omc_oracle_shor as sh
    A, mask = orc.make_instance(10, 12, 1, n_indices=60, seed=2, noise=0.1)
    eng = omc.Engine(A, mask, GAMMA, 1)
    full, _ = sh.driver_shor_lists(mask, (4,))
    Ps = omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0, slots=2)
    root = eng.matrix_completion_SDP_relaxation([[]], "linear", params=omc.default_params(rho_scale=4.0), want_X=False)[0]
    kids = omc.pkg.bnb.make_children([], root, "linear", 1)[:2]
    shor_nodes = [[], kids[0], kids[1]] * 2
    info = [(full, None)] * 3 + [(full[:104], None)] * 3
    out["H"] = (eng.matrix_completion_SDP_relaxation(shor_nodes, "linear", Ps, add_Shor_valid_inequalities=True, shor_info=info, want_Y=False, want_Theta=True),
                _counts(eng))
    eng.close()
    return out


def _flat(scen):
    """Every number and array of every result, and every count, by name."""
    flat = {}
    for name, (res, counts) in scen.items():
        flat[name + "/n"] = np.asarray(len(res))
        for i, o in enumerate(res):
            for key, v in o.items():
                if _compared(key, v):
                    flat["%s/%d/%s" % (name, i, key)] = np.asarray(v)
        for key, v in counts.items():
            flat["%s/count/%s" % (name, key)] = np.asarray(v)
    return flat


@pytest.fixture(scope="module")
def scen(omc, orc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return _scenarios(omc, orc)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for key, v in x.items():
            if _compared(key, v):
                assert np.array_equal(np.asarray(v), np.asarray(y[key]), equal_nan=True), key


@pytest.mark.parametrize("name", ["B", "C", "D", "solo"])
def test_paths_agree_bit_for_bit(scen, name):
    """12 nodes through 4 slots with graph replay (A) against the eager path (B), the eager path with asynchronous harvests from one live
    slot on (C), one stream (D), and one slot per node."""
    _same(scen["A"][0], scen[name][0])


def test_the_scenarios_take_their_paths(scen):
    """What each scenario is there for did happen: replay and eager launches, asynchronous harvests, refills, the statuses."""
    cnt = {k: v[1] for k, v in scen.items()}
    for k in scen:
        print(k, [(o["iters"], o["status_code"]) for o in scen[k][0]], {c: v for c, v in cnt[k].items() if v})
    assert cnt["A"]["kernel/colprox/launches"] == 0 and cnt["B"]["kernel/colprox/launches"] > 0      # replayed iterations launch no timed kernel
    assert cnt["A"]["host/async_harvests"] == 0 and cnt["B"]["host/async_harvests"] == 0 and cnt["C"]["host/async_harvests"] > 0
    assert cnt["A"]["kernel/harvest/units"] == 12 and cnt["C"]["kernel/harvest/units"] == 12 and cnt["solo"]["kernel/harvest/launches"] >= 1
    assert cnt["A"]["kernel/setup/units"] == 4 + 8 and cnt["solo"]["kernel/setup/units"] == 12
    assert cnt["E"]["kernel/harvest/units"] == 10 and cnt["E"]["kernel/setup/units"] == 4 + 8      # four slots set up at the start, two of them idle
    _same(scen["E"][0], scen["A"][0][:10])
    assert [o["termination_status"] for o in scen["F"][0]] == ["TIME_LIMIT"] * 6
    assert [o["iters"] for o in scen["F"][0]] == [25, 25, 0, 0, 0, 0] and cnt["F"]["kernel/harvest/units"] == 2
    race = scen["G"][0]
    assert race[1]["status_code"] == 0 and all(o["iters"] <= race[1]["iters"] for o in race) and 1 in (race[0]["status_code"], race[2]["status_code"])
    assert cnt["H"]["kernel/harvest/units"] == 6 and cnt["H"]["kernel/harvest/launches"] >= 2 and all("W" in o and "Theta" in o for o in scen["H"][0])


def test_against_another_build(scen, tmp_path):
    """Every scenario on the library OMC_PARENT_LIB names, in a child process: results, launches, units and host phase counts are equal."""
    parent = os.environ.get("OMC_PARENT_LIB")
    if not parent:
        pytest.skip("OMC_PARENT_LIB is not set: no other build to compare with")
    out = str(tmp_path / "parent.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, OMC_AMD_LIB=parent), timeout=300)
    z = np.load(out)
    mine = _flat(scen)
    assert sorted(mine) == sorted(z.files)
    for key, v in mine.items():
        assert np.array_equal(v, z[key], equal_nan=True), (key, v, z[key])


if __name__ == "__main__":      # child process of test_against_another_build: the scenarios on the library OMC_AMD_LIB names
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import omc_amd
    import omc_oracle
    np.savez(sys.argv[1], **_flat(_scenarios(omc_amd, omc_oracle)))
