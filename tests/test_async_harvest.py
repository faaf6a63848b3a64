"""The harvest off the iteration path, and the full eigen-kernel as one launch in quiet intervals: both are scheduling changes around
unchanged kernels, so every per-node output must be bit-identical to the path they replace (OMC_HARVEST_ASYNC=0, OMC_WS_QUIET=0).

Asynchronous harvest (omc_harvest_plan): with OMC_HARVEST_ASYNC_MIN_LIVE=1 a frontier through 4 slots takes the asynchronous path whenever
a slot finishes while another keeps running -- the harvest kernels run beside the next 25 iterations of the live slots, and the slot is
booked and refilled at the next check.  Shapes: 48 x 52 at rank 1 (np16 = 48: the tracked block is on, so k_sep_prepare / k_cone_sub<2>
are among the harvest kernels); a node costs milliseconds.

Quiet intervals: 70 x 72 at rank 1, the root and its two children warm-started from the root's state as in test_cone_sub_chain.py, with
hipGraph replay off (three nodes would otherwise replay a captured graph, which keeps the split it was captured with)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0
SCALARS = ("objective", "dual_bound", "status_code", "iters")
ARRAYS = ("U", "lambda_min", "breakpoint_vec", "Y")
ASYNC = {"OMC_HARVEST_ASYNC": "1", "OMC_HARVEST_ASYNC_MIN_LIVE": "1"}
SYNC = {"OMC_HARVEST_ASYNC": "0", "OMC_HARVEST_ASYNC_MIN_LIVE": "1"}
EAGER = {"OMC_GRAPH_MAX": "0"}


@pytest.fixture(scope="module")
def have_gpu(omc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


class _Knobs:
    def __init__(self, eng, env):
        self.eng, self.env = eng, env

    def __enter__(self):
        for k_, v in self.env.items():
            self.eng.tuning_set(k_, v)

    def __exit__(self, *exc):
        for k_ in self.env:
            self.eng.tuning_set(k_, None)


def _run(eng, nodes, P, env, **kw):
    with _Knobs(eng, env):
        return eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False, **kw)


def _same_node(x, y, arrays=ARRAYS):
    assert tuple(x[s] for s in SCALARS) == tuple(y[s] for s in SCALARS)
    for s in arrays:
        assert np.array_equal(x[s], y[s], equal_nan=True), s


def _same(a, b, arrays=ARRAYS):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        _same_node(x, y, arrays)


@pytest.fixture(scope="module")
def fam(have_gpu, omc):
    """48 x 52, rank 1: the depth-3 frontier (parents of the warm chain) and up to 24 nodes of the depth-5 frontier, expanded once."""
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, 48, 52, 874, seed=0)
    eng = omc.Engine(A, mask, GAMMA, 1)
    Pe = omc.default_params(rho_scale=4.0, max_iters=400)
    n5, _ = omc.pkg.bnb.expand_frontier(eng, 5, "linear", params=Pe)
    n3, _ = omc.pkg.bnb.expand_frontier(eng, 3, "linear", params=Pe)
    n5 = n5[:24]
    assert 16 <= len(n5) <= 32 and 4 <= len(n3) <= 8
    eng.state_pool_create(len(n3))
    yield dict(eng=eng, n5=n5, n3=n3, P4=omc.default_params(rho_scale=4.0, max_iters=400, slots=4))
    eng.close()


def test_frontier_through_four_slots(fam):
    """Several harvest and refill cycles: every output of every node equal to the synchronous path, and the counter says the asynchronous
    path was taken (and was not with the knob at 0)."""
    eng, nodes, P4 = fam["eng"], fam["n5"], fam["P4"]
    ref = _run(eng, nodes, P4, SYNC)
    assert eng.host_phases()["async_harvests"]["count"] == 0
    nharv = eng.kernel_stats()["harvest"]
    got = _run(eng, nodes, P4, ASYNC)
    hp = eng.host_phases()
    print("iters", [o["iters"] for o in ref], "async harvests", hp["async_harvests"]["count"], "harvests", eng.kernel_stats()["harvest"], "sync arm", nharv)
    assert len({o["iters"] for o in ref}) > 1          # the slots do not finish in lockstep: some harvest has live slots beside it
    assert hp["async_harvests"]["count"] >= 2
    assert eng.kernel_stats()["harvest"]["units"] == len(nodes)
    _same(ref, got)
    _same(ref, _run(eng, nodes, P4, {}))                # the default: below 256 live slots everything is synchronous
    assert eng.host_phases()["async_harvests"]["count"] == 0


@pytest.fixture(scope="module")
def chain(fam, omc):
    """The synchronous reference of the warm chain: the depth-3 nodes save their states, their children load them."""
    eng, parents, P4 = fam["eng"], fam["n3"], fam["P4"]
    save = list(range(len(parents)))
    par = _run(eng, parents, P4, SYNC, save_to=save)
    kids, lf, key = [], [], []
    for p, (cuts, o) in enumerate(zip(parents, par)):
        if not o["feasible"]:
            continue
        for c, kid in enumerate(omc.pkg.bnb.make_children(cuts, o, "linear", 1)):
            kids.append(kid); lf.append(p); key.append((p, c))
    assert len(kids) >= 4
    out = _run(eng, kids, P4, SYNC, load_from=lf)
    return dict(save=save, par=par, kids=kids, lf=lf, key=key, out=out)


def test_warm_chain_reads_states_an_asynchronous_harvest_saved(fam, chain):
    eng, parents, P4 = fam["eng"], fam["n3"], fam["P4"]
    par = _run(eng, parents, P4, ASYNC, save_to=chain["save"])
    na = eng.host_phases()["async_harvests"]["count"]
    _same(chain["par"], par)
    out = _run(eng, chain["kids"], P4, ASYNC, load_from=chain["lf"])
    print("async harvests: parents", na, "children", eng.host_phases()["async_harvests"]["count"], "iters", [o["iters"] for o in out])
    assert na + eng.host_phases()["async_harvests"]["count"] >= 1
    _same(chain["out"], out)
    assert any(o["iters"] < 400 for o in out)


def test_warm_chain_streamed_with_hold(fam, chain):
    """submit / append / wait with hold: the parents run through 4 slots and save their states; the children of a parent are appended,
    loading its entry, once fetch_done has delivered it -- with an asynchronous harvest that is at the check after the one that found it
    finished, when the state save has completed."""
    eng, parents, P4 = fam["eng"], fam["n3"], fam["P4"]
    kids_of = {}
    for kid, (p, c) in zip(chain["kids"], chain["key"]):
        kids_of.setdefault(p, []).append((c, kid))
    ref = {key: o for key, o in zip(chain["key"], chain["out"])}
    delivered = []
    with _Knobs(eng, ASYNC):
        eng.reserve(len(parents) - 2 + len(chain["kids"]), 4)
        eng.stage(parents[:2], "linear", P4, save_to=chain["save"][:2])
        eng.hold(True)
        eng.submit()
        try:
            eng.append(parents[2:], "linear", save_to=chain["save"][2:])
            order = [("p", p) for p in range(len(parents))]
            seen = 0
            deadline = time.monotonic() + 60.0
            while seen < len(parents) and time.monotonic() < deadline:
                for d in eng.fetch_done(max_nodes=64, want_Y=True):
                    kind, p = order[d["node"]]
                    if kind != "p":
                        continue
                    seen += 1
                    delivered.append((p, d))
                    fam_kids = kids_of.get(p, [])
                    if fam_kids:
                        eng.append([kid for _, kid in fam_kids], "linear", load_from=[p] * len(fam_kids))
                        order.extend(("k", (p, c)) for c, _ in fam_kids)
                time.sleep(0.001)
        finally:          # whatever happened above, the held solve is released and joined
            eng.hold(False)
            eng.wait()
        out = eng.fetch(want_X=False)
        hp = eng.host_phases()
    assert seen == len(parents)
    for p, d in delivered:
        _same_node(chain["par"][p], d)
    print("streamed: async harvests", hp["async_harvests"]["count"], "of", eng.kernel_stats()["harvest"]["launches"])
    assert len(out) == len(order) == len(parents) + len(chain["kids"])
    for (kind, key), o in zip(order, out):
        _same_node(chain["par"][key] if kind == "p" else ref[key], o)


def test_first_wins_leaves_no_harvest_dangling(fam, omc):
    eng, nodes = fam["eng"], fam["n5"]
    P = omc.default_params(rho_scale=4.0, max_iters=400, slots=4, first_wins=1)
    ref = _run(eng, nodes, P, SYNC)
    got = _run(eng, nodes, P, ASYNC)
    assert eng.host_phases()["async_harvests"]["count"] == 0          # first_wins keeps the synchronous path
    print("first_wins status", [o["status_code"] for o in got])
    assert len(got) == len(nodes) and all(o["status_code"] in (0, 1, 2, 3) for o in got)
    assert any(o["status_code"] == 0 for o in got)
    _same(ref, got)


def test_time_limit_mid_solve_leaves_no_harvest_dangling(fam, omc):
    """The limit strikes while slots are running, pending nodes wait and -- at most checks -- an asynchronous harvest is in flight: every
    node comes back with a status, those that never ran or were cut short with TIME_LIMIT."""
    eng, nodes = fam["eng"], fam["n5"]
    _run(eng, nodes, fam["P4"], ASYNC)
    full = eng.solver_info()["solve_seconds"]
    P = omc.default_params(rho_scale=4.0, max_iters=400, slots=4, time_limit=0.4 * full)
    got = _run(eng, nodes, P, ASYNC)
    st = [o["status_code"] for o in got]
    print("time_limit", 0.4 * full, "status", st, "async harvests", eng.host_phases()["async_harvests"]["count"])
    assert len(got) == len(nodes) and all(s in (0, 1, 2, 3) for s in st)
    assert st.count(2) >= 1
    assert eng.solver_info()["solve_seconds"] < full


def test_shor_batch_through_two_slots(have_gpu, omc, orc):
    """Shor mode (10 x 12, rank 1, the 208 class-4 minors of test_gpu_shor_append.py): the root and its two children, twice, through two
    slots.  Their harvests -- the base kernels and k_shor_state_save / k_shor_harvest -- run beside the other slot's iterations; scalars and
    X, W, Theta equal the synchronous path."""
    import omc_oracle_shor as sh
    A, mask = orc.make_instance(10, 12, 1, n_indices=60, seed=2, noise=0.1)
    full, _ = sh.driver_shor_lists(mask, (4,))
    eng = omc.Engine(A, mask, GAMMA, 1)
    kw = dict(add_Shor_valid_inequalities=True, want_Y=False, want_Theta=True)
    P1 = omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0, slots=1)
    P2 = omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0, slots=2)
    root = eng.matrix_completion_SDP_relaxation([[]], "linear", P1, shor_info=[(full, None)], **kw)[0]
    assert root["status_code"] == 0
    nodes = ([[]] + omc.pkg.bnb.make_children([], root, "linear", 1)) * 2
    info = [(full, None)] * len(nodes)
    res = {}
    for name, env in (("sync", SYNC), ("async", ASYNC)):
        with _Knobs(eng, env):
            res[name] = eng.matrix_completion_SDP_relaxation(nodes, "linear", P2, shor_info=info, **kw)
        res[name + "_n"] = eng.host_phases()["async_harvests"]["count"]
    print("shor iters", [o["iters"] for o in res["sync"]], "async harvests", res["async_n"])
    assert res["sync_n"] == 0 and res["async_n"] >= 1
    _same(res["sync"], res["async"], arrays=("U", "lambda_min", "breakpoint_vec", "X", "W", "Theta"))
    eng.close()


# ---- quiet intervals ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fam70(have_gpu, omc):
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, 70, 72, 1512, seed=0)
    eng = omc.Engine(A, mask, GAMMA, 1)
    eng.state_pool_create(1)
    root = _run(eng, [[]], omc.default_params(rho_scale=4.0, max_iters=1500), {}, save_to=[0])[0]
    nodes = [[]] + omc.pkg.bnb.make_children([], root, "linear", 1)
    yield dict(eng=eng, nodes=nodes, lf=[0] * len(nodes), P=omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14))
    eng.close()


def _quiet_pair(f, env, warm):
    eng, kw = f["eng"], (dict(load_from=f["lf"]) if warm else {})
    off = _run(eng, f["nodes"], f["P"], {**EAGER, **env, "OMC_WS_QUIET": "0"}, **kw)
    k0, h0, s0 = eng.kernel_stats(), eng.host_phases(), eng.subspace_stats()
    on = _run(eng, f["nodes"], f["P"], {**EAGER, **env, "OMC_WS_QUIET": "1"}, **kw)
    k1, h1, s1 = eng.kernel_stats(), eng.host_phases(), eng.subspace_stats()
    print("quiet intervals", h1["quiet_intervals"]["count"], "cone launches", k0["cone"]["launches"], "->", k1["cone"]["launches"],
          "global", k1["global"]["launches"], "subspace", s1)
    _same(off, on)
    assert s0 == s1
    assert h0["quiet_intervals"]["count"] == 0
    assert k0["cone"]["launches"] == 2 * k0["global"]["launches"] and k0["global"]["launches"] == k1["global"]["launches"]
    # an iteration of a quiet interval has one launch of the class instead of two; an interval is 25 iterations and a solve ends at a check
    assert k0["cone"]["launches"] - k1["cone"]["launches"] == 25 * h1["quiet_intervals"]["count"]
    return h1["quiet_intervals"]["count"], s1


def test_quiet_intervals_warm(fam70):
    q, _ = _quiet_pair(fam70, {}, True)
    assert q >= 1


def test_quiet_intervals_with_failures_inside(fam70):
    """A step cap of 2 makes calls fail on the cap (test_cone_sub_chain.py): a failure inside a quiet interval is served by the one
    launch behind k_cone_sub."""
    q, st = _quiet_pair(fam70, {"OMC_SUB_QMAX": "2"}, True)
    # warm slots follow their block from the first iteration, so after the first interval only a failed call sets w.ws_need: the first
    # failure of every burst falls into an interval that was launched quiet (and takes the next one out)
    assert st["fail_steps"] > 0 and q >= 1


def test_quiet_intervals_cold(fam70):
    """A cold start is never quiet at first: every slot is in the full kernel for its first iterations."""
    _quiet_pair(fam70, {}, False)
