"""GPU tests of appending Shor nodes to a staged / running Shor batch (omc_relax_reserve_shor, omc_relax_append_shor,
omc_relax_fetch_done_shor; DESIGN.md sections 3.4, 3.8b) and of the Shor mode of the queue-driven driver.  Run on the MI355X box:
`pytest -m gpu`.

Instance (that of test_gpu_shor_warm.py): 10 x 12 rank 1, 60 observed entries, seed 2, noise 0.1, gamma 80; the static class-4 list
(208 minors) and its first 104 minors, both with the complement SOC shorthand; eps_gap 1e-5, at most 6000 iterations, rho_scale 1.  The
cut is the oracle's root breakpoint vector, `left` or `right`.  The CPU oracle certifies all six (cut, list) pairs inside the cap (root /
left / right with 208 minors: 600 / 625 / 975 iterations, with 104: 3200 / 1800 / 3975), so every test may require status 0 of all six.

What is compared is bit identity (== / array_equal): a node's relaxation does not depend on its slot, on the moment it starts, on
whether it was staged or appended, or on the strides a reservation gave the batch.  The reference batch `ref` uses no reservation."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GAMMA = 80.0
NQ = 208
ORDER = ["root/208", "left/208", "right/208", "root/104", "left/104", "right/104"]


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


class Env:
    pass


def _key(o):
    return (o["objective"], o["dual_bound"], o["iters"], o["status_code"])


def _same(a, b, mats=("X", "W", "Theta")):
    return _key(a) == _key(b) and all(np.array_equal(a[q], b[q]) for q in mats)


def _collect(eng, lists, want_V):
    """Results of the batch the engine has just solved, as matrix_completion_SDP_relaxation returns them: fetch + W (+ V cut to the node's list)."""
    out = eng.fetch(want_Y=False, want_X=True, want_Theta=True)
    for r, W in zip(out, eng.fetch_shor()):
        r["W"] = W
    if want_V:
        for r, V, l in zip(out, eng.fetch_shor_V(), lists):
            r["V"] = V[:len(l)]
    return out


@pytest.fixture(scope="module")
def env(have_gpu, omc, orc):
    """The oracle's root (computed once) for the cut, the six nodes, one engine, `ref` = the six nodes in one stage_shor batch through two slots
    (no reservation), and the solo solves of the two roots.  Tests only read these."""
    import omc_oracle_shor as sh
    e = Env()
    e.omc = omc
    e.A, e.mask = orc.make_instance(10, 12, 1, n_indices=60, seed=2, noise=0.1)
    inst = orc.Instance(e.A, e.mask, GAMMA, 1)
    e.full, soc = sh.driver_shor_lists(e.mask, (4,))
    assert len(e.full) == NQ
    e.half = e.full[:104]
    o_root = sh.sdp_relaxation_shor(inst, e.full, soc, params=sh.ShorParams(eps_gap=1e-5, max_iters=6000))
    assert o_root["termination_status"] == 0
    x = orc.breakpoint_vector(o_root["Y"], o_root["U"])[0]
    e.left = [(x, o_root["U"], ["left"])]; e.right = [(x, o_root["U"], ["right"])]
    e.nodes = [[], e.left, e.right, [], e.left, e.right]
    e.lists = [e.full] * 3 + [e.half] * 3
    e.info = [(l, None) for l in e.lists]
    e.P1 = omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0, slots=1)
    e.P2 = omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0, slots=2)
    e.eng = omc.Engine(e.A, e.mask, GAMMA, 1)
    e.ref = e.eng.matrix_completion_SDP_relaxation(e.nodes, "linear", e.P2, add_Shor_valid_inequalities=True, shor_info=e.info,
                                                   want_Y=False, want_Theta=True, want_V=True)
    print("  ref iterations:", {nm: r["iters"] for nm, r in zip(ORDER, e.ref)})
    for nm, r in zip(ORDER, e.ref):
        assert r["status_code"] == 0, (nm, r["iters"], r["objective"], r["dual_bound"])
    e.solo = {}
    for i in (0, 3):
        e.solo[i] = e.eng.matrix_completion_SDP_relaxation([e.nodes[i]], "linear", e.P1, add_Shor_valid_inequalities=True, shor_info=[e.info[i]],
                                                           want_Y=False, want_Theta=True)[0]
    yield e
    e.eng.close()


def _stage_two_append_four(e, running):
    eng = e.eng
    eng.reserve(4, 1); eng.reserve_shor(NQ, 1)
    eng.stage_shor(e.nodes[:2], e.info[:2], "linear", e.P2, keep_V=True)
    if running:
        eng.submit()
    eng.append_shor(e.nodes[2:4], e.info[2:4], "linear")
    eng.append_shor(e.nodes[4:], e.info[4:], "linear")
    if running:
        assert eng.poll()["nodes_total"] == 6
        eng.wait()
    else:
        eng.solve()
    return _collect(eng, e.lists, want_V=True)


def test_appended_before_the_solve_equals_staged(env):
    """Nodes 0-1 staged behind reserve(4, 1) / reserve_shor(208, 1), the other four appended in two calls before solve(), default tuning:
    every scalar and X, W, Theta, V of every node equal `ref` bit for bit."""
    got = _stage_two_append_four(env, running=False)
    assert len(got) == 6
    for nm, g, r in zip(ORDER, got, env.ref):
        assert _same(g, r, ("X", "W", "Theta", "V")), (nm, _key(g), _key(r))


def test_appended_while_the_solve_runs_equals_staged(env):
    """The same with the four nodes appended after submit(), without graph replay (as the queue-driven driver runs)."""
    env.eng.tuning_set("OMC_NO_GRAPH", "1")
    try:
        got = _stage_two_append_four(env, running=True)
    finally:
        env.eng.tuning_set("OMC_NO_GRAPH", None)
    assert len(got) == 6
    for nm, g, r in zip(ORDER, got, env.ref):
        assert _same(g, r, ("X", "W", "Theta", "V")), (nm, _key(g), _key(r))
    with pytest.raises(env.omc.OmcError):
        env.eng.append_shor(env.nodes[:1], env.info[:1], "linear")          # the solve has ended


@pytest.mark.parametrize("order", [(0, 3), (3, 0)])
def test_slot_reuse_across_list_lengths(env, order):
    """One slot: root/208 staged and root/104 appended, then the reverse.  Each node equals its solo solve (and `ref`) bit for bit: nothing of
    the longer list's state survives in the slot, nothing of the shorter one's is missing."""
    e = env; eng = e.eng
    a, b = order
    eng.reserve(1, 0); eng.reserve_shor(NQ, 1)
    eng.stage_shor([e.nodes[a]], [e.info[a]], "linear", e.P1)
    eng.append_shor([e.nodes[b]], [e.info[b]], "linear")
    eng.solve()
    got = _collect(eng, [e.lists[a], e.lists[b]], want_V=False)
    for i, g in zip(order, got):
        assert _same(g, e.solo[i]), (ORDER[i], _key(g), _key(e.solo[i]))
        assert _same(g, e.ref[i]), (ORDER[i], _key(g), _key(e.ref[i]))


def _wait_for(eng, count, seconds=120.0):
    seen = []
    deadline = time.time() + seconds
    while len(seen) < count and time.time() < deadline:
        got = eng.fetch_done()
        seen += got
        if not got:
            time.sleep(0.002)
    assert len(seen) == count, [o["node"] for o in seen]
    return seen


def test_warm_start_of_an_appended_prefix_child(env, omc):
    """Pool of 4 with room for 208 minors.  Parent root/104 saves to entry 0; the child root/208 is appended with load_from=[0] once the
    parent has come back through fetch_done, while the solve is held open.  The child equals, bit for bit, the child staged by stage_shor
    with load_from=[0] in a batch of its own after the parent; it is certified and needs strictly fewer iterations than its cold solve;
    one prefix load and one save are counted.  An entry saved by a base-mode solve is refused and counted, and the node still certifies."""
    e = env
    eng = omc.Engine(e.A, e.mask, GAMMA, 1)
    try:
        eng.state_pool_create(4); eng.state_pool_reserve_shor(NQ)
        kw = dict(add_Shor_valid_inequalities=True, want_Y=False, want_Theta=True)
        # the reference: two batches
        par = eng.matrix_completion_SDP_relaxation([[]], "linear", e.P1, shor_info=[(e.half, None)], save_to=[0], **kw)[0]
        want = eng.matrix_completion_SDP_relaxation([[]], "linear", e.P1, shor_info=[(e.full, None)], load_from=[0], **kw)[0]
        assert eng.shor_warm_stats() == dict(loaded_identical=0, loaded_prefix=1, refused=0, saved=0)
        assert _same(par, e.solo[3])
        # the same through one running batch
        eng.tuning_set("OMC_NO_GRAPH", "1")
        eng.reserve(1, 0); eng.reserve_shor(NQ, 1)
        eng.stage_shor([[]], [(e.half, None)], "linear", e.P1, save_to=[0])
        eng.hold(True)
        eng.submit()
        first = _wait_for(eng, 1)
        assert first[0]["node"] == 0 and first[0]["iters"] == par["iters"]
        eng.append_shor([[]], [(e.full, None)], "linear", load_from=[0])
        eng.hold(False)
        eng.wait()
        got = _collect(eng, [e.half, e.full], want_V=False)
        stats = eng.shor_warm_stats()
        cold = e.solo[0]
        print("  prefix child appended: iterations cold", cold["iters"], "warm", got[1]["iters"], "(parent", got[0]["iters"], ")", stats)
        assert stats == dict(loaded_identical=0, loaded_prefix=1, refused=0, saved=1)
        assert _same(got[0], par)
        assert _same(got[1], want), (_key(got[1]), _key(want))
        assert got[1]["status_code"] == 0 and got[1]["dual_bound"] <= got[1]["objective"] * (1 + 1e-5)
        assert got[1]["iters"] < cold["iters"], (got[1]["iters"], cold["iters"])
        # an entry a base-mode solve saved: refused, counted, cold
        eng.tuning_set("OMC_NO_GRAPH", None)
        eng.matrix_completion_SDP_relaxation([[]], "linear", omc.default_params(rho_scale=4.0), save_to=[1], want_X=False, want_Y=False)
        eng.reserve(1, 0)
        eng.stage_shor([[]], [(e.full, None)], "linear", e.P1)
        eng.append_shor([[]], [(e.full, None)], "linear", load_from=[1])
        eng.solve()
        got = _collect(eng, [e.full, e.full], want_V=False)
        assert eng.shor_warm_stats() == dict(loaded_identical=0, loaded_prefix=0, refused=1, saved=0)
        assert got[1]["status_code"] == 0 and _same(got[1], cold) and _same(got[0], cold)
    finally:
        eng.close()


def test_queue_driven_loop_append_shor_and_fetch_done_shor(env):
    """The shape of test_queue_driven_loop_append_and_fetch_done with the six Shor nodes: two slots, two nodes staged, the solve held open,
    one append per finished node.  Every node comes back exactly once with the scalars of `ref`, and fetch_done_shor gives `ref`'s X, W and
    Theta while the solve is still open."""
    e = env; eng = e.eng
    eng.tuning_set("OMC_NO_GRAPH", "1")
    try:
        eng.reserve(4, 1); eng.reserve_shor(NQ, 1)
        eng.stage_shor(e.nodes[:2], e.info[:2], "linear", e.P2)
        eng.hold(True)
        eng.submit()
        sent, seen, mats, deadline = 2, {}, {}, time.time() + 120
        while len(seen) < 6 and time.time() < deadline:
            got = eng.fetch_done()
            for o in got:
                assert o["node"] not in seen
                seen[o["node"]] = o
            if got:
                for d in eng.fetch_done_shor([o["node"] for o in got], want_W=True, want_Theta=True):
                    mats[d["node"]] = d
                more = min(len(got), 6 - sent)
                if more:
                    eng.append_shor(e.nodes[sent:sent + more], e.info[sent:sent + more], "linear")
                    sent += more
            else:
                time.sleep(0.002)
        assert eng.poll()["running"]                                        # every node is back and the solve is still open
        with pytest.raises(e.omc.OmcError) as err:
            eng.fetch_done_shor([6])                                        # out of range
        assert err.value.code == -3
        eng.hold(False)
        eng.wait()
    finally:
        eng.tuning_set("OMC_NO_GRAPH", None)
    assert sorted(seen) == list(range(6))
    for i in range(6):
        assert _key(seen[i]) == _key(e.ref[i]), (ORDER[i], _key(seen[i]), _key(e.ref[i]))
        for q in ("X", "W", "Theta"):
            assert np.array_equal(mats[i][q], e.ref[i][q]), (ORDER[i], q)
    assert eng.fetch_done() == []
    after = _collect(eng, e.lists, want_V=False)
    for i in range(6):
        assert _same(after[i], e.ref[i]), ORDER[i]


def test_limits(env, omc):
    """Every refusal of omc_relax_append_shor raises OmcError (OMC_ERR_ARGUMENT) and leaves the batch as it was: the batch afterwards solves to
    `ref`.  omc_relax_append on a Shor batch and append_shor on a base batch raise too."""
    e = env; eng = e.eng

    def refused(*a, **k):
        with pytest.raises(omc.OmcError) as err:
            eng.append_shor(*a, **k)
        assert err.value.code == -3, err.value
        return str(err.value)

    fresh = omc.Engine(e.A, e.mask, GAMMA, 1)
    try:
        with pytest.raises(omc.OmcError) as err:
            fresh.append_shor([[]], [(e.full, None)], "linear")             # nothing staged
        assert err.value.code == -3
        with pytest.raises(omc.OmcError) as err:
            fresh.reserve_shor(-1, 0)
        assert err.value.code == -3
        with pytest.raises(omc.OmcError) as err:
            fresh.reserve_shor(1, -1)
        assert err.value.code == -3
        fresh.reserve(2, 1)
        fresh.stage([[]], "linear", omc.default_params(rho_scale=4.0))
        with pytest.raises(omc.OmcError) as err:
            fresh.append_shor([[]], [(e.full, None)], "linear")             # a base batch
        assert err.value.code == -3 and "Shor" in str(err.value)
    finally:
        fresh.close()
    eng.reserve(4, 1); eng.reserve_shor(NQ, 1)
    eng.stage_shor(e.nodes[:2], e.info[:2], "linear", e.P2)
    with pytest.raises(omc.OmcError):
        eng.append(e.nodes[2:3], "linear")                                  # omc_relax_append keeps refusing Shor batches
    used = set(tuple(t) for t in e.full)
    extra = next((i1, i2, j1, j2) for i1 in range(1, 11) for i2 in range(i1 + 1, 11) for j1 in range(1, 13) for j2 in range(j1 + 1, 13)
                 if (i1, i2, j1, j2) not in used)
    assert "minors" in refused([[]], [(list(e.full) + [extra], None)], "linear")                       # a list longer than nqmax
    assert "cuts" in refused([e.left + e.right], [(e.full, None)], "linear")                           # more cuts than reserved
    assert "capacity" in refused([[]] * 5, [(e.full, None)] * 5, "linear")                             # beyond node_cap
    assert "pool" in refused([[]], [(e.full, None)], "linear", load_from=[0])                          # warm indices without a pool
    refused([[]], [([(1, 1, 1, 2)], None)], "linear")                                                    # an argument error of omc_relax_stage_shor
    refused([[]], [([(1, 2, 1, 2), (1, 2, 1, 2)], None)], "linear")                                      # duplicate minor
    refused([[]], [(e.half, [(11, 1)])], "linear")                                                       # SOC coordinate out of range
    eng.append_shor(e.nodes[3:4], e.info[3:4], "linear")                                                 # the half list takes the one reserved list
    assert "list capacity" in refused([[]], [(e.full[50:150], None)], "linear")                        # a new list when the list capacity is used up
    eng.append_shor([e.nodes[2]] + e.nodes[4:], [e.info[2]] + e.info[4:], "linear")                      # known lists: no list capacity needed
    refused([[]], [(e.full, None)], "linear")                                                            # node capacity is used up now
    eng.solve()
    got = _collect(eng, [e.lists[i] for i in (0, 1, 3, 2, 4, 5)], want_V=False)
    for g, i in zip(got, (0, 1, 3, 2, 4, 5)):
        assert _same(g, e.ref[i]), (ORDER[i], _key(g), _key(e.ref[i]))
    assert "ended" in refused([[]], [(e.full, None)], "linear")                                        # the solve has ended
    with pytest.raises(omc.OmcError) as err:
        eng.fetch_done_shor([0])                                            # finished, but fetch_done has not returned it yet
    assert err.value.code == -3
    assert len(eng.fetch_done()) == 6
    assert np.array_equal(eng.fetch_done_shor([2])[0]["X"], e.ref[3]["X"])


def test_streaming_driver_with_shor_against_the_round_based_driver(have_gpu, omc, orc):
    """bnb_stream.branch_and_bound_streaming with the Shor inequalities, static and iterative, against bnb.branch_and_bound on the instance of
    test_streaming_branch_and_bound_against_the_round_based_driver (14 x 18, seed 5, noise 0.15), class-4 minors: the runs bracket one
    optimum, the streaming runs keep the invariants of SURVEY 8c, explore more than the root, and in iterative mode relax nodes that carry
    minors and start warm.  No node count or rate is asserted."""
    A, mask = orc.make_instance(14, 18, 1, seed=5, kind="lowrank", n_indices=int(0.35 * 14 * 18), noise=0.15)
    eng = omc.Engine(A, mask, GAMMA, 1)
    try:
        a, ia = omc.pkg.bnb.branch_and_bound(eng, A, mask, add_Shor_valid_inequalities=True, Shor_valid_inequalities_noisy_rank1_num_entries_present=(4,),
                                             use_max_steps=True, max_steps=6, batch=4)
        for kw in (dict(), dict(add_Shor_valid_inequalities_iterative=True, update_Shor_indices_n_minors=20)):
            b, ib = omc.pkg.bnb_stream.branch_and_bound_streaming(eng, A, mask, add_Shor_valid_inequalities=True,
                                                                  Shor_valid_inequalities_noisy_rank1_num_entries_present=(4,), time_limit=6.0, slots=8,
                                                                  shor_warm_start=True, **kw)
            c = ib["run_details"]; log = np.array(ib["run_log"])
            print("  round-based:", ia["run_details"]["nodes_explored"], "nodes, lb", a["lower_bound"], "ub", a["objective"], "; streaming", kw, ":",
                  {q: c.get(q) for q in ("nodes_explored", "epochs", "warm_started", "shor_updates", "shor_nodes_with_minors", "shor_warm_refused", "shor_warm_outgrown")},
                  "lb", b["lower_bound"], "ub", b["objective"])
            assert a["lower_bound"] <= b["objective"] * (1 + 1e-9) and b["lower_bound"] <= a["objective"] * (1 + 1e-9)
            assert (np.diff(log[:, 3]) >= -1e-9).all() and b["lower_bound"] <= b["objective"] * (1 + 1e-9)
            assert c["nodes_relax_infeasible"] + c["nodes_relax_feasible"] == c["nodes_explored"]
            assert np.linalg.matrix_rank(b["X"], tol=1e-8) <= 1
            assert b["objective"] == pytest.approx(orc.evaluate_objective(b["X"], A, mask, GAMMA), rel=1e-10)
            assert c["nodes_explored"] > 1
            if kw:
                assert c.get("shor_nodes_with_minors", 0) >= 1 and c["warm_started"] > 0, c
    finally:
        eng.close()
