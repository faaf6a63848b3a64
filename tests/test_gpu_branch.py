"""GPU tests of the children by reference (Engine.append_children / omc_relax_append_children; run on the MI355X box: `pytest -m gpu`).

A child's descriptor is built on the device from its parent's (omc_branch.hip).  The standard is the host path: the same node appended
from its whole cut list (Engine.append -> pack_nodes) on a second engine must have the same descriptor byte for byte, padding included,
and then the same relaxation bit for bit (the standard of test_gpu_parity.py::test_append_nodes_to_a_staged_and_to_a_running_batch).  No
field needed the fall-back bounds: every comparison here is equality.

Instances: shape 0 of tests/golden/certificate_paths.json (12 x 15, k = 1, linear: n below one wave), the golden 24 x 28 k = 1 linear2 and
16 x 20 k = 2 linear3 instances (16 children per parent, 5 rows per cut), and a seeded 70 x 72 k = 2 linear instance (n above one wave, no
multiple of 64).  early_stop_factor = 0 as in test_gpu_cutoff.py; the larger instances are capped at 400 iterations, which changes nothing
in what is compared (two engines, the same cap) and keeps every test to a few seconds.

A parent must have finished, and a batch whose solve has ended is closed to every append, so children by reference always enter a
submitted solve: one that is held and idle (the root's children) or one that is still relaxing the parent's siblings (the grandchildren).
Before omc_relax_submit no node can have finished: that call is one of the refusals below."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from test_gpu_certificate import GAMMA, REPRO, SHAPES

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("objective", "dual_bound", "iters", "status_code")
INT_FIELDS = ("rkind", "rcut", "rbi", "rbj")
NAMES = ("cert0_12x15_k1_linear", "lowrank_24x28_k1_linear2", "lowrank_16x20_k2_linear3", "seeded_70x72_k2_linear")
MAX_CUTS = 3


@pytest.fixture(scope="module")
def have_gpu(omc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


class Inst:
    def __init__(self, omc, orc, name):
        self.omc, self.name = omc, name
        self.max_iters = 400
        if name.startswith("cert0"):
            n, m, k, kind, cut_type, rho_scale, _ = SHAPES[0]
            self.A, self.mask = orc.make_instance(n, m, k, seed=21, kind=kind, n_indices=None)
            self.gamma, self.k, self.cut_type, self.rho_scale, self.max_iters = GAMMA, k, cut_type, rho_scale, 3000
        elif name.startswith("lowrank"):
            z = np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)
            self.A, self.mask, self.gamma, self.k = z["A"], z["mask"], float(z["gamma"]), int(z["k"])
            self.cut_type, self.rho_scale = str(z["cut_type"]), float(z["rho_scale"])
        else:
            self.A, self.mask = omc.pkg.data.generate_matrix_completion_data(2, 70, 72, int(0.35 * 70 * 72), seed=1)
            self.gamma, self.k, self.cut_type, self.rho_scale = GAMMA, 2, "linear", 4.0
        self.n = self.A.shape[0]

    def engine(self, keep=False):
        eng = self.omc.Engine(self.A, self.mask, self.gamma, self.k)
        if keep:
            eng.keep_certificates(True)
        return eng

    def params(self, **kw):
        return self.omc.default_params(rho_scale=self.rho_scale, early_stop_factor=0.0, max_iters=self.max_iters, **kw)


def wait_for(eng, res, ids, seconds=120.0):
    """Poll fetch_done (as the queue-driven driver does) until every id of `ids` has been returned; results by node id in `res`."""
    deadline = time.time() + seconds
    while any(i not in res for i in ids):
        got = eng.fetch_done()
        for o in got:
            res[o["node"]] = o
        if not got:
            assert time.time() < deadline, "the held solve did not return the nodes"
            time.sleep(0.001)


def grow(inst, device, pick=None, keep=False, capacity=64):
    """Root, its children, and the children of one child (`pick`: index among the root's children; None: the first that is not
    infeasible, once all of them have finished), through one held solve.  device: the children go in by reference, the grandchildren as
    soon as their parent has been returned, while its siblings may still be running; else from their host cut lists."""
    omc, k, ct = inst.omc, inst.k, inst.cut_type
    make_children = omc.pkg.bnb.make_children
    eng = inst.engine(keep)
    eng.reserve(capacity, MAX_CUTS)
    eng.stage([[]], ct, inst.params())
    eng.hold(True); eng.submit()
    res, cuts = {}, {0: []}
    wait_for(eng, res, [0])
    plan = eng.branch_plan(ct)
    before = eng.poll()["nodes_total"]
    kids = list(range(1, 1 + len(plan)))
    for i, c in zip(kids, make_children(cuts[0], res[0], ct, k)):
        cuts[i] = c
    if device:
        assert eng.append_children([0]) == kids
    else:
        eng.append([cuts[i] for i in kids], ct)
    assert eng.poll()["nodes_total"] == before + len(plan)
    if pick is None:
        wait_for(eng, res, kids)
        pick = next((q for q, i in enumerate(kids) if res[i]["status_code"] != 3), 0)
    parent = kids[pick]
    wait_for(eng, res, [parent])
    grand = list(range(kids[-1] + 1, kids[-1] + 1 + len(plan)))
    for i, c in zip(grand, make_children(cuts[parent], res[parent], ct, k)):
        cuts[i] = c
    if device:
        assert eng.append_children([parent], None) == grand
    else:
        eng.append([cuts[i] for i in grand], ct)
    wait_for(eng, res, kids + grand)
    desc = {i: eng.fetch_descriptor(i) for i in [0] + kids + grand}
    eng.hold(False); eng.wait()
    out = dict(res=res, cuts=cuts, desc=desc, kids=kids, grand=grand, pick=pick, parent=parent, fetch=eng.fetch(want_Y=False, want_X=False),
               info=eng.solver_info(), certs=None)
    if keep:
        out["certs"] = {i: c for i, c in zip(kids + grand, eng.fetch_certificate(kids + grand))}
    eng.close()
    return out


@pytest.fixture(scope="module")
def trees(have_gpu, omc, orc):
    """Per instance the host tree (the reference) and the device tree, grown once and shared, not modified."""
    done = {}

    def get(name):
        if name not in done:
            inst = Inst(omc, orc, name)
            keep = name.startswith("cert0")
            host = grow(inst, device=False, keep=keep)
            done[name] = (inst, host, grow(inst, device=True, pick=host["pick"], keep=keep))
        return done[name]
    return get


def assert_same_descriptor(a, b, where):
    for f in ("R", "L", "r"):
        assert a[f] == b[f], (where, f, a[f], b[f])
    for f in INT_FIELDS + ("rcoef", "rrhs", "cutx", "Q"):
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape, (where, f)
        assert a[f].tobytes() == b[f].tobytes(), (where, f, np.argwhere(a[f] != b[f])[:4].tolist())


def assert_padding_is_zero(d, where):
    R, L, r = d["R"], d["L"], d["r"]
    for f in INT_FIELDS + ("rcoef", "rrhs"):
        assert not d[f][R:].any(), (where, f)
    assert not d["cutx"][L:].any() and not d["Q"][:, r:].any(), where


# ---- 1. descriptor equality ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_descriptors_equal_the_host_path_byte_for_byte(trees, name):
    inst, host, dev = trees(name)
    k = inst.k
    assert dev["info"]["R_max"] == host["info"]["R_max"] and dev["info"]["r_max"] == host["info"]["r_max"]
    for i in [0] + dev["kids"] + dev["grand"]:
        assert_same_descriptor(dev["desc"][i], host["desc"][i], (name, i))
        assert_padding_is_zero(dev["desc"][i], (name, i))
    root, kid, gc = dev["desc"][0], dev["desc"][dev["parent"]], dev["desc"][dev["grand"][0]]
    assert (kid["L"], gc["L"]) == (1, 2) and (kid["R"], gc["R"]) == (root["R"] + 2 * k + 1, root["R"] + 2 * (2 * k + 1))
    if not np.array_equal(host["res"][0]["breakpoint_vec"], np.zeros(inst.n)):
        assert kid["r"] == root["r"] + 1      # x of the root is not in the span of the default box rows' unit vectors
    assert gc["r"] in (kid["r"], kid["r"] + 1)
    Q = gc["Q"][:, :gc["r"]]
    assert np.abs(Q.T @ Q - np.eye(gc["r"])).max() < 1e-12


# ---- 2. full row space -----------------------------------------------------------------------------------------------------------------------
def test_parent_with_full_row_space_gets_no_new_column(have_gpu, omc, orc):
    """The 12 x 15 root staged with U_lower = -0.999 on column 0: n box rows, r = n.  Its children keep r = n (pack_nodes' rule r < n).  The
    host twin cannot come from append (appended nodes have the default U bounds): it is staged, root and children with the same bounds,
    behind the same reservation, so the strides agree."""
    inst = Inst(omc, orc, NAMES[0])
    n, k, ct = inst.n, inst.k, inst.cut_type
    lo = np.full((n, k), -0.999)
    eng = inst.engine()
    eng.reserve(8, 6)
    eng.stage([[]], ct, inst.params(), U_lower=[lo])
    eng.hold(True); eng.submit()
    res = {}
    wait_for(eng, res, [0])
    kids = eng.append_children([0])
    assert kids == [1, 2]
    dev = {i: eng.fetch_descriptor(i) for i in [0] + kids}
    wait_for(eng, res, kids)
    eng.hold(False); eng.wait()
    eng.close()
    nodes = [[]] + omc.pkg.bnb.make_children([], res[0], ct, k)
    twin = inst.engine()
    twin.reserve(8, 6)
    twin.stage(nodes, ct, inst.params(), U_lower=[lo] * 3)
    host = {i: twin.fetch_descriptor(i) for i in range(3)}
    twin.solve()
    out = twin.fetch(want_Y=False, want_X=False)
    twin.close()
    assert dev[0]["r"] == n and dev[0]["R"] == 1 + n
    for i in range(3):
        assert_same_descriptor(dev[i], host[i], i)
        assert_padding_is_zero(dev[i], i)
        assert dev[i]["r"] == n
        assert all(res[i][q] == out[i][q] for q in KEYS), (i, [res[i][q] for q in KEYS], [out[i][q] for q in KEYS])


# ---- 3. solve equality -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_children_by_reference_relax_bit_for_bit_like_appended_ones(trees, name):
    """Both ways a child by reference can enter: into a held solve that has run dry (the root's children) and into a solve that may
    still be relaxing the parent's siblings (the grandchildren)."""
    inst, host, dev = trees(name)
    ids = [0] + dev["kids"] + dev["grand"]
    assert sorted(dev["res"]) == sorted(host["res"]) == ids
    for i in ids:
        a, b = dev["res"][i], host["res"][i]
        print(name, i, [a[q] for q in KEYS])
        assert all(a[q] == b[q] for q in KEYS), (name, i, [a[q] for q in KEYS], [b[q] for q in KEYS])
        assert a["U"].tobytes() == b["U"].tobytes() and a["breakpoint_vec"].tobytes() == b["breakpoint_vec"].tobytes(), (name, i)
    assert len(dev["fetch"]) == len(ids)
    for i in ids:                      # omc_relax_fetch after the solve: every node, the children behind the staged root in id order
        assert all(dev["fetch"][i][q] == dev["res"][i][q] for q in KEYS) and np.array_equal(dev["fetch"][i]["U"], dev["res"][i]["U"])


# ---- 4. order, ids, children as parents, certificates ----------------------------------------------------------------------------------------
def test_plan_order_ids_and_certificates(trees, omc):
    inst, host, dev = trees(NAMES[2])                                   # 16 children per parent
    plan = omc.pkg.bnb.child_directions(inst.cut_type, inst.k)
    assert dev["kids"] == list(range(1, 17)) and dev["grand"] == list(range(17, 33))
    codes = omc.pkg.api.DIR_CODES
    for c, i in enumerate(dev["kids"]):                                 # child c carries plan[c]: its host cut list does, and the rows agree (test 1)
        assert list(dev["cuts"][i][-1][2]) == plan[c]
        d = dev["desc"][i]
        assert d["rcut"][d["R"] - 1] == 0 and d["rkind"][d["R"] - 1] == 3      # the last row is the cut row of cut 0
    assert codes[plan[1][0]] != codes[plan[0][0]] and plan[1][1] == plan[0][1]
    # children were parents (the grandchildren), and every child's exported certificate re-checks against its host cut list
    inst, host, dev = trees(NAMES[0])
    cert = omc.pkg.certificate
    checked = 0
    for i in dev["kids"] + dev["grand"]:
        o, c = dev["res"][i], dev["certs"][i]
        val = cert.dual_bound(inst.A, inst.mask, GAMMA, inst.k, dev["cuts"][i], inst.cut_type, c, want_defects=True)[0]
        scale = max(1.0, abs(o["objective"] if abs(o["objective"]) < 1e299 else o["dual_bound"]))
        print("node", i, "status", o["status_code"], "dual_bound", o["dual_bound"], "numpy", val)
        assert c.bound == o["dual_bound"] and o["dual_bound"] - val <= REPRO * scale
        assert np.array_equal(c.Q, dev["desc"][i]["Q"][:, :dev["desc"][i]["r"]])
        checked += 1
    assert checked == 4


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(omc, eng, code, word, *args, **kw):
    before = eng.poll()["nodes_total"]
    with pytest.raises(omc.OmcError) as e:
        eng.append_children(*args, **kw)
    assert e.value.code == code and word in str(e.value), str(e.value)
    assert eng.poll()["nodes_total"] == before


def held_root(inst, nodes=1, reserve=(8, MAX_CUTS), **stage_kw):
    eng = inst.engine()
    eng.reserve(*reserve)
    eng.stage([[]] * nodes, inst.cut_type, inst.params(), **stage_kw)
    eng.hold(True); eng.submit()
    res = {}
    wait_for(eng, res, list(range(nodes)))
    return eng, res


def test_refusals_leave_the_batch_as_it_was(have_gpu, omc, orc):
    inst = Inst(omc, orc, NAMES[0])
    inst.max_iters = 200                                                # a refusal does not depend on how far the parent got
    n, lib = inst.n, omc.load()
    # nothing staged; C <= 0; a NULL argument
    eng = inst.engine()
    with pytest.raises(omc.OmcError) as e:
        eng.append_children([0], [("left",)])
    assert e.value.code == -3 and "nothing staged" in str(e.value)
    eng.reserve(8, MAX_CUTS)
    eng.stage([[]], inst.cut_type, inst.params())
    first = C.c_int(-1); p = (C.c_int * 1)(0); d = (C.c_int8 * 1)(0)
    assert lib.omc_relax_append_children(eng._h, 0, p, d, None, None, C.byref(first)) == -3
    assert lib.omc_relax_append_children(eng._h, 1, None, d, None, None, C.byref(first)) == -3
    assert lib.omc_relax_append_children(eng._h, 1, p, None, None, None, C.byref(first)) == -3
    assert lib.omc_relax_append_children(eng._h, 1, p, d, None, None, None) == -3
    # before omc_relax_submit no node has finished
    refused(omc, eng, -3, "has not finished", [0])
    eng.hold(True); eng.submit()
    res = {}
    wait_for(eng, res, [0])
    refused(omc, eng, -3, "has not finished", [1])                      # not a node at all
    refused(omc, eng, -3, "has not finished", [-1])
    refused(omc, eng, -1, "direction code", [0], [("middle",)])         # linear has no middle piece
    refused(omc, eng, -1, "direction code", [0, 0], [("left",), (7,)])  # nothing of the call is written, its valid first child neither
    refused(omc, eng, -3, "capacity", [0] * 9, [("left",)] * 9)
    kids = eng.append_children([0])                                      # and a valid call still succeeds
    assert kids == [1, 2]
    refused(omc, eng, -3, "has not finished", [kids[0]])                 # appended; fetch_done has not returned it, finished or not
    eng.hold(False); eng.wait()
    refused(omc, eng, -3, "ended", [0])
    eng.close()
    # more cuts than reserved
    eng, res = held_root(inst, reserve=(8, 1))
    kids = eng.append_children([0])
    wait_for(eng, res, kids)
    refused(omc, eng, -3, "more cuts", [kids[0]])
    eng.hold(False); eng.wait(); eng.close()
    # more rows than the stride: a root with four extra box rows fills Rmax, its child needs 2k + 1 more
    lo = np.full((n, 1), -1.0); lo[n - 1] = 0.0
    hi4 = np.ones((n, 1)); hi4[:4] = 0.5
    eng, res = held_root(inst, reserve=(8, 1), U_lower=[lo], U_upper=[hi4])
    refused(omc, eng, -3, "more rows", [0])
    eng.hold(False); eng.wait(); eng.close()
    # more row-subspace columns than the stride: node 0 (two rows on each of four entries) sets Rmax = 10, node 1 (one row on each of five)
    # sets rmax = 6 = its own r, and has room for the rows of a child but not for its column
    lo4 = lo.copy(); lo4[:4] = -0.5
    lo5 = lo.copy(); lo5[:5] = -0.5
    eng, res = held_root(inst, nodes=2, reserve=(8, 1), U_lower=[lo4, lo5], U_upper=[hi4, np.ones((n, 1))])
    refused(omc, eng, -3, "row-subspace", [1])
    refused(omc, eng, -3, "more rows", [0])
    eng.hold(False); eng.wait(); eng.close()
    # a Shor-mode batch
    idx = orc.shor_constraints_indexes(inst.mask, [4])[:8]
    eng = inst.engine()
    eng.reserve(4, 1); eng.reserve_shor(len(idx), 1)
    eng.stage_shor([[]], [(idx, None)], inst.cut_type, omc.default_params(rho_scale=1.0, max_iters=50))
    refused(omc, eng, -4, "Shor mode", [0])
    eng.close()


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------------------------
def test_streaming_driver_with_device_branching_walks_the_same_tree(have_gpu, omc, orc):
    """The 14 x 18 instance of test_streaming_branch_and_bound_against_the_round_based_driver.  One node in flight at a time (slots = 1,
    in_flight_target = 1), so that the order in which nodes finish -- and with it the tree -- does not depend on timing, and the
    reference's node cap (max_steps = 120 nodes created) instead of the time limit, so that both runs stop at the same node after a few
    seconds; device_branching on and off must then log the same nodes with the same statuses and iteration counts, count the same and
    end at the same bounds.  (Measured without the cap: the two runs logged the same 2063 nodes until the 60 s limit struck.)"""
    A, mask = orc.make_instance(14, 18, 1, seed=5, kind="lowrank", n_indices=int(0.35 * 14 * 18), noise=0.15)
    runs = []
    for on in (False, True):
        eng = omc.Engine(A, mask, GAMMA, 1)
        sol, inst = omc.pkg.bnb_stream.branch_and_bound_streaming(eng, A, mask, gap=1e-4, time_limit=300.0, slots=1, in_flight_target=1, rho_scale=8.0,
                                                                  capacity=256, device_branching=on, use_max_steps=True, max_steps=120)
        eng.close()
        runs.append((sol, inst))
    (sa, ia), (sb, ib) = runs
    ca, cb = dict(ia["run_details"]), dict(ib["run_details"])
    by_ref = cb.pop("nodes_appended_by_reference")
    print("nodes", ca["nodes_explored"], "by reference", by_ref, "epochs", cb["epochs"], "lb", sb["lower_bound"], "ub", sb["objective"])
    assert by_ref > 0 and "nodes_appended_by_reference" not in ca
    for key in ("time_taken", "solve_time_relaxation", "solve_time_altmin", "append_seconds"):
        ca.pop(key); cb.pop(key)
    assert ia["relax_log"] == ib["relax_log"] and len(ia["relax_log"]) > 3
    assert ca == cb
    assert (sa["lower_bound"], sa["objective"]) == (sb["lower_bound"], sb["objective"])
