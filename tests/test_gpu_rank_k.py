"""The SDP relaxation at ranks 3, 4, 5 and 8 on the GPU (run on the MI355X box: `pytest -m gpu`).

Every input is a rank-k fixture of tools/make_golden.py (RANK_K_CASES; tests/test_rank_k_cpu.py holds the conditions they meet): cut paths on
which cut rows carry multipliers and move the objective, up to R = 190 rows and r = 17 at rank 8, on both sides of k_small's r <= 16 boundary.
No oracle solve runs here; the oracle's objective of every node is in the fixture (test_golden.py::test_hip_reproduces_golden compares it),
and the oracle's helpers that need no solve rebuild the rows and re-evaluate the returned point.

The kernels are generic in k, and every other GPU comparison of a relaxation with the oracle is at k <= 2, where the k(k+1)/2 triangle rows,
the k x k blocks D3T / W3T / Q3T, the rmax x k blocks D3V / Vt, Psi3 of order r + k and the 2k + 1 rows per cut of the device branching sit at
their smallest sizes.  A mistake there is shared by both arms of an A/B test; sections a-c hold it to references, d-f to the engine's own
other paths.  Tolerances are those of the tests named in each section."""
import os

import numpy as np
import pytest

from test_golden import REL, load
from test_gpu_branch import KEYS, assert_padding_is_zero, assert_same_descriptor, wait_for
from test_gpu_certificate import OBJ_REL, REPRO, random_multipliers, scale_of
from test_gpu_parity import assert_finite

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K3, K4, K5, K8 = "lowrank_16x20_k3_linear", "lowrank_16x20_k4_linear3", "lowrank_16x20_k5_linear2", "lowrank_20x26_k8_linear2"
NAMES = (K3, K4, K5, K8)
ARM_KEYS = ("objective", "dual_bound", "iters", "status_code")


@pytest.fixture(scope="module")
def have_gpu(omc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


class Fixture:
    """One fixture: the instance, its listed nodes, the options it was made with, and (lazily, once) the engine's solve of all nodes in one
    batch with certificates kept (keeping them changes no result: test_gpu_certificate.py, section 3)."""

    def __init__(self, omc, name):
        self.omc, self.name = omc, name
        self.z, self.nodes = load(os.path.join(HERE, "golden", name + ".npz"))
        z = self.z
        self.A, self.mask, self.gamma, self.k = z["A"], z["mask"], float(z["gamma"]), int(z["k"])
        self.n = self.A.shape[0]
        self.cut_type, self.rho_scale = str(z["cut_type"]), float(z["rho_scale"])
        self.q1, self.breakpoints = bool(z["reference_quirk_q1"]), str(z["breakpoints"])
        self.L = [int(L) for L in z["node_L"]]
        self._kept = None

    def params(self, **kw):
        return self.omc.default_params(rho_scale=self.rho_scale, reference_quirk_q1=int(self.q1),
                                       breakpoints=self.omc.pkg.api.BREAKPOINTS[self.breakpoints], **kw)

    def engine(self):
        return self.omc.Engine(self.A, self.mask, self.gamma, self.k)

    def at(self, L):
        """Index of the listed node with L cuts."""
        return self.L.index(L)

    def kept(self):
        if self._kept is None:
            eng = self.engine()
            eng.keep_certificates(True)
            out = eng.matrix_completion_SDP_relaxation(self.nodes, self.cut_type, params=self.params(), want_Theta=True)
            certs = eng.fetch_certificate(range(len(self.nodes)))
            info = eng.solver_info()
            eng.close()
            self._kept = (out, certs, info)
        return self._kept


@pytest.fixture(scope="module")
def fixtures(have_gpu, omc):
    done = {}

    def get(name):
        if name not in done:
            done[name] = Fixture(omc, name)
        return done[name]
    return get


# ---- a. the returned point, per listed node (test_gpu_parity.py::test_relaxation_matches_oracle, lines 73-86) ---------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_returned_point_is_feasible_and_reproduces_its_objective(fixtures, orc, name):
    """The only place where SMALL_RECOVER's U = Y Q (Q'YQ)^+ Vt, the triangle rows and the cut rows are checked at these ranks.  A row
    projection that overflowed its 64-row passive set cannot end OPTIMAL (k_check_final reads the flag): every node must certify, as it
    did for the oracle.  smallest_2_eigvec: the mix of the two eigenvectors is compared with orc.breakpoint_vector on the GPU's own (Y, U) as
    test_rank2_linear3_smallest2_matches_oracle does, where both eigenvectors are determined (both gaps above 1e-6, the second eigenvalue
    away from the rule's switch at -1e-10)."""
    fx = fixtures(name)
    out, _, info = fx.kept()
    z = fx.z
    inst = orc.Instance(fx.A, fx.mask, fx.gamma, fx.k)
    assert info["R_max"] == int(z["R"].max()) and info["r_max"] == int(z["r"].max())
    compared = 0
    for b, (g, cuts) in enumerate(zip(out, fx.nodes)):
        assert_finite(g)
        assert g["status_code"] == 0, (name, fx.L[b], g["termination_status"])
        assert g["objective"] == pytest.approx(float(z["objective"][b]), rel=REL)
        assert abs(g["objective"] - g["dual_bound"]) <= 1.01e-6 * max(1.0, abs(g["objective"]))
        S = g["U"] @ g["U"].T - g["Y"]
        w, V = np.linalg.eigh(0.5 * (S + S.T))
        assert g["lambda_min"][0] == pytest.approx(w[0], abs=1e-9)
        if fx.breakpoints == "smallest_1_eigvec":
            if w[1] - w[0] > 1e-6:
                v = V[:, 0] * np.sign(V[np.argmax(np.abs(V[:, 0])), 0])
                assert np.allclose(g["breakpoint_vec"], v, atol=1e-6), (name, fx.L[b])
                compared += 1
        else:
            x_ref, ev_ref = orc.breakpoint_vector(g["Y"], g["U"], fx.breakpoints)
            assert g["lambda_min"][0] == pytest.approx(ev_ref[0], abs=1e-9)
            if w[1] - w[0] > 1e-6 and w[2] - w[1] > 1e-6 and abs(w[1] + 1e-10) > 1e-8:
                assert np.allclose(g["breakpoint_vec"], x_ref, atol=1e-6) or np.allclose(g["breakpoint_vec"], -x_ref, atol=1e-6), (name, fx.L[b])
                compared += 1
        rows = orc.build_rows(inst, cuts, fx.cut_type, reference_quirk_q1=fx.q1)
        assert len(rows) == int(z["R"][b])
        Theta = 0.5 * (g["Theta"] + g["Theta"].T)
        res = orc.primal_residuals(inst, rows, g["Y"], g["U"], g["X"], Theta)
        print(name, "L", fx.L[b], "iters", g["iters"], "residuals", res)
        assert res["max"] <= 2e-5 * max(1.0, np.abs(Theta).max()), (name, fx.L[b], res)
        assert orc.compute_SDP_relaxation_objective(g["X"], Theta, fx.A, fx.mask, fx.gamma) == pytest.approx(g["objective"], rel=1e-8)
    assert compared >= 2, "the separation vector was compared on fewer than two nodes"


# ---- b. certificates (test_gpu_certificate.py, sections 1 and 4) ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_certificates_reproduce_the_bound_on_numpy_and_on_the_device(fixtures, name):
    fx = fixtures(name)
    cert = fx.omc.pkg.certificate
    out, certs, _ = fx.kept()
    eng = fx.engine()
    dev = eng.dual_bound(fx.nodes, certs, fx.cut_type, reference_quirk_q1=fx.q1)
    Qs = eng.row_basis(fx.nodes, fx.cut_type, reference_quirk_q1=fx.q1)
    eng.close()
    for b, (o, c, node) in enumerate(zip(out, certs, fx.nodes)):
        val, df = cert.dual_bound(fx.A, fx.mask, fx.gamma, fx.k, node, fx.cut_type, c, q1=fx.q1, want_defects=True)
        rows = cert.node_rows(fx.n, fx.k, node, fx.cut_type, q1=fx.q1)
        ref = cert.evaluate(fx.A, fx.mask, fx.gamma, fx.k, rows, c)
        print(f"{name} L {fx.L[b]}: dual_bound {o['dual_bound']!r} numpy {val!r} shortfall {o['dual_bound'] - val:.3e} device {dev[b]!r} defects {df}")
        assert len(rows) == int(fx.z["R"][b]) and c.lam.shape == (len(rows),)
        assert c.Q.shape == (fx.n, int(fx.z["r"][b])) and c.Psi3.shape == (c.Q.shape[1] + fx.k,) * 2
        assert np.array_equal(Qs[b], c.Q)
        assert c.bound == o["dual_bound"]
        assert o["dual_bound"] - val <= REPRO * scale_of(o)
        assert df["off_support"] == 0.0 and df["min_lam"] >= 0.0
        obj = float(fx.z["objective"][b])                                    # the oracle certified it: within 1e-6 of the optimum
        assert val <= obj + OBJ_REL * max(1.0, abs(obj))
        assert val <= o["objective"] + OBJ_REL * max(1.0, abs(o["objective"]))
        assert abs(dev[b] - ref) <= 1e-7 * max(1.0, abs(ref))
        assert abs(dev[b] - o["dual_bound"]) <= REPRO * scale_of(o)


@pytest.mark.parametrize("name,L", [(K3, 9), (K8, 7), (K8, 9)])
def test_device_bound_of_random_multipliers(fixtures, name, L):
    """omc_dual_bound_batch against numpy on multipliers that are dense in every block (rank 3: Psi3 of order 15; rank 8: orders 23 and 25)."""
    fx = fixtures(name)
    cert = fx.omc.pkg.certificate
    node = fx.nodes[fx.at(L)]
    eng = fx.engine()
    Q = eng.row_basis([node], fx.cut_type, reference_quirk_q1=fx.q1)[0]
    rows = cert.node_rows(fx.n, fx.k, node, fx.cut_type, q1=fx.q1)
    assert np.allclose(Q, cert.row_basis(rows, fx.n, fx.k), atol=1e-13)
    c = random_multipliers(cert, np.random.default_rng(5), fx.mask, len(rows), Q, fx.k)
    dev = eng.dual_bound([node], [c], fx.cut_type, reference_quirk_q1=fx.q1)[0]
    eng.close()
    ref = cert.evaluate(fx.A, fx.mask, fx.gamma, fx.k, rows, c)
    print(f"{name} L {L}: device {dev!r} numpy {ref!r} diff {dev - ref:.3e}")
    assert abs(dev - ref) <= 1e-7 * max(1.0, abs(ref))


# ---- c. children by reference (test_gpu_branch.py, sections 1, 3 and 4) -----------------------------------------------------------------------
def grow(fx, device, L, max_iters):
    """The root and the listed node with L cuts, then every child of both through one held solve: by reference (device) or from their host
    cut lists.  Ids: 0, 1 the parents, 2 ... 2 + C the root's children in plan order, then those of the other parent."""
    ct, k = fx.cut_type, fx.k
    parents = [fx.nodes[0], fx.nodes[fx.at(L)]]
    eng = fx.engine()
    plan = eng.branch_plan(ct)
    C = len(plan)
    eng.reserve(2 * C, L + 1)
    eng.stage(parents, ct, fx.params(early_stop_factor=0.0, max_iters=max_iters))
    eng.hold(True); eng.submit()
    res = {}
    wait_for(eng, res, [0, 1])
    kids = list(range(2, 2 + 2 * C))
    cuts = {}
    for p in (0, 1):
        for c, child in enumerate(fx.omc.pkg.bnb.make_children(parents[p], res[p], ct, k)):
            cuts[2 + p * C + c] = child
    if device:
        assert eng.append_children([0, 1]) == kids
    else:
        eng.append([cuts[i] for i in kids], ct)
    assert eng.poll()["nodes_total"] == 2 + 2 * C
    wait_for(eng, res, kids)
    desc = {i: eng.fetch_descriptor(i) for i in [0, 1] + kids}
    eng.hold(False); eng.wait()
    info = eng.solver_info()
    eng.close()
    return dict(res=res, cuts=cuts, desc=desc, kids=kids, plan=plan, info=info)


@pytest.mark.parametrize("name,L,max_iters", [(K3, 7, 3000), (K4, 2, 400)])
def test_children_by_reference_equal_their_host_twins(fixtures, orc, name, L, max_iters):
    """Rank 3, linear: 2^3 = 8 children of the root and of the node with 7 cuts (8 rows active there), solved to the end.  Rank 4, linear3:
    4^4 = 256 children of the root and of the node with 2 cuts, capped at 400 iterations as the larger instances of test_gpu_branch.py are
    (two engines, the same cap).  Descriptors and relaxations equal byte for byte; child c carries branch_plan's tuple c."""
    fx = fixtures(name)
    k = fx.k
    host, dev = grow(fx, False, L, max_iters), grow(fx, True, L, max_iters)
    plan = dev["plan"]
    C = len(plan)
    assert C == len(orc.DIRECTIONS_OF[fx.cut_type]) ** k
    assert plan == [tuple(d) for d in orc.child_directions(fx.cut_type, k)]
    assert dev["info"]["R_max"] == host["info"]["R_max"] and dev["info"]["r_max"] == host["info"]["r_max"]
    ids = [0, 1] + dev["kids"]
    assert sorted(dev["res"]) == sorted(host["res"]) == ids
    for i in ids:
        assert_same_descriptor(dev["desc"][i], host["desc"][i], (name, i))
        assert_padding_is_zero(dev["desc"][i], (name, i))
        a, b = dev["res"][i], host["res"][i]
        assert all(a[q] == b[q] for q in KEYS), (name, i, [a[q] for q in KEYS], [b[q] for q in KEYS])
        assert a["U"].tobytes() == b["U"].tobytes() and a["breakpoint_vec"].tobytes() == b["breakpoint_vec"].tobytes(), (name, i)
    for p, Lp in ((0, 0), (1, L)):
        dp = dev["desc"][p]
        for c in range(C):
            i = 2 + p * C + c
            assert tuple(host["cuts"][i][-1][2]) == plan[c]               # the host twin of child c was built from plan[c]
            d = dev["desc"][i]
            assert (d["L"], d["R"], d["r"]) == (Lp + 1, dp["R"] + 2 * k + 1, min(fx.n, dp["r"] + 1))
            assert d["rcut"][d["R"] - 1] == Lp and d["rkind"][d["R"] - 1] == 3     # the last row is the cut row of the new cut
    print(name, "children", 2 * C, "statuses", sorted(set(dev["res"][i]["status_code"] for i in dev["kids"])))


# ---- d. arms that must agree bit for bit (test_small_chain.py, test_global_schedule.py) -------------------------------------------------------
def solve_arm(eng, fx, nodes, P, env):
    for key, v in env.items():
        eng.tuning_set(key, v)
    try:
        return eng.matrix_completion_SDP_relaxation(nodes, fx.cut_type, params=P, want_X=False), eng.solver_info()
    finally:
        for key in env:
            eng.tuning_set(key, None)


@pytest.mark.parametrize("name,Ls", [(K5, (9,)), (K8, (2, 7, 8)), (K8, (7, 9))])
def test_arms_agree_bit_for_bit(fixtures, name, Ls):
    """One rank-5 node (r = 14, N3 = 19); rank-8 nodes with r <= 16 (small_proj_chain; N3 up to 24: the MFMA products) at the stride
    rmax = 16; and the rank-8 node with r = 17 (the scalar body in both arms of OMC_SMALL_CHAIN) next to one with r = 15 at the stride
    rmax = 17: the path is chosen per node, the strides per batch.  300 iterations, nothing stops early."""
    fx = fixtures(name)
    nodes = [fx.nodes[fx.at(L)] for L in Ls]
    P = fx.params(max_iters=300, eps_gap=1e-14)
    eng = fx.engine()
    base, info = solve_arm(eng, fx, nodes, P, {})
    assert info["r_max"] == fx.k + max(Ls) and info["global_lds"] and info["small_lds"]
    for env in ({"OMC_SMALL_CHAIN": "0"}, {"OMC_DENSE_PROJ": "1"}, {"OMC_GLOBAL_NOLDS": "1"}):
        arm, info = solve_arm(eng, fx, nodes, P, env)
        assert info["global_lds"] == ("OMC_GLOBAL_NOLDS" not in env)
        for L, a, b in zip(Ls, base, arm):
            assert a["iters"] == 300
            assert all(a[q] == b[q] for q in ARM_KEYS), (name, L, env, [a[q] for q in ARM_KEYS], [b[q] for q in ARM_KEYS])
            assert np.array_equal(a["Y"], b["Y"]), (name, L, env)
    eng.close()


# ---- e. warm start (test_gpu_parity.py::test_warm_start_same_optimum_fewer_iterations_and_oracle_mirror) ---------------------------------------
@pytest.mark.parametrize("name,L", [(K3, 9), (K8, 9)])
def test_warm_start_from_the_parent(fixtures, name, L):
    """The listed node with L cuts from the final state of its parent (L - 1 cuts, listed too) through the state pool: the same certified
    value (2e-6, against the oracle's recorded objective and the cold solve) in no more iterations than from a cold start.  The nodes are
    those where the oracle's own warm start (sdp_relaxation(warm=...), the same state transfer) saves iterations: 450 against 500 cold at
    rank 3, 625 against 800 at rank 8 (r = 17: Vt, D3V and the small-cone duals start at the stride of the deepest node)."""
    fx = fixtures(name)
    b = fx.at(L)
    assert fx.L[b - 1] == L - 1
    P = fx.params()
    eng = fx.engine()
    eng.state_pool_create(2)
    parent = eng.matrix_completion_SDP_relaxation([fx.nodes[b - 1]], fx.cut_type, params=P, save_to=[0], want_X=False)[0]
    cold = eng.matrix_completion_SDP_relaxation([fx.nodes[b]], fx.cut_type, params=P, want_X=False)[0]
    warm = eng.matrix_completion_SDP_relaxation([fx.nodes[b]], fx.cut_type, params=P, load_from=[0], save_to=[1], want_X=False)[0]
    eng.close()
    print(name, "L", L, "parent", parent["iters"], "cold", cold["iters"], cold["objective"], "warm", warm["iters"], warm["objective"])
    assert parent["status_code"] == 0 and cold["status_code"] == 0 and warm["status_code"] == 0
    assert_finite(warm)
    assert warm["objective"] == pytest.approx(float(fx.z["objective"][b]), rel=OBJ_REL)
    assert warm["objective"] == pytest.approx(cold["objective"], rel=OBJ_REL)
    assert abs(warm["objective"] - warm["dual_bound"]) <= 1.01e-6 * max(1.0, abs(warm["objective"]))
    assert warm["iters"] <= cold["iters"]


# ---- f. slots (test_gpu_parity.py::test_continuous_batching_slots) ----------------------------------------------------------------------------
def test_rank8_nodes_through_two_slots(fixtures):
    """Ten nodes, R from 37 to 190 and r from 8 to 17, through 2 slots: a slot is re-initialised for a node of another size."""
    fx = fixtures(K8)
    ref, _, _ = fx.kept()
    eng = fx.engine()
    out = eng.matrix_completion_SDP_relaxation(fx.nodes, fx.cut_type, params=fx.params(slots=2), want_Theta=True)
    eng.close()
    assert len(out) == len(ref) > 2
    for L, a, b in zip(fx.L, out, ref):
        assert all(a[q] == b[q] for q in ARM_KEYS), (L, [a[q] for q in ARM_KEYS], [b[q] for q in ARM_KEYS])
        for key in ("Y", "U", "X", "Theta", "breakpoint_vec", "lambda_min"):
            assert a[key].tobytes() == b[key].tobytes(), (L, key)
