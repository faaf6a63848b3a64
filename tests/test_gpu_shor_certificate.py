"""GPU tests of the exported Shor-mode certificates (run on the MI355X box: `pytest -m gpu`).

A Shor node's dual_bound is re-evaluated from the exported multipliers by certificate.shor_dual_bound (numpy, sanitised: a valid bound whatever
the engine exported).  Shapes are those of test_gpu_shor.py (12 x 14 / 152 minors, 20 x 24 / about 150, the cut nodes at the 1500 cap) and, for
the schedules, the six nodes of test_gpu_shor_append.py (10 x 12, 208 and 104 minors, root / left / right).

Conditions (the project's, nothing is pinned to the reference: Julia + Mosek, no fixtures).  REPRO = 1e-7 max(1, |objective|): how far the
sanitised numpy bound may fall below the reported dual_bound, a tenth of eps_gap as in test_gpu_certificate.py.  OBJ_REL = 2e-6 against the
oracle's certified objective."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GAMMA = 80.0
OBJ_REL = 2e-6
REPRO = 1e-7
KEYS = ("objective", "dual_bound", "iters", "status_code")
FIELDS = ("scale", "lam", "Q", "Psi3", "Gam", "zeta", "xi", "Xbar", "bound")


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


def _instance(orc, n, m, nidx, seed, noise, kind="lowrank"):
    A, mask = orc.make_instance(n, m, 1, n_indices=nidx, seed=seed, noise=noise, kind=kind)
    return A, mask, orc.Instance(A, mask, GAMMA, 1)


def _thin(minors, target, seed):
    rng = np.random.default_rng(seed)
    return [q for q in minors if rng.random() < target / max(len(minors), 1)]


def _shor(eng, nodes, info, params, **kw):
    return eng.matrix_completion_SDP_relaxation(nodes, "linear", params, add_Shor_valid_inequalities=True, shor_info=info, want_Theta=True, **kw)


def _same_certificate(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def _check(omc, tag, A, mask, node, minors, o, c, upper=None):
    """The assertions every exported certificate must pass; `upper`: a value the optimum cannot exceed.  Returns (numpy bound, shortfall)."""
    cert = omc.pkg.certificate
    val, df = cert.shor_dual_bound(A, mask, GAMMA, node, "linear", minors, None, c, want_defects=True)
    sc = max(1.0, abs(o["objective"]))
    print(f"{tag}: status {o['status_code']} iters {o['iters']} objective {o['objective']!r} dual_bound {o['dual_bound']!r} numpy {val!r} "
          f"shortfall {o['dual_bound'] - val:.3e} cap {REPRO * sc:.3e} defects {df}")
    assert c.bound == o["dual_bound"]                                     # the certificate of the check that gave the reported bound
    assert len(c.Gam) == len(minors)
    assert o["dual_bound"] - val <= REPRO * sc
    if upper is not None:
        assert val <= upper + OBJ_REL * max(1.0, abs(upper))
    return val, o["dual_bound"] - val


class Env12:
    """12 x 14 / 152 minors: instance, lists, the cut nodes of test_cut_nodes_with_minors..., the oracle's certified root (once)."""

    def __init__(self, omc, orc, sh):
        self.A, self.mask, self.inst = _instance(orc, 12, 14, 70, 2, 0.1)
        self.minors, self.soc = sh.driver_shor_lists(self.mask, (4,))
        assert len(self.minors) == 152
        cuts = []; self.nodes = [[]]
        for d in range(2):
            r0 = orc.sdp_relaxation(self.inst, cuts=cuts)
            x, _ = orc.breakpoint_vector(r0["Y"], r0["U"])
            cuts = cuts + [(x, r0["U"], ["left" if d % 2 == 0 else "right"])]
            self.nodes.append(list(cuts))
        self.ro = sh.sdp_relaxation_shor(self.inst, self.minors, self.soc, params=sh.ShorParams(eps_gap=1e-6))
        assert self.ro["termination_status"] == 0
        self.P_root = omc.default_params(eps_gap=1e-6, max_iters=6000)
        self.P_cap = omc.default_params(eps_gap=1e-12, max_iters=1500)
        eng = omc.Engine(self.A, self.mask, GAMMA, 1)
        eng.keep_shor_certificates(True)
        self.root = _shor(eng, [[]], [(self.minors, None)], self.P_root)[0]
        self.root_cert = eng.fetch_shor_certificate([0])[0]
        self.capped = _shor(eng, self.nodes[1:], [(self.minors, None)] * 2, self.P_cap)
        self.capped_certs = eng.fetch_shor_certificate([0, 1])
        eng.close()


@pytest.fixture(scope="module")
def env12(have_gpu, omc, orc, sh):
    return Env12(omc, orc, sh)


# ---- 1. reproduction ----------------------------------------------------------------------------------------------------------------------------
def test_root_certificate_reproduces_the_bound_and_is_valid(env12, omc):
    """Measured on the MI355X: see DESIGN.md section 3.12b."""
    e = env12
    assert e.root["status_code"] == 0
    _check(omc, "12x14/152 root", e.A, e.mask, [], e.minors, e.root, e.root_cert, upper=float(e.ro["objective"]))
    assert e.root_cert.scale == pytest.approx(e.ro["scale"], rel=1e-14)


def test_20x24_certificate_reproduces_the_bound_and_is_valid(have_gpu, omc, orc, sh):
    A, mask, inst = _instance(orc, 20, 24, 150, 5, 0.05)
    minors = _thin(orc.shor_constraints_indexes(mask, [4]), 150, 5)
    minors, soc = sh.driver_shor_lists(mask, minors=minors)
    assert 100 <= len(minors) <= 200
    eng = omc.Engine(A, mask, GAMMA, 1)
    eng.keep_shor_certificates(True)
    r = _shor(eng, [[]], [(minors, None)], omc.default_params(eps_gap=1e-6, max_iters=8000))[0]
    c = eng.fetch_shor_certificate([0])[0]
    eng.close()
    ro = sh.sdp_relaxation_shor(inst, minors, soc, params=sh.ShorParams(eps_gap=1e-6, max_iters=8000))
    assert r["status_code"] == 0 and ro["termination_status"] == 0
    _check(omc, f"20x24/{len(minors)} root", A, mask, [], minors, r, c, upper=float(ro["objective"]))


# ---- 2. the best check, not the last one ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
def test_cut_node_certificate_is_of_the_best_check(env12, omc, d):
    """Depth-1 and depth-2 cut nodes at the 1500 cap with eps_gap = 1e-12: rows, small cone and the penalty bump are exercised, and the reported
    bound may come from an earlier check than the last.  The numpy bound stays below the node's own objective at the cap."""
    e = env12
    o, c = e.capped[d - 1], e.capped_certs[d - 1]
    assert o["iters"] == 1500
    _check(omc, f"12x14/152 depth {d}", e.A, e.mask, e.nodes[d], e.minors, o, c, upper=o["objective"])
    assert len(c.lam) == 2 + 3 * d and c.Q.shape == (12, 1 + d)


# ---- 3. column types 1 and 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", [2, 1])
def test_column_types_on_the_device(have_gpu, omc, orc, sh, ctype):
    """Fully observed 6 x 7: every class-4 minor (every column an equality, type 2) and the list thinned to rows 1-4 (rows 5 and 6 stay outside
    the minors and are observed: the slack is paid for, type 1)."""
    A, mask = orc.make_instance(6, 7, 1, n_indices=42, seed=7, noise=0.1)
    assert mask.all()
    inst = orc.Instance(A, mask, GAMMA, 1)
    allm = orc.shor_constraints_indexes(mask, [4])
    minors = allm if ctype == 2 else [q for q in allm if q[1] <= 4]
    minors, soc = sh.driver_shor_lists(mask, minors=minors)
    assert (omc.pkg.certificate.shor_structure(6, 7, mask, minors, None).ctype == ctype).all()
    eng = omc.Engine(A, mask, GAMMA, 1)
    eng.keep_shor_certificates(True)
    r = _shor(eng, [[]], [(minors, None)], omc.default_params(eps_gap=1e-6, max_iters=8000))[0]
    c = eng.fetch_shor_certificate([0])[0]
    eng.close()
    ro = sh.sdp_relaxation_shor(inst, minors, soc, params=sh.ShorParams(eps_gap=1e-6, max_iters=8000))
    assert ro["termination_status"] == 0 and r["status_code"] == 0
    _check(omc, f"6x7/{len(minors)} type {ctype}", A, mask, [], minors, r, c, upper=float(ro["objective"]))


# ---- 4. schedule independence -------------------------------------------------------------------------------------------------------------------------
class Env10:
    pass


@pytest.fixture(scope="module")
def env10(have_gpu, omc, orc, sh):
    """The six nodes of test_gpu_shor_append.py and their certificates from one staged batch through two slots."""
    e = Env10()
    e.A, e.mask = orc.make_instance(10, 12, 1, n_indices=60, seed=2, noise=0.1)
    inst = orc.Instance(e.A, e.mask, GAMMA, 1)
    e.full, soc = sh.driver_shor_lists(e.mask, (4,))
    assert len(e.full) == 208
    e.half = e.full[:104]
    e.o_root = sh.sdp_relaxation_shor(inst, e.full, soc, params=sh.ShorParams(eps_gap=1e-5, max_iters=6000))
    assert e.o_root["termination_status"] == 0
    x = orc.breakpoint_vector(e.o_root["Y"], e.o_root["U"])[0]
    left = [(x, e.o_root["U"], ["left"])]; right = [(x, e.o_root["U"], ["right"])]
    e.nodes = [[], left, right, [], left, right]
    e.lists = [e.full] * 3 + [e.half] * 3
    e.info = [(l, None) for l in e.lists]
    e.P1 = omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0, slots=1)
    e.P2 = omc.default_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0, slots=2)
    e.eng = omc.Engine(e.A, e.mask, GAMMA, 1)
    e.eng.keep_shor_certificates(True)
    e.ref = _shor(e.eng, e.nodes, e.info, e.P2, want_Y=False)
    e.certs = e.eng.fetch_shor_certificate(range(6))
    yield e
    e.eng.close()


def test_staged_certificates_reproduce(env10, omc):
    e = env10
    for i in range(6):
        assert e.ref[i]["status_code"] == 0
        _check(omc, f"10x12 node {i}", e.A, e.mask, e.nodes[i], e.lists[i], e.ref[i], e.certs[i],
               upper=float(e.o_root["objective"]) if i == 0 else None)


def test_certificates_do_not_depend_on_the_schedule(env10, omc):
    e = env10; eng = e.eng
    # through one slot
    one = _shor(eng, e.nodes, e.info, e.P1, want_Y=False)
    c1 = eng.fetch_shor_certificate(range(6))
    # two staged, four appended to the held solve, certificates fetched by id while it runs
    eng.tuning_set("OMC_NO_GRAPH", "1")
    try:
        eng.reserve(4, 1); eng.reserve_shor(208, 1)
        eng.stage_shor(e.nodes[:2], e.info[:2], "linear", e.P2)
        eng.hold(True)
        eng.submit()
        with pytest.raises(omc.OmcError):
            eng.keep_shor_certificates(False)                               # refused while a solve runs
        with pytest.raises(omc.OmcError):
            eng.fetch_shor_certificate([0])                                 # fetch_done has not returned it yet
        eng.append_shor(e.nodes[2:], e.info[2:], "linear")
        got = {}
        t0 = time.monotonic()
        while len(got) < 6:
            assert time.monotonic() - t0 < 120.0
            for r in eng.fetch_done():
                got[r["node"]] = (r, eng.fetch_shor_certificate([r["node"]])[0])
        assert eng.poll()["running"]
        with pytest.raises(omc.OmcError) as err:
            eng.fetch_shor_certificate([6])                                 # id = capacity
        assert err.value.code == -3
        eng.hold(False)
        eng.wait()
    finally:
        eng.tuning_set("OMC_NO_GRAPH", None)
    after = eng.fetch_shor_certificate(range(6))
    for i in range(6):
        assert all(one[i][key] == e.ref[i][key] for key in KEYS) and all(got[i][0][key] == e.ref[i][key] for key in KEYS)
        for c in (c1[i], got[i][1], after[i]):
            for f in FIELDS:
                assert np.array_equal(getattr(c, f), getattr(e.certs[i], f)), (i, f)


def test_warm_started_node_still_reproduces(env10, omc):
    """Parent root/104 saves its state, child root/208 starts from it: the certificate reproduces the reported bound and is valid (bit identity
    with the cold run is not asked)."""
    e = env10
    eng = omc.Engine(e.A, e.mask, GAMMA, 1)
    try:
        eng.state_pool_create(2); eng.state_pool_reserve_shor(208)
        eng.keep_shor_certificates(True)
        _shor(eng, [[]], [(e.half, None)], e.P1, want_Y=False, save_to=[0])
        r = _shor(eng, [[]], [(e.full, None)], e.P1, want_Y=False, load_from=[0])[0]
        assert eng.shor_warm_stats()["loaded_prefix"] == 1 and r["status_code"] == 0 and r["iters"] < e.ref[0]["iters"]
        _check(omc, "10x12 warm child", e.A, e.mask, [], e.full, r, eng.fetch_shor_certificate([0])[0], upper=float(e.o_root["objective"]))
    finally:
        eng.close()


# ---- 5. switches --------------------------------------------------------------------------------------------------------------------------------------
def test_switches(env12, omc, orc):
    e = env12
    eng = omc.Engine(e.A, e.mask, GAMMA, 1)
    P = omc.default_params(eps_gap=1e-6, max_iters=200)
    try:
        eng.keep_certificates(True)                                        # the base switch alone: the refusal stands
        with pytest.raises(omc.OmcError) as err:
            eng.stage_shor([[]], [(e.minors, None)], "linear", P)
        assert err.value.code == -4
        eng.keep_shor_certificates(True)                                   # with the Shor switch it stages, whatever the base switch says
        eng.stage_shor([[]], [(e.minors, None)], "linear", P)
        with pytest.raises(omc.OmcError) as err:
            eng.fetch_shor_certificate([0])                                # staged, not solved
        assert err.value.code == -3
        eng.solve()
        assert eng.fetch_shor_certificate([0])[0].bound == eng.fetch()[0]["dual_bound"]
        with pytest.raises(omc.OmcError) as err:
            eng.fetch_shor_certificate([1])                                # id = capacity
        assert err.value.code == -3
        with pytest.raises(omc.OmcError):
            eng.fetch_certificate([0])                                     # a Shor batch has no base certificate
        eng.keep_certificates(False)
        eng.stage_shor([[]], [(e.minors, None)], "linear", P)              # and with the base switch off
        # the Shor switch has no effect on stage(): with it alone nothing is kept there, with the base switch the base certificate is what it was
        base_off = eng.matrix_completion_SDP_relaxation([[]], "linear", omc.default_params(rho_scale=4.0), want_X=False)[0]
        with pytest.raises(omc.OmcError):
            eng.fetch_certificate([0])
        with pytest.raises(omc.OmcError):
            eng.fetch_shor_certificate([0])
        eng.keep_shor_certificates(False)
        plain = eng.matrix_completion_SDP_relaxation([[]], "linear", omc.default_params(rho_scale=4.0), want_X=False)[0]
        assert all(plain[key] == base_off[key] for key in KEYS) and np.array_equal(plain["Y"], base_off["Y"])
        # staged without the switch
        eng.stage_shor([[]], [(e.minors, None)], "linear", P)
        eng.solve()
        with pytest.raises(omc.OmcError) as err:
            eng.fetch_shor_certificate([0])
        assert err.value.code == -3 and "keep_shor_certificates" in str(err.value)
    finally:
        eng.close()
    # rank 2 with the switch: unsupported
    A2, mask2 = orc.make_instance(12, 14, 2, n_indices=90, seed=3, noise=0.1)
    eng2 = omc.Engine(A2, mask2, GAMMA, 2)
    try:
        eng2.keep_shor_certificates(True)
        with pytest.raises(omc.OmcError) as err:
            eng2.stage_shor([[]], [([], None)], "linear")
        assert err.value.code == -4
        eng2.keep_shor_certificates(False)
        eng2.stage_shor([[]], [([], None)], "linear")
    finally:
        eng2.close()


# ---- 6. off means off ---------------------------------------------------------------------------------------------------------------------------------
def test_keeping_shor_certificates_changes_nothing(env12, omc):
    e = env12
    eng = omc.Engine(e.A, e.mask, GAMMA, 1)                                # the switch is never touched on this engine
    try:
        root = _shor(eng, [[]], [(e.minors, None)], e.P_root)[0]
        capped = _shor(eng, e.nodes[1:2], [(e.minors, None)], e.P_cap)[0]
        W = eng.fetch_shor()[0]
        with pytest.raises(omc.OmcError) as err:
            eng.fetch_shor_certificate([0])
        assert err.value.code == -3
    finally:
        eng.close()
    for off, on in ((root, e.root), (capped, e.capped[0])):
        print(f"switch off {[off[key] for key in KEYS]} on {[on[key] for key in KEYS]}")
        assert all(off[key] == on[key] for key in KEYS)
        for q in ("X", "W", "Theta"):
            assert np.array_equal(off[q], on[q]), q
    assert np.array_equal(W, capped["W"])
