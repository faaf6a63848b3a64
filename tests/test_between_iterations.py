"""The path between the ADMM iterations: k_setup_gram (the rows' Gram matrix on a grid of its own, beside the harvest) against the
serial walk inside k_setup (OMC_SETUP_GRAM_INLINE=1), k_check_build with the active rows listed once against the CPU oracle (or, bit
for bit, against another build of the library named by OMC_PARENT_LIB), and the launch / time accounting of a solve that crosses
several checks and harvests with the timing events read one interval late.

Shapes: 24 x 30, rank 1 and 2 (the instance of smoke()); a node costs milliseconds.  At rank 1 a node with L cuts has
R = 2 + 3 L rows, so 0, 1, 2 and 6 cuts give 3, 15, 36 and 210 row pairs: one chunk of 8 pairs that is not full, and chunk counts
with a ragged last chunk.  The frontier the cases draw their nodes from is expanded once per module."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0
OBJ_REL = 2e-6          # tests/test_gpu_parity.py: objective and certified dual bound against the oracle
INLINE = {"OMC_SETUP_GRAM_INLINE": "1"}
SCALARS = ("objective", "dual_bound", "iters", "status_code")
ARRAYS = ("Y", "U", "lambda_min", "breakpoint_vec")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def have_gpu(omc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


def _instance(omc, k):
    return omc.pkg.data.generate_matrix_completion_data(k, 24, 30, int(0.35 * 24 * 30), seed=3)


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
        assert tuple(x[s] for s in SCALARS) == tuple(y[s] for s in SCALARS)
        for s in ARRAYS:
            assert np.array_equal(x[s], y[s], equal_nan=True), s


@pytest.fixture(scope="module")
def fam(have_gpu, omc):
    """Engine at rank 1 and the frontiers of depth 2 and 6 (nodes with 2 and with 6 cuts), expanded once with the default arm."""
    A, mask = _instance(omc, 1)
    eng = omc.Engine(A, mask, GAMMA, 1)
    Pe = omc.default_params(rho_scale=4.0, max_iters=400)
    n2, _ = omc.pkg.bnb.expand_frontier(eng, 2, "linear", params=Pe)
    n6, _ = omc.pkg.bnb.expand_frontier(eng, 6, "linear", params=Pe)
    assert len(n2) >= 2 and len(n6) >= 12 and all(len(c) == 6 for c in n6)
    yield dict(eng=eng, A=A, mask=mask, n2=n2, n6=n6, P=omc.default_params(rho_scale=4.0, max_iters=300))
    eng.close()


def test_gram_root_two_rows(fam, omc):
    """R = 2 (trace and one box row), no cuts: three pairs, one workgroup of k_setup_gram."""
    eng, P = fam["eng"], fam["P"]
    a = _run(eng, [[]], P, {})
    assert eng.solver_info()["R_max"] == 2
    _same(a, _run(eng, [[]], P, INLINE))


def test_gram_rank_two_box_rows(have_gpu, omc):
    """k = 2: the box rows' coefficient stride (rcoef has k entries per row) and their (i, j) positions; root and four children."""
    A, mask = _instance(omc, 2)
    eng = omc.Engine(A, mask, GAMMA, 2)
    P = omc.default_params(rho_scale=4.0, max_iters=300)
    root = _run(eng, [[]], P, {})
    nodes = [[]] + omc.pkg.bnb.make_children([], root[0], "linear", 2)[:4]
    a = _run(eng, nodes, P, {})
    assert eng.solver_info()["R_max"] == 1 + 3 + 5          # 1 + k (k + 1) / 2 + L (2 k + 1) rows with L = 1 cut
    _same(a, _run(eng, nodes, P, INLINE))
    eng.close()


@pytest.mark.parametrize("cuts", [1, 2, 6])
def test_gram_ragged_pair_chunks(fam, cuts):
    """1, 2 and 6 cuts: 15, 36 and 210 row pairs, none a multiple of the chunk of 8; every kind of pair (trace, box, bound, cut)."""
    eng, P = fam["eng"], fam["P"]
    nodes = [fam["n6"][0][:cuts], fam["n6"][-1][:cuts]]
    a = _run(eng, nodes, P, {})
    assert eng.solver_info()["R_max"] == 2 + 3 * cuts
    _same(a, _run(eng, nodes, P, INLINE))


def test_gram_two_identical_cuts(fam):
    """The same cut twice: two equal rows for each of its three rows, a singular Gram matrix (the ridge of the row projection matters)."""
    eng, P = fam["eng"], fam["P"]
    c = fam["n6"][0][0]
    nodes = [[c, c], [c, fam["n6"][0][1], c]]
    _same(_run(eng, nodes, P, {}), _run(eng, nodes, P, INLINE))


def test_gram_beside_a_harvest(fam, omc):
    """12 nodes through 4 slots: k_setup_gram runs beside the harvest of the slots' previous nodes, from a job list that differs from
    node_of; and 3 nodes through 1 slot: every refill is of a single slot.  The results are those of one node per slot as well."""
    eng = fam["eng"]
    nodes = fam["n6"][:12]
    P4 = omc.default_params(rho_scale=4.0, max_iters=300, slots=4)
    a = _run(eng, nodes, P4, {})
    _same(a, _run(eng, nodes, P4, INLINE))
    _same(a, _run(eng, nodes, fam["P"], {}))
    P1 = omc.default_params(rho_scale=4.0, max_iters=300, slots=1)
    b = _run(eng, nodes[:3], P1, {})
    _same(b, _run(eng, nodes[:3], P1, INLINE))
    _same(b, a[:3])


def test_gram_for_appended_nodes(fam, omc):
    """refill_idle: two nodes staged into four slots, eight more appended while the held solve is running; they reach the idle slots
    (and, later, harvested ones) with their Gram matrices formed from the appended descriptors."""
    eng = fam["eng"]
    nodes = fam["n6"][:10]
    P4 = omc.default_params(rho_scale=4.0, max_iters=300, slots=4)
    ref = _run(eng, nodes, P4, {})

    def appended(env):
        for k_, v in env.items():
            eng.tuning_set(k_, v)
        try:
            eng.reserve(8, 6)
            eng.stage(nodes[:2], "linear", P4)
            eng.hold(True)
            eng.submit()
            eng.append(nodes[2:], "linear")
            eng.hold(False)
            eng.wait()
            return eng.fetch(want_X=False)
        finally:
            for k_ in env:
                eng.tuning_set(k_, None)

    _same(ref, appended({}))
    _same(ref, appended(INLINE))


# ---- k_check_build -------------------------------------------------------------------------------------------------------------------

def _check_cases(omc, eng, n2, n6):
    """What the k_check_build tests solve, by name: lists of results."""
    out = {}
    # no cut rows, first check after ONE iteration from the cold start: the cut list is empty and M = -rho E3 - gamma/2 L L'.  (The
    # multipliers are never all zero at a check: the trace row is active from the first iteration on -- the oracle has
    # lam = [1.40, 0] after it on this instance -- so the list of active rows holds the trace row, whose coefficient on U is zero.)
    out["cold"] = _run(eng, [[]], omc.default_params(rho_scale=4.0, max_iters=1, check_every=1), {})
    out["first"] = _run(eng, [[]], omc.default_params(rho_scale=4.0, max_iters=25), {})
    P = omc.default_params(rho_scale=4.0)
    for xs in ("16", "1", "0"):      # staged vectors: all, one (the second active cut row reads global memory), none
        out["depth2_xs" + xs] = _run(eng, n2[:2], P, {"OMC_CHECK_XS": xs})
        out["depth6_xs" + xs] = _run(eng, n6[:4], P, {"OMC_CHECK_XS": xs})
    return out


@pytest.fixture(scope="module")
def check_cases(fam, omc):
    return _check_cases(omc, fam["eng"], fam["n2"], fam["n6"])


def test_check_build_first_check_from_cold_start(fam, check_cases, orc):
    """The first check of a cold start: after one iteration (check_every = 1) and after 25.  This stands in for the case "all multipliers
    zero at the first check", which does not occur: the column prox raises Y from its start k/n I, whose trace is exactly k, so the trace
    row is violated by the first averaged iterate and its multiplier is positive from iteration 1 on (asserted below on the oracle's lam;
    1.40 on this instance).  What the case was to reach is reached: the list of cut rows is empty (nc = 0, Mchk = -rho E3 - gamma/2 L L')
    and the only listed row, the trace row, has a zero coefficient on U; an empty list of active rows (na = 0) is the same two loops with
    zero trips and cannot be produced by a solve."""
    inst = orc.Instance(fam["A"], fam["mask"], GAMMA, 1)
    for name, mi, ce in (("cold", 1, 1), ("first", 25, 25)):
        g = check_cases[name][0]
        r = orc.sdp_relaxation(inst, [], "linear", params=orc.RelaxParams(rho_scale=4.0, max_iters=mi, check_every=ce), want_certificate=False)
        print(name, g["objective"], r["objective"], g["dual_bound"], r["dual_bound"], r["lam"])
        assert list(r["rows"].kinds) == ["trace", "box_lo"] and r["lam"][0] > 0.0 and r["lam"][1] == 0.0
        assert g["iters"] == r["iters"] == mi and g["status_code"] == r["termination_status"]
        assert g["objective"] == pytest.approx(r["objective"], rel=OBJ_REL)
        assert g["dual_bound"] == pytest.approx(r["dual_bound"], rel=OBJ_REL)


def test_check_build_cut_rows_staged_and_from_global_memory(fam, check_cases, orc):
    """Nodes with 2 and with 6 cuts at OMC_CHECK_XS = 16 (every listed cut vector in LDS), 1 and 0 (the remainder path: the vectors
    of the listed cut rows beyond the staged ones come from global memory): the three arms agree bit for bit, and the depth-2 nodes
    agree with the oracle.  That cut rows are listed at a check is taken from the oracle, which runs the same iteration: at its check of
    iteration 100 the first depth-6 node has at least two cut rows with a nonzero multiplier, so OMC_CHECK_XS = 0 and = 1 both leave
    listed cut rows to the global-memory loop."""
    inst = orc.Instance(fam["A"], fam["mask"], GAMMA, 1)
    r6 = orc.sdp_relaxation(inst, fam["n6"][0], "linear", params=orc.RelaxParams(rho_scale=4.0, max_iters=100), want_certificate=False)
    active_cuts = [l for kind, l in zip(r6["rows"].kinds, r6["lam"]) if kind == "cut" and l != 0.0]
    print("depth 6, iteration 100: multipliers of the cut rows", active_cuts)
    assert r6["iters"] == 100 and len(active_cuts) >= 2
    assert check_cases["depth6_xs16"][0]["iters"] >= 100          # the GPU node was still running at that check
    for d in ("depth2", "depth6"):
        _same(check_cases[d + "_xs16"], check_cases[d + "_xs1"])
        _same(check_cases[d + "_xs16"], check_cases[d + "_xs0"])
    certified = 0
    for cuts, g in zip(fam["n2"][:2], check_cases["depth2_xs16"]):
        r = orc.sdp_relaxation(inst, cuts, "linear", params=orc.RelaxParams(rho_scale=4.0), want_certificate=False)
        kinds = [getattr(row, "kind", None) for row in r["rows"]] if not hasattr(r["rows"], "kinds") else list(r["rows"].kinds)
        print("depth 2:", g["status_code"], g["objective"], r["objective"], g["dual_bound"], r["dual_bound"], r["lam"], kinds)
        assert g["status_code"] == r["termination_status"]
        if g["status_code"] == 3:
            continue
        assert g["objective"] == pytest.approx(r["objective"], rel=OBJ_REL)
        if g["status_code"] == 0:
            certified += 1
            assert g["dual_bound"] == pytest.approx(r["dual_bound"], rel=OBJ_REL)
    assert certified >= 1


def test_check_build_against_another_build(fam, check_cases, omc, tmp_path):
    """With OMC_PARENT_LIB naming another build of the library (the parent commit's), the same cases run there in a child process and
    every result must be bit-identical.  Without it the oracle comparisons above are the check and this test has nothing to add."""
    parent = os.environ.get("OMC_PARENT_LIB")
    if not parent:
        return
    out = str(tmp_path / "parent.npz")
    env = dict(os.environ, OMC_AMD_LIB=parent)
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, timeout=300)
    z = np.load(out)
    for name, res in check_cases.items():
        if name.endswith("_xs1") or name.endswith("_xs0"):
            continue                                   # the other build has no such knob
        for i, o in enumerate(res):
            for s in SCALARS + ARRAYS:
                assert np.array_equal(np.asarray(o[s]), z[f"{name}/{i}/{s}"], equal_nan=True), (name, i, s)


# ---- accounting ----------------------------------------------------------------------------------------------------------------------

def test_kernel_stats_over_checks_and_harvests(fam, omc):
    """20 nodes through 4 slots, 100 iterations each (eps_gap far below reach): five rounds in lockstep, so 500 iterations, 20 checks,
    5 harvests, 5 setups.  The launches of every class follow from those counts -- k_setup_gram adds its time to the setup class but
    is not a launch of it -- and every class that launched has its time, although the events are read one interval late."""
    eng = fam["eng"]
    pair = [[], fam["n2"][0][:1]]                                # the root and its first child: both feasible (they are smoke()'s nodes)
    nodes = [pair[i % 2] for i in range(20)]
    P = omc.default_params(rho_scale=4.0, max_iters=100, eps_gap=1e-14, slots=4)
    out = _run(eng, nodes, P, {})
    assert all(o["iters"] == 100 for o in out), [o["iters"] for o in out]
    iters = 100 * (len(nodes) // 4)
    checks = iters // 25
    ks = eng.kernel_stats()
    print(ks)
    for cls in ("global", "colprox", "small"):
        assert ks[cls]["launches"] == iters, cls
    assert ks["cone"]["launches"] in (iters, 2 * iters)          # one launch, or the two phases beside / behind k_cone_sub
    assert ks["cone_sub"]["launches"] in (0, iters)
    for cls in ("check", "check_col", "check_build"):
        assert ks[cls]["launches"] == checks, cls
    assert ks["harvest"]["launches"] == 5 and ks["harvest"]["units"] == 20
    assert ks["setup"]["launches"] == 5 and ks["setup"]["units"] == 4 + 16
    for cls, v in ks.items():
        assert (v["ms"] > 0) == (v["launches"] > 0), (cls, v)
    hp = eng.host_phases()
    print(hp)
    assert hp["check_total"]["count"] + hp["harvest_total"]["count"] == checks and hp["harvest_total"]["count"] == 5
    assert hp["check_wait"]["count"] == checks and hp["event_drain"]["count"] == checks - 1
    assert all(v["ms"] >= 0 for v in hp.values())
    inl = _run(eng, nodes, P, INLINE)
    _same(out, inl)
    ki = eng.kernel_stats()
    assert {c: (v["launches"], v["units"]) for c, v in ki.items()} == {c: (v["launches"], v["units"]) for c, v in ks.items()}


if __name__ == "__main__":      # child process of test_check_build_against_another_build: the same cases on the library OMC_AMD_LIB names
    sys.path.insert(0, os.path.dirname(HERE))
    import omc_amd
    A_, mask_ = _instance(omc_amd, 1)
    eng_ = omc_amd.Engine(A_, mask_, GAMMA, 1)
    Pe_ = omc_amd.default_params(rho_scale=4.0, max_iters=400)
    n2_, _ = omc_amd.pkg.bnb.expand_frontier(eng_, 2, "linear", params=Pe_)
    n6_, _ = omc_amd.pkg.bnb.expand_frontier(eng_, 6, "linear", params=Pe_)
    flat = {}
    real_run = _run

    def _run(eng, nodes, P, env, **kw):      # noqa: F811 -- the other build knows none of the new knobs: its only arm is the default
        return real_run(eng, nodes, P, {}, **kw)

    for name_, res_ in _check_cases(omc_amd, eng_, n2_, n6_).items():
        for i_, o_ in enumerate(res_):
            for s_ in SCALARS + ARRAYS:
                flat[f"{name_}/{i_}/{s_}"] = np.asarray(o_[s_])
    np.savez(sys.argv[1], **flat)
    eng_.close()
