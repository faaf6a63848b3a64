"""Multi-workgroup eigen-kernels (csrc/omc_cone_mw.hip) and omc_psd_project_batch: the spectral clip on its own against numpy.linalg.eigh,
warm starts, dispatch by the knob OMC_CONE_MULTI_MIN, and the solver through the new path against its default path and the oracles.

Bounds.  Projection, eigenvalues: 1e-8 ||M||_F; orthogonality of V: 1e-8 -- 100 x the 1e-10 rotation threshold of the kernels, for the
accumulation over the pairs (the numpy prototype of the scheme sits at 1e-10 with the 1e-7 stop rule and fails with 1e-5).  Solver
comparisons: the project's own OBJ_REL = 2e-6 on objectives, 1e-5 on dual bounds at a common iteration cap, equal iteration counts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GAMMA = 80.0
OBJ_REL = 2e-6
TOL = 1e-8


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


@pytest.fixture(scope="module")
def eng(have_gpu, omc):
    """psd_project does not depend on the instance's n and m: any small instance carries it"""
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, 8, 10, 40, seed=1)
    e = omc.Engine(A, mask, GAMMA, 1)
    yield e
    e.close()


def _gauss(N, rng):
    G = rng.standard_normal((N, N))
    return (G + G.T) / (2.0 * np.sqrt(N))


def _shor_like(N, rng):
    """spectrum of the big cone of a Shor root: 67.9, 0.038 and the rest geometric from -7e-4 to -8.5, random orthogonal basis"""
    lam = np.concatenate([[67.9, 0.038], -np.geomspace(7e-4, 8.5, N - 2)])
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    return (Q * lam) @ Q.T


def _lowrank(N, rng):
    L = rng.standard_normal((N, 3))
    return L @ L.T - 0.1 * np.eye(N)


CASES = [("gauss", _gauss, 0.0, 1.0), ("shor", _shor_like, 0.0, np.inf), ("lowrank", _lowrank, 0.0, np.inf), ("zero", lambda N, rng: np.zeros((N, N)), 0.0, 1.0)]


def _reference(M, lo, hi):
    M = 0.5 * (M + M.T)
    w, V = np.linalg.eigh(M)
    return (V * np.clip(w, lo, hi)) @ V.T, w


def _check(M, lo, hi, P, ev, V, tag):
    Pr, wr = _reference(M, lo, hi)
    nrm = np.linalg.norm(M)
    e_p = np.linalg.norm(P - Pr); e_w = np.abs(ev - wr).max(); e_v = np.abs(V.T @ V - np.eye(M.shape[0])).max()
    print(f"{tag}: |P-Pref|_F={e_p:.3e} max|ev-evref|={e_w:.3e} (|M|_F={nrm:.3e}) max|V'V-I|={e_v:.3e}")
    assert np.isfinite(P).all() and np.isfinite(ev).all() and np.isfinite(V).all(), tag
    assert e_p <= TOL * nrm, (tag, e_p, nrm)
    assert e_w <= TOL * nrm, (tag, e_w, nrm)
    assert e_v <= TOL, (tag, e_v)
    assert np.array_equal(P, P.T), tag


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [130, 400, 1000, 1001, 1040, 2000])
def test_projection_multi_workgroup_against_eigh(eng, N, B):
    """T1: algo = 2 at every order, one and three different matrices per call, the four matrix families."""
    for ci, (name, make, lo, hi) in enumerate(CASES):
        rng = np.random.default_rng(1000 * ci + N + B)
        M = np.stack([make(N, rng) for _ in range(B)])
        P, ev, V = eng.psd_project(M, lo=lo, hi=hi, algo=2, want_evals=True, want_V=True)
        st = eng.cone_multi_stats()
        print(f"N={N} B={B} {name}: sweeps={st['last_sweeps']} exhausted={st['exhausted']}")
        assert st["exhausted"] == 0, st
        for b in range(B):
            _check(M[b], lo, hi, P[b], ev[b], V[b], f"N={N} B={B} {name}[{b}]")
        if name == "zero":
            assert not P.any()


@pytest.mark.parametrize("N", [400, 1040])
def test_warm_start_needs_fewer_sweeps(eng, N):
    """T2: the V of a call on M as V0 for M + eps ||M|| E / ||E||: same bounds, fewer sweeps than the cold call on the same matrix, and no
    call uses up its sweep budget."""
    rng = np.random.default_rng(7 + N)
    M = _shor_like(N, rng)
    _, _, V = eng.psd_project(M, algo=2, want_evals=True, want_V=True)
    assert eng.cone_multi_stats()["exhausted"] == 0
    for eps in (1e-3, 1e-5):
        E = _gauss(N, rng)
        M2 = M + eps * np.linalg.norm(M) * E / np.linalg.norm(E)
        Pc, evc, Vc = eng.psd_project(M2, algo=2, want_evals=True, want_V=True)
        cold = eng.cone_multi_stats()
        Pw, evw, Vw = eng.psd_project(M2, algo=2, V0=V, want_evals=True, want_V=True)
        warm = eng.cone_multi_stats()
        print(f"N={N} eps={eps:g}: cold sweeps={cold['last_sweeps']} warm sweeps={warm['last_sweeps']}")
        _check(M2, 0.0, np.inf, Pc, evc, Vc, f"N={N} eps={eps:g} cold")
        _check(M2, 0.0, np.inf, Pw, evw, Vw, f"N={N} eps={eps:g} warm")
        assert cold["exhausted"] == 0 and warm["exhausted"] == 0
        assert warm["last_sweeps"] < cold["last_sweeps"], (cold, warm)


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_dispatch_and_determinism(eng):
    """T3: algo = 0 is the single-workgroup path up to order 1024 and the multi-workgroup path above at the default knob; with the knob
    at 145 order 400 moves to the new path and order 130 (below 145) does not; two runs are bit-identical."""
    rng = np.random.default_rng(3)
    # orders 129 .. 144 have no k_cone_ws (more than 32 rows per lane): a relaxation runs the cold k_cone there, which returns P only
    run = lambda M, algo: eng.psd_project(M, lo=0.0, hi=1.0, algo=algo, want_V=M.shape[0] != 130)
    mats = {N: _gauss(N, rng) for N in (130, 400, 1000, 1040)}
    for N in (130, 400, 1000):
        assert _same(run(mats[N], 0), run(mats[N], 1)), N
    a2 = run(mats[1040], 2)
    assert _same(run(mats[1040], 0), a2)
    assert _same(run(mats[1040], 2), a2)
    b2 = run(mats[400], 2)
    assert _same(run(mats[400], 2), b2)
    assert not _same(b2, run(mats[400], 1))          # the two paths are different arithmetic
    eng.tuning_set("OMC_CONE_MULTI_MIN", "145")
    try:
        assert _same(run(mats[400], 0), b2)
        assert _same(run(mats[130], 0), run(mats[130], 1))
    finally:
        eng.tuning_set("OMC_CONE_MULTI_MIN", None)


def test_cold_single_workgroup_kernel_against_eigh(eng, N=130):
    """algo = 1 where k_cone_ws does not exist (orders 129 - 144; above 1024 it is the same kernel, seconds per call): the cold kernel
    k_cone through a zeroed workspace view, which returns P only.  Same bound on P as T1 (the kernel rotates to the same 1e-10)."""
    for ci, (name, make, lo, hi) in enumerate(CASES):
        M = make(N, np.random.default_rng(50 * ci + N))
        P = eng.psd_project(M, lo=lo, hi=hi, algo=1)
        Pr, _ = _reference(M, lo, hi)
        e_p, nrm = np.linalg.norm(P - Pr), np.linalg.norm(M)
        print(f"N={N} {name} algo=1: |P-Pref|_F={e_p:.3e} (|M|_F={nrm:.3e})")
        assert np.isfinite(P).all() and e_p <= TOL * nrm, (name, e_p, nrm)
        assert np.array_equal(P, P.T), name


def test_knob_is_typed_and_unknown_names_are_refused(eng):
    """OMC_CONE_MULTI_MIN goes through omc_tuning_set like every knob; a misspelt name is an error, not a silent no-op"""
    rng = np.random.default_rng(11)
    M2, M4 = _gauss(200, rng), _gauss(400, rng)
    eng.tuning_set("OMC_CONE_MULTI_MIN", "300")
    try:
        assert np.array_equal(eng.psd_project(M4, hi=1.0, algo=0), eng.psd_project(M4, hi=1.0, algo=2))
        assert np.array_equal(eng.psd_project(M2, hi=1.0, algo=0), eng.psd_project(M2, hi=1.0, algo=1))
    finally:
        eng.tuning_set("OMC_CONE_MULTI_MIN", None)
    assert np.array_equal(eng.psd_project(M4, hi=1.0, algo=0), eng.psd_project(M4, hi=1.0, algo=1))      # back at the default
    with pytest.raises(Exception):
        eng.tuning_set("OMC_CONE_MULTI_MINIMUM", "145")


def _knob_run(e, nodes, P, knob, **kw):
    if knob is not None:
        e.tuning_set("OMC_CONE_MULTI_MIN", knob)
    try:
        return e.matrix_completion_SDP_relaxation(nodes, "linear", params=P, **kw)[0]
    finally:
        e.tuning_set("OMC_CONE_MULTI_MIN", None)


def _thin(minors, target, seed):
    rng = np.random.default_rng(seed)
    return [q for q in minors if rng.random() < target / max(len(minors), 1)]


def _compare(a, b, tag):
    print(f"{tag}: iters {a['iters']} / {b['iters']}  objective {a['objective']!r} / {b['objective']!r}  dual bound {a['dual_bound']!r} / {b['dual_bound']!r}")
    assert a["iters"] == b["iters"], tag
    assert a["objective"] == pytest.approx(b["objective"], rel=OBJ_REL), tag
    assert a["dual_bound"] == pytest.approx(b["dual_bound"], rel=1e-5), tag


def test_shor_root_with_the_knob_lowered(have_gpu, omc, orc, sh):
    """T4a: Shor root 100 x 120, rank 1, ~2000 thinned class-4 minors (big cone of order 220): knob at 145 against the default path."""
    A, mask = orc.make_instance(100, 120, 1, n_indices=int(0.2 * 100 * 120), seed=0, noise=0.05)
    minors = _thin(orc.shor_constraints_indexes(mask, [4]), 2000, 1)
    minors, soc = sh.driver_shor_lists(mask, minors=minors)
    print("minors", len(minors))
    e = omc.Engine(A, mask, GAMMA, 1)
    P = omc.default_params(eps_gap=1e-12, max_iters=400)
    kw = dict(add_Shor_valid_inequalities=True, shor_info=[(minors, None)])
    d = _knob_run(e, [[]], P, None, **kw)
    assert e.cone_multi_stats()["calls"] == 0
    k = _knob_run(e, [[]], P, "145", **kw)
    st = e.cone_multi_stats()
    print("multi-workgroup stats", st)
    assert st["calls"] > 0 and st["exhausted"] == 0, st
    _compare(k, d, "shor root 100x120")
    e.close()


def test_config5_node_with_the_knob_lowered(have_gpu, omc, orc):
    """T4b: the node of test_config5_node_evaluation (cone order 1000), 100 iterations: knob at 145 against the default path, and the
    tracked block is seeded by the new select kernel and then used."""
    A, mask, gamma, c = omc.pkg.data.config_instance(5, seed=0)
    e = omc.Engine(A, mask, gamma, 2)
    P = omc.default_params(rho_scale=4.0, max_iters=100, check_every=25)
    d = _knob_run(e, [[]], P, None)
    k = _knob_run(e, [[]], P, "145")
    st, mw = e.subspace_stats(), e.cone_multi_stats()
    print("subspace", st, "multi-workgroup", mw)
    assert mw["calls"] > 0 and mw["exhausted"] == 0, mw
    assert st["calls"] >= 20 and st["fallbacks"] <= 5, st
    _compare(k, d, "config 5 node")
    e.close()


def test_base_mode_above_order_1024_against_the_oracle(have_gpu, omc, orc):
    """T5: 1040 x 1100, rank 1, 5 % observed: the cone block of order 1040 runs on the multi-workgroup kernels at the default knob."""
    A, mask = orc.make_instance(1040, 1100, 1, n_indices=int(0.05 * 1040 * 1100), seed=0, noise=0.01)
    e = omc.Engine(A, mask, GAMMA, 1)
    g = e.matrix_completion_SDP_relaxation([[]], "linear", params=omc.default_params(rho_scale=4.0, eps_gap=1e-12, max_iters=50))[0]
    mw = e.cone_multi_stats()
    print("multi-workgroup", mw)
    assert mw["calls"] > 0 and mw["exhausted"] == 0, mw
    r = orc.sdp_relaxation(orc.Instance(A, mask, GAMMA, 1), [], "linear", params=orc.RelaxParams(rho_scale=4.0, eps_gap=1e-12, max_iters=50), want_certificate=False)
    print(f"iters {g['iters']} / {r['iters']}  objective {g['objective']!r} / {r['objective']!r}")
    assert g["iters"] == r["iters"]
    assert g["objective"] == pytest.approx(r["objective"], rel=OBJ_REL)
    e.close()


def test_shor_mode_above_order_1024_against_the_oracle(have_gpu, omc, orc, sh):
    """T6: 500 x 560 Shor root, class-4 minors of the first 40 rows thinned to ~2000: the big cone of order 1060 on the new kernels."""
    A, mask = orc.make_instance(500, 560, 1, n_indices=int(0.1 * 500 * 560), seed=0, noise=0.05)
    top = mask.copy(); top[40:, :] = False
    allm = orc.shor_constraints_indexes(top, [4])
    assert len(allm) == 13302
    rng = np.random.default_rng(1)
    minors = [q for q in allm if rng.random() < 2000 / len(allm)]
    minors, soc = sh.driver_shor_lists(mask, minors=minors)
    e = omc.Engine(A, mask, GAMMA, 1)
    g = e.matrix_completion_SDP_relaxation([[]], "linear", omc.default_params(eps_gap=1e-12, max_iters=100), add_Shor_valid_inequalities=True,
                                           shor_info=[(minors, None)])[0]
    mw = e.cone_multi_stats()
    print("multi-workgroup", mw)
    assert mw["calls"] > 0 and mw["exhausted"] == 0, mw
    r = sh.sdp_relaxation_shor(orc.Instance(A, mask, GAMMA, 1), minors, soc, params=sh.ShorParams(eps_gap=1e-12, max_iters=100))
    print(f"iters {g['iters']} / {r['iters']}  objective {g['objective']!r} / {r['objective']!r}")
    assert g["iters"] == r["iters"]
    assert g["objective"] == pytest.approx(r["objective"], rel=OBJ_REL)
    e.close()
