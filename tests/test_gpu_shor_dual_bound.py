"""GPU tests of the device evaluator of Shor-mode certificates (omc_shor_dual_bound_batch / Engine.shor_dual_bound; run on the MI355X box:
`pytest -m gpu`).

The device is compared with numpy on the same multipliers: certificate.evaluate_shor for sanitise = 0, certificate.shor_dual_bound for
sanitise = 1.  Condition (the project's own, test_gpu_certificate.py): |device - numpy| <= 1e-7 max(1, |numpy|); -inf must match exactly.
Every input with a finite value must have numpy's min_j mu_j >= 1e-3 cT (asserted with the largest cT of the instance's column types, which
implies it per column), so that 1/mu cannot hide a disagreement behind amplification.  Set-ups are those of test_gpu_shor_certificate.py
(12 x 14 / 152 root and its cut nodes at the 1500 cap, 6 x 7 types 2 and 1, the six 10 x 12 nodes) and, for the L2-resident order class, a
synthetic 150 x 150 instance without a solve.  Measured differences: DESIGN.md section 3.12c."""
import math

import numpy as np
import pytest

from test_gpu_certificate import one_cut, synthetic
from test_gpu_shor_certificate import GAMMA, OBJ_REL, REPRO, _same_certificate, _shor, env10, env12, have_gpu, sh  # noqa: F401 (fixtures)
from test_shor_certificate_cpu import perturbed

pytestmark = pytest.mark.gpu
DEV_TOL = 1e-7
KEYS = ("objective", "dual_bound", "iters", "status_code")


def numpy_values(cert, A, mask, node, minors, c):
    """(evaluate_shor, its terms, shor_dual_bound, its defects) of one certificate."""
    n, m = A.shape
    st = cert.shor_structure(n, m, mask, minors, None)
    rows = cert.node_rows(n, 1, list(node), "linear")
    raw, terms = cert.evaluate_shor(A, mask, GAMMA, rows, st, c, want_terms=True)
    clean, df = cert.shor_dual_bound(A, mask, GAMMA, list(node), "linear", minors, None, c, want_defects=True)
    # the terms of the evaluation shor_dual_bound returned: the larger of its two
    cl, _ = cert.sanitise_shor(c, st)
    cands = [cert.evaluate_shor(A, mask, GAMMA, rows, st, cl, want_terms=True)]
    if st.nq:
        G = np.asarray(c.Gam, float).reshape(-1, 5, 5)
        cands.append(cert.evaluate_shor(A, mask, GAMMA, rows, st, cert.ShorCertificate(scale=cl.scale, lam=cl.lam, Q=cl.Q, Psi3=cl.Psi3,
                                                                                       Gam=0.5 * (G + np.transpose(G, (0, 2, 1))), zeta=cl.zeta,
                                                                                       xi=cl.xi, Xbar=cl.Xbar), want_terms=True))
    assert max(v for v, _ in cands) == clean
    cterms = max(cands, key=lambda t: t[0])[1]
    return raw, terms, clean, df, cterms, st


def compare(omc, eng, tag, A, mask, nodes, lists, certs, check_mu=True):
    """Device against numpy for every node of one call, both modes; prints every difference; returns (device raw, device sanitised, numpy
    sanitised, largest difference)."""
    cert = omc.pkg.certificate
    info = [(l, None) for l in lists]
    raw_d, df_d, t0 = eng.shor_dual_bound(nodes, info, certs, sanitise=False, want_defects=True, want_terms=True)
    cl_d, df_d1, t1 = eng.shor_dual_bound(nodes, info, certs, sanitise=True, want_defects=True, want_terms=True)
    worst = 0.0
    refs = []
    for b, c in enumerate(certs):
        raw, terms, clean, df, cterms, st = numpy_values(cert, A, mask, nodes[b], lists[b], c)
        refs.append(clean)
        cT = 1.0 / (2.0 * GAMMA) + (0.5 if (st.ctype == 1).any() else 0.0)
        for mode, dev, ref, tr, td in (("as given", raw_d[b], raw, terms, t0[b]), ("sanitised", cl_d[b], clean, cterms, t1[b])):
            if math.isinf(ref):
                print(f"{tag} node {b} {mode}: numpy {ref!r} device {dev!r}")
                assert dev == ref
                continue
            diff = abs(dev - ref)
            worst = max(worst, diff / max(1.0, abs(ref)))
            print(f"{tag} node {b} {mode}: numpy {ref!r} device {dev!r} difference {diff:.3e} cap {DEV_TOL * max(1.0, abs(ref)):.3e} "
                  f"min mu {tr[3]:.3e} (1e-3 cT = {1e-3 * cT:.3e}) terms numpy {tr} device {tuple(td)}")
            if check_mu:
                assert tr[3] >= 1e-3 * cT, (tag, b, mode, tr[3], cT)
            assert diff <= DEV_TOL * max(1.0, abs(ref)), (tag, b, mode, dev, ref)
            assert abs(td[3] - tr[3]) <= 1e-9 * cT
        gmax = float(np.abs(c.Gam).max()) if len(c.Gam) else 0.0
        pmax = float(np.abs(c.Psi3).max()) if np.size(c.Psi3) else 0.0
        for dd in (df_d[b], df_d1[b]):
            print(f"{tag} node {b} defects numpy {df} device {dd}")
            assert abs(dd["gam_min_eig"] - df["gam_min_eig"]) <= 1e-12 * gmax and abs(dd["v_residual"] - df["v_residual"]) <= 1e-12 * gmax
            assert dd["min_zeta"] == df["min_zeta"] and dd["min_lam"] == df["min_lam"]
            assert abs(dd["psi_min_eig"] - df["psi_min_eig"]) <= 1e-12 * max(pmax, gmax)
    print(f"{tag}: largest |device - numpy| / max(1, |numpy|) = {worst:.3e}")
    return raw_d, cl_d, refs, worst


@pytest.fixture(scope="module")
def eng12(env12, omc):
    eng = omc.Engine(env12.A, env12.mask, GAMMA, 1)
    yield eng
    eng.close()


# ---- 1. exported certificates ---------------------------------------------------------------------------------------------------------------------
def test_exported_certificates_12x14(env12, eng12, omc):
    e = env12
    nodes = [[], e.nodes[1], e.nodes[2]]
    outs = [e.root] + list(e.capped)
    certs = [e.root_cert] + list(e.capped_certs)
    raw_d, cl_d, refs, _ = compare(omc, eng12, "12x14/152", e.A, e.mask, nodes, [e.minors] * 3, certs)
    for b, o in enumerate(outs):
        sc = max(1.0, abs(o["objective"]))
        print(f"12x14/152 node {b}: reported dual_bound {o['dual_bound']!r} device sanitised {cl_d[b]!r} shortfall {o['dual_bound'] - cl_d[b]:.3e}")
        assert abs(o["dual_bound"] - cl_d[b]) <= REPRO * sc and abs(o["dual_bound"] - raw_d[b]) <= REPRO * sc


@pytest.mark.parametrize("ctype", [2, 1])
def test_exported_certificates_column_types(have_gpu, omc, orc, sh, ctype):
    """Fully observed 6 x 7: every class-4 minor (315: more than one 256-lane block, every column type 2) and the list thinned to rows 1-4
    (type 1)."""
    A, mask = orc.make_instance(6, 7, 1, n_indices=42, seed=7, noise=0.1)
    allm = orc.shor_constraints_indexes(mask, [4])
    minors = allm if ctype == 2 else [q for q in allm if q[1] <= 4]
    minors, _ = sh.driver_shor_lists(mask, minors=minors)
    assert (omc.pkg.certificate.shor_structure(6, 7, mask, minors, None).ctype == ctype).all() and (ctype == 1 or len(minors) == 315)
    eng = omc.Engine(A, mask, GAMMA, 1)
    try:
        eng.keep_shor_certificates(True)
        r = _shor(eng, [[]], [(minors, None)], omc.default_params(eps_gap=1e-6, max_iters=8000))[0]
        c = eng.fetch_shor_certificate([0])[0]
        raw_d, cl_d, _, _ = compare(omc, eng, f"6x7/{len(minors)} type {ctype}", A, mask, [[]], [minors], [c])
        assert abs(r["dual_bound"] - cl_d[0]) <= REPRO * max(1.0, abs(r["objective"]))
    finally:
        eng.close()


def test_exported_certificates_10x12(env10, omc):
    e = env10
    raw_d, cl_d, _, _ = compare(omc, e.eng, "10x12", e.A, e.mask, e.nodes, e.lists, e.certs)
    for b in range(6):
        assert abs(e.ref[b]["dual_bound"] - cl_d[b]) <= REPRO * max(1.0, abs(e.ref[b]["objective"]))


# ---- 2. one batch, several lists: a node's result does not depend on the batch around it ----------------------------------------------------------
def test_batch_composition_does_not_matter(env10, omc):
    e = env10
    for sanitise in (False, True):
        full = e.eng.shor_dual_bound(e.nodes, e.info, e.certs, sanitise=sanitise, nq_stride=208)
        assert np.isfinite(full).all()
        alone = np.array([e.eng.shor_dual_bound([e.nodes[b]], [e.info[b]], [e.certs[b]], sanitise=sanitise)[0] for b in range(6)])
        rev = e.eng.shor_dual_bound(e.nodes[::-1], e.info[::-1], e.certs[::-1], sanitise=sanitise)[::-1]
        wide = e.eng.shor_dual_bound(e.nodes, e.info, e.certs, sanitise=sanitise, nq_stride=300)
        for other in (alone, rev, wide):
            assert np.array_equal(full, other), (sanitise, full, other)


# ---- 3. perturbed and inadmissible input ----------------------------------------------------------------------------------------------------------
def inadmissible(cert, c, rng, noise=0.05):
    """The trial of test_inadmissible_multipliers_are_sanitised_and_reported: indefinite blocks whose V entries do not cancel, negative zeta,
    lam and Psi3.  At its noise of 0.05 the diagonals push zeta past cT and numpy returns -inf in both modes (the device must too); the
    `mild` recipe is the same trial at a hundredth of that, where the values are finite (chosen on the CPU: min mu about 3.6e-3)."""
    scale_g = np.abs(c.Gam).max()
    Gam = c.Gam + noise * scale_g * rng.standard_normal(c.Gam.shape)
    zeta = c.zeta - 0.5 * np.abs(c.zeta).max() * rng.random(len(c.zeta)) - 1e-3
    lam = c.lam - 0.1 * rng.random(len(c.lam))
    Psi = c.Psi3 + 0.1 * max(np.abs(c.Psi3).max(), 1e-3) * (rng.standard_normal(c.Psi3.shape) - 2.0 * np.eye(len(c.Psi3)))
    return cert.ShorCertificate(scale=c.scale, lam=lam, Q=c.Q, Psi3=Psi, Gam=Gam, zeta=zeta, xi=c.xi, Xbar=c.Xbar)


@pytest.mark.parametrize("recipe", ["perturbed", "inadmissible", "mild"])
def test_perturbed_and_inadmissible_input(env12, eng12, omc, recipe):
    """Five seeds each on the 12 x 14 root.  The as-given evaluation of the inadmissible trial takes negative zeta, lam and an indefinite Psi3
    as they are (it is a number, not a bound); the sanitised value is a bound and stays below the oracle's certified optimum."""
    e = env12
    cert = omc.pkg.certificate
    certs = []
    for seed in range(5):
        rng = np.random.default_rng(100 + seed)
        certs.append(perturbed(cert, e.root_cert, rng) if recipe == "perturbed" else inadmissible(cert, e.root_cert, rng, 0.05 if recipe == "inadmissible" else 5e-4))
    _, cl_d, refs, _ = compare(omc, eng12, recipe, e.A, e.mask, [[]] * 5, [e.minors] * 5, certs)
    obj = float(e.ro["objective"])
    for v in cl_d:
        assert v <= obj + OBJ_REL * max(1.0, abs(obj))


# ---- 4. the -inf paths ------------------------------------------------------------------------------------------------------------------------------
def test_minus_infinity_paths(env12, eng12, omc):
    e = env12
    cert = omc.pkg.certificate
    c = e.root_cert
    rep = lambda **kw: cert.ShorCertificate(**{**{f: getattr(c, f) for f in ("scale", "lam", "Q", "Psi3", "Gam", "zeta", "xi", "Xbar")}, **kw})
    good = {s: eng12.shor_dual_bound([[]], [(e.minors, None)], [c], sanitise=s)[0] for s in (False, True)}
    assert np.isfinite(good[False]) and np.isfinite(good[True])
    info5 = [(e.minors, None)] * 5
    # a scale that is not positive and finite
    bad = [rep(scale=s) for s in (0.0, -1.0, math.inf, math.nan)]
    for s in (False, True):
        out = eng12.shor_dual_bound([[]] * 5, info5, bad[:2] + [c] + bad[2:], sanitise=s)
        assert list(out[[0, 1, 3, 4]]) == [-math.inf] * 4 and out[2] == good[s]
        assert all(cert.shor_dual_bound(e.A, e.mask, GAMMA, [], "linear", e.minors, None, b) == -math.inf for b in bad)
    # zeta of one type-0 column at twice cT: mu < 0 meets a nonzero phi
    st = cert.shor_structure(12, 14, e.mask, e.minors, None)
    j = int(np.flatnonzero(st.ctype == 0)[0])
    zeta = c.zeta.copy(); zeta[j] = 2.0 * (1.0 / (2.0 * GAMMA))
    cz = rep(zeta=zeta)
    rows = cert.node_rows(12, 1, [], "linear")
    assert cert.evaluate_shor(e.A, e.mask, GAMMA, rows, st, cz) == -math.inf
    out = eng12.shor_dual_bound([[], []], info5[:2], [cz, c], sanitise=False)
    assert out[0] == -math.inf and out[1] == good[False]
    # a NaN in one block: that node is -inf in both modes, its neighbours keep their values bit for bit
    Gam = c.Gam.copy(); Gam[77, 2, 3] = Gam[77, 3, 2] = math.nan
    cn = rep(Gam=Gam)
    assert cert.evaluate_shor(e.A, e.mask, GAMMA, rows, st, cn) == -math.inf
    for s in (False, True):
        out, terms = eng12.shor_dual_bound([[]] * 3, info5[:3], [c, cn, c], sanitise=s, want_terms=True)
        assert out[1] == -math.inf and out[0] == good[s] and out[2] == good[s], (s, out)
    Gam = c.Gam.copy(); Gam[5, 0, 1] = Gam[5, 1, 0] = math.inf
    assert eng12.shor_dual_bound([[]], info5[:1], [rep(Gam=Gam)], sanitise=False)[0] == -math.inf


# ---- 5. the empty list ------------------------------------------------------------------------------------------------------------------------------
def test_empty_list(env10, omc):
    e = env10
    cert = omc.pkg.certificate
    certs = []
    for b in (0, 1):
        c = e.certs[b]
        certs.append(cert.ShorCertificate(scale=c.scale, lam=c.lam, Q=c.Q, Psi3=c.Psi3, Gam=np.zeros((0, 5, 5)), zeta=c.zeta, xi=c.xi, Xbar=c.Xbar))
    compare(omc, e.eng, "10x12 empty list", e.A, e.mask, e.nodes[:2], [[], []], certs)


# ---- 6. the L2-resident order class, no solve -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncuts", [0, 1])
def test_order_150_random_multipliers(have_gpu, omc, ncuts):
    """Synthetic 150 x 150 (n is no multiple of 16), 400 class-4 minors, the multipliers of test_random_multipliers_smoke: the dense MFMA
    product and the L2-resident eigen-kernel."""
    n = m = 150
    A, mask = synthetic(n, m, 0.2, 3)
    cert = omc.pkg.certificate
    eng = omc.Engine(A, mask, GAMMA, 1)
    try:
        allm = np.asarray(eng.generate_rank1_matrix_completion_Shor_constraints_indexes([4]), np.int64).reshape(-1, 4)
        assert len(allm) >= 400
        minors = [tuple(int(v) for v in q) for q in allm[:: len(allm) // 400][:400]]
        rng = np.random.default_rng(40 + ncuts)
        node = one_cut(rng, n, 1, "linear") if ncuts else []
        Q = eng.row_basis([node])[0]
        R = len(cert.node_rows(n, 1, node, "linear"))
        G = rng.standard_normal((400, 5, 5))
        Gam = G @ np.transpose(G, (0, 2, 1))
        Gam *= 0.02 / np.abs(Gam).max()
        c = cert.ShorCertificate(scale=1.3, lam=np.abs(rng.standard_normal(R)) * 0.1, Q=Q, Psi3=np.zeros((Q.shape[1] + 1,) * 2), Gam=Gam,
                                 zeta=rng.random(m) * 0.005, xi=rng.standard_normal((n, m)) * 0.1, Xbar=rng.standard_normal((n, m)) * 0.1)
        compare(omc, eng, f"150x150/400 cuts {ncuts}", A, mask, [node], [minors], [c])
    finally:
        eng.close()


# ---- 7. isolation -------------------------------------------------------------------------------------------------------------------------------------
def test_a_staged_batch_is_left_alone(env12, env10, omc):
    e = env12
    eng = omc.Engine(e.A, e.mask, GAMMA, 1)
    try:
        eng.keep_shor_certificates(True)
        eng.stage_shor([[]], [(e.minors, None)], "linear", e.P_root)
        other = perturbed(omc.pkg.certificate, e.capped_certs[0], np.random.default_rng(7))
        # other multipliers, another node, a shorter list (the value itself is whatever numpy says of them; -inf is allowed)
        dev = eng.shor_dual_bound([e.nodes[1]], [(e.minors[:100], None)], [other_with(other, 100)])[0]
        ref = omc.pkg.certificate.shor_dual_bound(e.A, e.mask, GAMMA, e.nodes[1], "linear", e.minors[:100], None, other_with(other, 100))
        assert dev == ref if math.isinf(ref) else abs(dev - ref) <= DEV_TOL * max(1.0, abs(ref))
        assert np.isfinite(eng.shor_dual_bound([[]], [(e.minors, None)], [perturbed(omc.pkg.certificate, e.root_cert, np.random.default_rng(8))])[0])
        eng.solve()
        out = eng.fetch(want_Theta=True)[0]
        W = eng.fetch_shor()[0]
        c = eng.fetch_shor_certificate([0])[0]
        assert all(out[key] == e.root[key] for key in KEYS)
        assert np.array_equal(out["X"], e.root["X"]) and np.array_equal(W, e.root["W"]) and np.array_equal(out["Theta"], e.root["Theta"])
        assert _same_certificate(c, e.root_cert)
        # after a finished solve: the fetchable certificate is the same before and after an evaluator call
        eng.shor_dual_bound([[]] * 2, [(e.minors, None)] * 2, [c, e.root_cert])
        assert _same_certificate(eng.fetch_shor_certificate([0])[0], c)
        assert all(eng.fetch()[0][key] == e.root[key] for key in KEYS)
        # refused while a held submitted solve runs, works after wait()
        eng.stage_shor([[]], [(e.minors, None)], "linear", e.P_root)
        eng.hold(True)
        eng.submit()
        with pytest.raises(omc.OmcError) as err:
            eng.shor_dual_bound([[]], [(e.minors, None)], [c])
        assert err.value.code == -3 and "in flight" in str(err.value)
        eng.hold(False)
        eng.wait()
        assert np.isfinite(eng.shor_dual_bound([[]], [(e.minors, None)], [c])[0])
    finally:
        eng.close()


def other_with(c, nq):
    """The certificate with its first nq blocks only (a shorter list than the staged one)."""
    return type(c)(scale=c.scale, lam=c.lam, Q=c.Q, Psi3=c.Psi3, Gam=c.Gam[:nq], zeta=c.zeta, xi=c.xi, Xbar=c.Xbar)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(env12, eng12, omc, orc):
    e = env12
    c = e.root_cert
    info = [(e.minors, None)]
    with pytest.raises(omc.OmcError) as err:
        eng12.shor_dual_bound([[]], info, [c], nq_stride=100)
    assert err.value.code == -3 and "nq_stride" in str(err.value)
    dup = list(e.minors); dup[3] = dup[2]
    with pytest.raises(omc.OmcError) as err:
        eng12.shor_dual_bound([[]], [(dup, None)], [c])
    assert err.value.code == -3 and "duplicate" in str(err.value)
    out_of_range = list(e.minors); out_of_range[0] = (1, 13, 1, 2)
    with pytest.raises(omc.OmcError) as err:
        eng12.shor_dual_bound([[]], [(out_of_range, None)], [c])
    assert err.value.code == -3 and "Shor minors must satisfy" in str(err.value)
    # the same errors omc_relax_stage_shor gives
    for bad in (dup, out_of_range):
        with pytest.raises(omc.OmcError) as err2:
            eng12.stage_shor([[]], [(bad, None)], "linear")
        assert err2.value.code == -3
    # rank 2: no Shor-mode certificate exists
    A2, mask2 = orc.make_instance(12, 14, 2, n_indices=90, seed=3, noise=0.1)
    eng2 = omc.Engine(A2, mask2, GAMMA, 2)
    try:
        cert = omc.pkg.certificate
        Q2 = eng2.row_basis([[]])[0]
        R2 = len(cert.node_rows(12, 2, [], "linear"))
        c2 = cert.ShorCertificate(scale=1.0, lam=np.zeros(R2), Q=Q2, Psi3=np.zeros((Q2.shape[1] + 2,) * 2), Gam=np.zeros((0, 5, 5)), zeta=np.zeros(14),
                                  xi=np.zeros((12, 14)), Xbar=np.zeros((12, 14)))
        with pytest.raises(omc.OmcError) as err:
            eng2.shor_dual_bound([[]], [([], None)], [c2])
        assert err.value.code == -4
    finally:
        eng2.close()
