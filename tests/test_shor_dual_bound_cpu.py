"""CPU tests of the device evaluator of Shor-mode certificates (omc_shor_dual_bound_batch): what can be checked without a GPU -- the symbols,
the memory plan against the formula documented in include/omc.h, the refusals that are decided before any device call, and the four terms
certificate.evaluate_shor reports on request."""
import ctypes as C

import numpy as np
import pytest

GAMMA = 80.0


def plan_formula(n, m, B, nqs, max_cuts, box_rows, sanitise, slab):
    """The comment of omc_shor_dual_bound_plan, restated."""
    nmb = -(-nqs // 256)
    NP = (n + 15) // 16 * 16
    nn4 = (n * n + 3) // 4 * 4
    Rmax = 2 + box_rows + 3 * max_cuts
    rmax = max(1, min(n, 1 + box_rows + max_cuts))
    Lmax = max(max_cuts, 1)
    ps = (rmax + 1) ** 2
    node = 8 * (1 + 15 * nqs + m + 2 * n * m) + 8 * ((15 * nqs if sanitise else 0) + nmb) + 4 + 4 * (20 * nqs + n * m + m + 3) \
        + ((n * m + m + 15) & ~15) + 120
    view = 8 * (12 * nqs + 2 * nmb + n * m + 2 * m) + 4 * m + 8 + 8 * (2 * NP * NP + nn4 + slab) + 8 * (2 * Rmax + Lmax * n + n * rmax) \
        + 8 * (Rmax + ps + n * rmax + n + 5) + 4 * (4 * Rmax + 9)
    ways = 2 if sanitise else 1
    return dict(bytes_per_node=node + ways * view, bytes_total=B * (node + ways * view), node_bytes=node, view_bytes=view, ways=ways,
                slab_doubles=slab, Rmax=Rmax, rmax=rmax)


def test_symbols_exist(omc):
    lib = omc.load()
    for name in ("omc_shor_dual_bound_batch", "omc_shor_dual_bound_plan"):
        assert name in omc.EXPORTS
        getattr(lib, name)
    assert hasattr(omc.Engine, "shor_dual_bound") and hasattr(omc.pkg.api, "shor_dual_bound_plan")


@pytest.mark.parametrize("shape", [(12, 14, 3, 152, 2, 0, True), (200, 200, 1, 632732, 0, 5, False)])
def test_plan_matches_the_documented_formula(omc, shape):
    n, m, B, nqs, cuts, box, sanitise = shape
    got = omc.pkg.api.shor_dual_bound_plan(n, m, 1, B, nqs, max_cuts=cuts, nonstandard_box_rows=box, sanitise=sanitise)
    assert got == plan_formula(n, m, B, nqs, cuts, box, sanitise, got["slab_doubles"])
    # the slab is that of the eigen-kernel at order n: none where it works in LDS, more than the matrix where it does not
    assert (got["slab_doubles"] == 0) if n == 12 else (got["slab_doubles"] >= n * n)


def test_plan_refusals(omc):
    lib = omc.load()
    out = np.zeros(8, np.int64)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.omc_shor_dual_bound_plan(12, 14, 2, 1, 152, 0, 0, 1, p) == -4
    assert lib.omc_shor_dual_bound_plan(0, 14, 1, 1, 152, 0, 0, 1, p) == -3
    assert lib.omc_shor_dual_bound_plan(12, 14, 1, 1, 152, 0, 0, 1, None) == -3
    assert lib.omc_shor_dual_bound_plan(12, 14, 1, 1, 1 << 28, 0, 0, 1, p) == -4


def test_null_handle_is_refused_without_a_device(omc):
    lib = omc.load()
    assert lib.omc_shor_dual_bound_batch(None, 1, 0, 1, *([None] * 10), 1, 0, *([None] * 10)) == -3
    assert b"handle is NULL" in lib.omc_last_error()
    ms = np.zeros(1)
    assert lib.omc_last_shor_dual_bound_ms(None, ms.ctypes.data_as(C.c_void_p)) == -3


def test_evaluate_shor_reports_its_terms(omc, orc):
    """want_terms=True returns the old value first, and constant + min(eig_0, 0) - ||c|| is value * scale^2; the default return is unchanged."""
    import omc_oracle_shor as sh
    cert = omc.pkg.certificate
    A, mask = orc.make_instance(12, 14, 1, n_indices=70, seed=2, noise=0.1)
    minors, _ = sh.driver_shor_lists(mask, (4,))
    st = cert.shor_structure(12, 14, mask, minors, None)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(12); x /= np.linalg.norm(x)
    U = rng.standard_normal((12, 1)); U /= np.linalg.norm(U)
    for node in ([], [(x, U, ["left"])]):
        rows = cert.node_rows(12, 1, node, "linear")
        Q = cert.row_basis(rows, 12, 1)
        r = Q.shape[1]
        for trial in range(5):
            G = rng.standard_normal((len(minors), 5, 5))
            Gam = G @ np.transpose(G, (0, 2, 1))
            Gam *= 0.02 / np.abs(Gam).max()
            H = rng.standard_normal((r + 1, r + 1)) * 0.05
            c = cert.ShorCertificate(scale=0.7 + 0.1 * trial, lam=np.abs(rng.standard_normal(len(rows))) * 0.1, Q=Q, Psi3=H @ H.T, Gam=Gam,
                                     zeta=rng.random(14) * 0.005, xi=rng.standard_normal((12, 14)) * 0.1, Xbar=rng.standard_normal((12, 14)) * 0.1)
            plain = cert.evaluate_shor(A, mask, GAMMA, rows, st, c)
            val, terms = cert.evaluate_shor(A, mask, GAMMA, rows, st, c, want_terms=True)
            assert val == plain and np.isfinite(val) and len(terms) == 4
            assert terms[1] <= 0.0 and terms[2] >= 0.0 and 0.0 < terms[3] <= 1.0 / (2.0 * GAMMA) + 0.5
            assert abs((terms[0] + terms[1] - terms[2]) - val * c.scale ** 2) <= 1e-15 * abs(val * c.scale ** 2)
    # a -inf on the way: the value is -inf and the terms that were not reached are nan
    bad = cert.ShorCertificate(scale=-1.0, lam=c.lam, Q=c.Q, Psi3=c.Psi3, Gam=c.Gam, zeta=c.zeta, xi=c.xi, Xbar=c.Xbar)
    val, terms = cert.evaluate_shor(A, mask, GAMMA, rows, st, bad, want_terms=True)
    assert val == -np.inf and all(np.isnan(t) for t in terms)
