"""CPU tests of the certificate checker (optimalmatrixcompletion.jl_amd/certificate.py) and of the host-only plan: no GPU.

The checker restates the rows and the bound on its own; here it is held against the oracle's dual_bound_from on admissible multipliers
(same arithmetic in another order: rtol 1e-12, the project's tolerance for plain scans), its sanitising against hand-sanitised inputs, and
the validity of what it returns against the oracle's certified optimum (2e-6 relative, the project's stated tolerance)."""
import ctypes as C

import numpy as np
import pytest

GAMMA = 80.0
OBJ_REL = 2e-6


def path_of(orc, inst, cut_type, depth, seed=3):
    """A root-to-depth path of cuts on the oracle's own separation vectors (the recipe of the GPU parity tests)."""
    rng = np.random.default_rng(seed)
    dirs = orc.child_directions(cut_type, inst.k)
    cuts = []
    for _ in range(depth):
        r = orc.sdp_relaxation(inst, cuts, cut_type, params=orc.RelaxParams(rho_scale=8.0, max_iters=100), want_certificate=False)      # the cuts need not come from a converged parent
        x, _ = orc.breakpoint_vector(r["Y"], r["U"], "smallest_1_eigvec")
        vhat = r["U"].T @ x
        ok = [d for d in dirs if all((abs(vhat[j]) > 0.05) or (d[j] in ("left", "right")) for j in range(inst.k))]
        cuts = cuts + [(x, r["U"].copy(), ok[int(rng.integers(len(ok)))])]
    return cuts


def random_admissible(cert_mod, rng, inst, rows_len, Q):
    """Lam on Omega, lam >= 0, Psi3 = G G'."""
    r, k = Q.shape[1], inst.k
    Lam = np.where(inst.indices, rng.standard_normal(inst.A.shape) * 0.3, 0.0)
    lam = np.abs(rng.standard_normal(rows_len)) * (rng.random(rows_len) < 0.6)
    G = rng.standard_normal((r + k, r + k)) * 0.2
    return cert_mod.Certificate(Lam=Lam, lam=lam, Q=Q, Psi3=G @ G.T)


CASES = [
    (12, 15, 1, "readme", "linear", 2, False),
    (16, 20, 2, "lowrank", "linear3", 2, False),
    (12, 15, 2, "lowrank", "linear2", 1, True),       # non-default U bounds
]


@pytest.fixture(scope="module")
def cases(orc):
    out = []
    for (n, m, k, kind, cut_type, depth, custom) in CASES:
        A, mask = orc.make_instance(n, m, k, seed=21, kind=kind, n_indices=None if kind == "readme" else int(0.35 * n * m))
        inst = orc.Instance(A, mask, GAMMA, k)
        cuts = path_of(orc, inst, cut_type, depth)
        lo = hi = None
        if custom:
            lo, hi = orc.default_U_bounds(n, k)
            lo = lo.copy(); hi = hi.copy()
            lo[0, 0] = -0.5; hi[1, 0] = 0.25; lo[n - 1, k - 1] = -1.0; hi[2, k - 1] = 0.75      # two rows added, one default row removed
        out.append((inst, cuts, cut_type, lo, hi))
    return out


def test_rows_and_basis_match_the_oracle(omc, orc, cases):
    cert = omc.pkg.certificate
    for (inst, cuts, cut_type, lo, hi) in cases:
        rows = orc.build_rows(inst, cuts, cut_type, lo, hi)
        mine = cert.node_rows(inst.n, inst.k, cuts, cut_type, lo, hi)
        assert [r[0] for r in mine] == rows.kinds
        assert np.array_equal(np.array([r[3] for r in mine]), np.array(rows.rhs))
        for a, b in zip(mine, rows.CU):
            assert np.array_equal(a[2], b)
        assert np.array_equal(cert.row_basis(mine, inst.n, inst.k), orc.row_subspace(rows, inst.n, inst.k))


def test_formula_against_the_oracle(omc, orc, cases):
    cert = omc.pkg.certificate
    rng = np.random.default_rng(7)
    for (inst, cuts, cut_type, lo, hi) in cases:
        rows = orc.build_rows(inst, cuts, cut_type, lo, hi)
        Q = orc.row_subspace(rows, inst.n, inst.k)
        for _ in range(4):
            c = random_admissible(cert, rng, inst, len(rows), Q)
            ref = orc.dual_bound_from(inst, c.Lam, rows, c.lam, Q, c.Psi3)
            got = cert.dual_bound(inst.A, inst.indices, GAMMA, inst.k, cuts, cut_type, c, lo, hi)
            assert got == pytest.approx(ref, rel=1e-12)
            d = cert.defects(c, inst.indices)
            assert d["off_support"] == 0.0 and d["min_lam"] >= 0.0 and d["psi_min_eig"] >= -1e-14


def test_sanitising_gives_a_valid_bound(omc, orc, cases):
    cert = omc.pkg.certificate
    rng = np.random.default_rng(11)
    inst, _, cut_type, lo, hi = cases[0]
    cuts = []                                              # the root: the oracle certifies it in a few hundred iterations
    sol = orc.sdp_relaxation(inst, cuts, cut_type, params=orc.RelaxParams(rho_scale=8.0), want_certificate=False)
    assert sol["termination_status"] == 0                  # the oracle certifies this node: its objective is within 1e-6 of the optimum
    obj = sol["objective"]
    rows = sol["rows"]; Q = sol["Q"]
    # the oracle's own final multipliers, spoiled: a negative lam entry, an indefinite Psi3, mass off Omega
    _, Lam = inst.f_value(sol["Y"], want=True)
    good = cert.Certificate(Lam=Lam, lam=sol["lam"].copy(), Q=Q, Psi3=np.zeros((Q.shape[1] + inst.k,) * 2))
    bad_lam = good.lam.copy(); bad_lam[1] = -0.3
    G = rng.standard_normal(good.Psi3.shape); bad_psi = 0.05 * (G + G.T)
    bad_Lam = Lam + np.where(inst.indices, 0.0, 0.2)
    bad = cert.Certificate(Lam=bad_Lam, lam=bad_lam, Q=Q, Psi3=bad_psi)
    d = cert.defects(bad, inst.indices)
    assert d["off_support"] == pytest.approx(0.2 * (~inst.indices).sum()) and d["min_lam"] == -0.3 and d["psi_min_eig"] < 0.0
    got = cert.dual_bound(inst.A, inst.indices, GAMMA, inst.k, cuts, cut_type, bad)
    w, V = np.linalg.eigh(bad_psi)
    ref = orc.dual_bound_from(inst, Lam, rows, np.maximum(bad_lam, 0.0), Q, (V * np.maximum(w, 0.0)) @ V.T)
    assert got == pytest.approx(ref, rel=1e-12)
    assert got <= obj + OBJ_REL * max(1.0, abs(obj))
    # the unspoiled multipliers too, and random admissible ones: every admissible certificate bounds the optimum from below
    for c in [good] + [random_admissible(cert, rng, inst, len(rows), Q) for _ in range(4)]:
        assert cert.dual_bound(inst.A, inst.indices, GAMMA, inst.k, cuts, cut_type, c) <= obj + OBJ_REL * max(1.0, abs(obj))


def test_plan_and_symbols(omc):
    lib = omc.load()
    for s in ("omc_relax_keep_certificates", "omc_relax_fetch_certificate", "omc_certificate_plan", "omc_dual_bound_batch"):
        assert hasattr(lib, s) and s in omc.EXPORTS
    cert = omc.pkg.certificate
    for (n, k, nnz, L, extra) in [(12, 1, 63, 0, 0), (16, 2, 112, 2, 0), (24, 1, 252, 3, 5), (100, 8, 3000, 12, 0), (5, 2, 9, 6, 3)]:
        out = np.zeros(6, np.int64)
        assert lib.omc_certificate_plan(n, k, nnz, L, extra, out.ctypes.data_as(C.c_void_p)) == 0
        p = cert.plan(n, k, nnz, L, extra)
        assert [int(v) for v in out] == [p["Lam"], p["lam"], p["Q"], p["Psi3"], p["bytes_per_node"], p["rmax"]]
        assert omc.pkg.api.certificate_plan(n, k, nnz, L, extra) == p
    out = np.zeros(6, np.int64)
    assert lib.omc_certificate_plan(0, 1, 1, 0, 0, out.ctypes.data_as(C.c_void_p)) == -3
    assert lib.omc_certificate_plan(12, 9, 1, 0, 0, out.ctypes.data_as(C.c_void_p)) == -4
    assert lib.omc_certificate_plan(12, 1, 1, 0, 0, None) == -3
    # NULL handles are refused before anything touches a device
    assert lib.omc_relax_keep_certificates(None, 1) == -3
    assert lib.omc_relax_fetch_certificate(None, 0, None, None, None, None, None, None, None, None) == -3
    assert lib.omc_dual_bound_batch(None, 1, 0, 1, None, None, None, None, None, None, None, None, None, None, None, None) == -3
