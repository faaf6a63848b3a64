"""CPU tests of the Shor-mode certificate checker (certificate.py: numpy only) against the oracle's own multipliers, and of the host-only
plan of the C ABI.  No GPU.

The oracle (oracle/omc_oracle_shor.py) evaluates shor_dual_bound at every check of a solve; wrapping it captures the multipliers of every
check.  Packed into a ShorCertificate they must give the oracle's value of that check (1e-12 relative), and a valid lower bound under any
perturbation.  Conditions: OBJ_REL = 2e-6 against the oracle's certified objective (the project's tolerance between a valid bound and a value
certified to 1e-6).  Nothing here is pinned to the reference (Julia + Mosek, no fixtures)."""
import ctypes as C
import math

import numpy as np
import pytest

GAMMA = 80.0
OBJ_REL = 2e-6


@pytest.fixture(scope="module")
def sh():
    import omc_oracle_shor
    return omc_oracle_shor


@pytest.fixture(scope="module")
def cert(omc):
    return omc.pkg.certificate


def _instance(orc, n, m, nidx, seed, noise, kind="lowrank"):
    A, mask = orc.make_instance(n, m, 1, n_indices=nidx, seed=seed, noise=noise, kind=kind)
    return A, mask, orc.Instance(A, mask, GAMMA, 1)


def captured_solve(sh, cert, inst, minors, soc, cuts=(), **kw):
    """The oracle's solve with the arguments and the value of shor_dual_bound at every check: (result, [(ShorCertificate, scaled value)])."""
    seen = []
    plain = sh.shor_dual_bound
    sc = sh.shor_scale(inst)

    def recording(inst_, st, Ah, rows, lam, Q, Psi3, Gam, zeta_adm, xi_at, Xbar, qX, cX, cW, cT):
        v = plain(inst_, st, Ah, rows, lam, Q, Psi3, Gam, zeta_adm, xi_at, Xbar, qX, cX, cW, cT)
        seen.append((cert.ShorCertificate(scale=sc, lam=np.array(lam), Q=np.array(Q), Psi3=np.array(Psi3), Gam=np.array(Gam).reshape(-1, 5, 5),
                                          zeta=np.array(zeta_adm), xi=np.array(xi_at), Xbar=np.array(Xbar)), float(v)))
        return v

    sh.shor_dual_bound = recording
    try:
        ro = sh.sdp_relaxation_shor(inst, minors, soc, cuts=cuts, params=sh.ShorParams(**kw))
    finally:
        sh.shor_dual_bound = plain
    assert ro["scale"] == sc
    return ro, seen


class Root:
    """12 x 14 with its 152 class-4 minors: the instance, the lists, the oracle's certified root with every check captured, and a depth-1 cut
    node at a 500-iteration cap."""

    def __init__(self, orc, sh, cert):
        self.A, self.mask, self.inst = _instance(orc, 12, 14, 70, 2, 0.1)
        self.minors, self.soc = sh.driver_shor_lists(self.mask, (4,))
        assert len(self.minors) == 152
        self.ro, self.seen = captured_solve(sh, cert, self.inst, self.minors, self.soc, eps_gap=1e-6)
        assert self.ro["termination_status"] == 0
        r0 = orc.sdp_relaxation(self.inst)
        x, _ = orc.breakpoint_vector(r0["Y"], r0["U"])
        self.cut_node = [(x, r0["U"], ["left"])]
        self.rc, self.seen_cut = captured_solve(sh, cert, self.inst, self.minors, self.soc, cuts=self.cut_node, eps_gap=1e-12, max_iters=500)
        self.obj = float(self.ro["objective"])

    def bound(self, cert, c, node=(), **kw):
        return cert.shor_dual_bound(self.A, self.mask, GAMMA, list(node), "linear", self.minors, None, c, **kw)


@pytest.fixture(scope="module")
def root(orc, sh, cert):
    return Root(orc, sh, cert)


# ---- 1. exact reproduction on the oracle ------------------------------------------------------------------------------------------------------
def _checks(root):
    return (((), root.ro, root.seen), (root.cut_node, root.rc, root.seen_cut))


def test_every_check_of_the_oracle_is_reproduced(root, cert):
    """shor_dual_bound (sanitised) within 1e-12 relative of the oracle's value at every check of the 12 x 14 / 152-minor root (43 checks) and
    of its depth-1 cut node at the 500 cap.  Measured: at most 5.1e-15.  The oracle's Gam_q = rho r4 (P - input) has eigenvalues down to
    -2.6e-14 (rounding of the projection times the penalty).  Taking the PSD part of every block before the spread moves all 152 of them by
    that rounding, and the bound with them, by 5.7e-13 ... 5.1e-12 relative (6.1e-11 at the one early check whose bound is -0.11): that
    evaluation alone misses this condition.  The second evaluation of shor_dual_bound leaves such blocks as they are -- the shift of the
    spread already covers a negative part of that size -- and the larger of the two valid bounds is returned."""
    worst = 0.0
    misses = []
    for node, ro, seen in _checks(root):
        s2 = ro["scale"] ** 2
        for i, (c, v) in enumerate(seen):
            mine = root.bound(cert, c, node)
            ref = v / s2
            if math.isinf(ref):
                assert mine == ref
                continue
            rel = abs(mine - ref) / abs(ref)
            worst = max(worst, rel)
            print(f"cuts {len(node)} check {i}: oracle {ref!r} sanitised {mine!r} relative difference {rel:.3e}")
            if rel > 1e-12:
                misses.append((len(node), i, rel))
    print(f"largest relative difference to the oracle: {worst:.3e}")
    assert not misses, misses


def test_unsanitised_evaluation_equals_the_oracle_at_every_check(root, cert):
    """evaluate_shor (steps 2-8, nothing sanitised) against the oracle's value of the same check: 1e-12 relative; the best check is the
    reported dual_bound."""
    for node, ro, seen in _checks(root):
        s2 = ro["scale"] ** 2
        st = cert.shor_structure(12, 14, root.mask, root.minors, None)
        rows = cert.node_rows(12, 1, list(node), "linear")
        vals = []
        for c, v in seen:
            mine = cert.evaluate_shor(root.A, root.mask, GAMMA, rows, st, c)
            ref = v / s2
            vals.append(mine)
            assert mine == ref if math.isinf(ref) else abs(mine - ref) <= 1e-12 * abs(ref), (mine, ref)
        assert len(seen) == len(ro["hist"])
        assert max(v / s2 for _, v in seen) == ro["dual_bound"]
        assert abs(max(vals) - ro["dual_bound"]) <= 1e-12 * abs(ro["dual_bound"])
    # the explicit SOC list and the complement shorthand are the same structure
    c, v = root.seen[-1]
    assert cert.shor_dual_bound(root.A, root.mask, GAMMA, [], "linear", root.minors, root.soc, c) == root.bound(cert, c)


# ---- 2. validity under admissible noise ---------------------------------------------------------------------------------------------------------
def perturbed(cert, c, rng, rel=1e-2, gam_rel=1e-3):
    Gam = c.Gam.copy()
    nrm = np.sqrt((Gam * Gam).sum((1, 2)))
    G = rng.standard_normal((len(Gam), 5, 5))
    GG = G @ np.transpose(G, (0, 2, 1))
    GG *= (gam_rel * rng.random(len(Gam)) * nrm / np.maximum(np.sqrt((GG * GG).sum((1, 2))), 1e-300))[:, None, None]
    f = lambda a: a * (1.0 + rel * rng.uniform(-1.0, 1.0, np.shape(a)))
    r = c.Psi3.shape[0]
    H = rng.standard_normal((r, r)) * 1e-2 * math.sqrt(max(np.abs(c.Psi3).max(), 1e-12))
    return cert.ShorCertificate(scale=c.scale, lam=f(c.lam), Q=c.Q, Psi3=c.Psi3 + H @ H.T, Gam=Gam + GG, zeta=f(c.zeta), xi=f(c.xi), Xbar=f(c.Xbar))


def test_perturbed_multipliers_stay_below_the_optimum(root, cert):
    rng = np.random.default_rng(11)
    c = root.seen[-1][0]
    cap = root.obj + OBJ_REL * max(1.0, abs(root.obj))
    vals = [root.bound(cert, perturbed(cert, c, rng)) for _ in range(50)]
    print(f"optimum {root.obj!r}; 50 perturbed bounds in [{min(vals)!r}, {max(vals)!r}]; unperturbed {root.bound(cert, c)!r}")
    assert all(v <= cap for v in vals)
    assert np.isfinite(vals).all() and min(vals) > root.obj - 0.5 * abs(root.obj)      # tight: the noise costs little, the test is not vacuous


def test_random_multipliers_smoke(root, cert):
    """Multipliers from scratch give bounds far below the optimum (they prove little); kept small so that mu > 0 and the bound is finite."""
    rng = np.random.default_rng(12)
    c0 = root.seen[-1][0]
    n, m = root.A.shape
    cap = root.obj + OBJ_REL * max(1.0, abs(root.obj))
    finite = 0
    for _ in range(20):
        G = rng.standard_normal((152, 5, 5))
        Gam = G @ np.transpose(G, (0, 2, 1))
        Gam *= 0.02 / np.abs(Gam).max()
        c = cert.ShorCertificate(scale=c0.scale, lam=np.abs(rng.standard_normal(len(c0.lam))) * 0.1, Q=c0.Q, Psi3=np.zeros_like(c0.Psi3), Gam=Gam,
                                 zeta=rng.random(m) * 0.005, xi=rng.standard_normal((n, m)) * 0.1, Xbar=rng.standard_normal((n, m)) * 0.1)
        v = root.bound(cert, c)
        assert v <= cap
        finite += int(np.isfinite(v))
    print(f"{finite} of 20 random certificates gave a finite bound")
    assert finite >= 10


# ---- 3. validity for inadmissible input ---------------------------------------------------------------------------------------------------------
def test_inadmissible_multipliers_are_sanitised_and_reported(root, cert):
    rng = np.random.default_rng(13)
    c = root.seen[-1][0]
    cap = root.obj + OBJ_REL * max(1.0, abs(root.obj))
    clean_val, clean_df = root.bound(cert, c, want_defects=True)
    assert clean_df["gam_min_eig"] >= -1e-12 and clean_df["min_zeta"] >= 0.0 and clean_df["min_lam"] >= 0.0 and clean_df["psi_min_eig"] >= -1e-12
    scale_g = np.abs(c.Gam).max()
    for trial in range(10):
        Gam = c.Gam + 0.05 * scale_g * rng.standard_normal(c.Gam.shape)                 # indefinite, not symmetric, V entries do not cancel
        zeta = c.zeta - 0.5 * np.abs(c.zeta).max() * rng.random(len(c.zeta)) - 1e-3
        lam = c.lam - 0.1 * rng.random(len(c.lam))
        Psi = c.Psi3 + 0.1 * max(np.abs(c.Psi3).max(), 1e-3) * (rng.standard_normal(c.Psi3.shape) - 2.0 * np.eye(len(c.Psi3)))
        bad = cert.ShorCertificate(scale=c.scale, lam=lam, Q=c.Q, Psi3=Psi, Gam=Gam, zeta=zeta, xi=c.xi, Xbar=c.Xbar)
        v, df = root.bound(cert, bad, want_defects=True)
        assert v <= cap, (trial, v)
        # each of the two ways of making the blocks admissible on its own, the other multipliers clean
        st = cert.shor_structure(12, 14, root.mask, root.minors, None)
        rows = cert.node_rows(12, 1, [], "linear")
        sym = 0.5 * (Gam + np.transpose(Gam, (0, 2, 1)))
        for G2 in (sym, cert.sanitise_shor(bad, st)[0].Gam):
            v2 = cert.evaluate_shor(root.A, root.mask, GAMMA, rows, st, cert.ShorCertificate(scale=c.scale, lam=c.lam, Q=c.Q, Psi3=c.Psi3, Gam=G2,
                                                                                          zeta=c.zeta, xi=c.xi, Xbar=c.Xbar))
            assert v2 <= cap, (trial, v2)
        assert df["gam_min_eig"] < 0.0 and df["min_zeta"] < 0.0 and df["min_lam"] < 0.0 and df["psi_min_eig"] < 0.0 and df["v_residual"] > 0.0
    # only the V entries wrong: the spread makes them cancel and the shift pays for it
    Gam = c.Gam.copy()
    Gam[:, 1, 2] += 0.01 * scale_g; Gam[:, 2, 1] += 0.01 * scale_g; Gam[:, 1, 4] += 0.02 * scale_g; Gam[:, 4, 1] += 0.02 * scale_g
    Gam += 0.1 * scale_g * np.eye(5)[None]                                                 # still PSD after the change
    v, df = root.bound(cert, cert.ShorCertificate(scale=c.scale, lam=c.lam, Q=c.Q, Psi3=c.Psi3, Gam=Gam, zeta=c.zeta, xi=c.xi, Xbar=c.Xbar),
                       want_defects=True)
    assert df["v_residual"] > 0.0 and df["gam_min_eig"] >= 0.0 and v <= cap and v < clean_val


# ---- 4. scale -----------------------------------------------------------------------------------------------------------------------------------
def test_scale(root, cert):
    """The program is homogeneous of degree 2 in A: X scales with s, W and Theta with s^2, Y and U not at all.  Multipliers rescaled
    consistently -- zeta fixed, xi and Xbar by s, lam and Psi3 by s^2 (their constraints are on (Y, U), the objective grows by s^2), the blocks by
    D Gam D with D = diag(s, 1, 1, 1, 1) (the row of the constant 1) -- give s^2 times the bound for s * A.  Leaving lam, Psi3 and Gam untouched
    does not: their constants do not scale.  The exported `scale` does the same job from the other side: s * A with scale / s is the same
    scaled program, so the bound is s^2 times as large."""
    c = root.seen[-1][0]
    # blocks without entries on V1 / V2 / V3 (an arrow: first row and diagonal), so that nothing is spread and no shift lands on the (0,0) entry,
    # which alone scales with s^2; diagonally dominant enough to be PSD
    g = 0.05 * c.Gam[:, 0, 1:5]
    g00 = c.Gam[:, 0, 0] + 1e-3 * np.abs(c.Gam).max()
    arrow = np.zeros_like(c.Gam)
    arrow[:, 0, 0] = g00; arrow[:, 0, 1:5] = g; arrow[:, 1:5, 0] = g
    arrow[:, [1, 2, 3, 4], [1, 2, 3, 4]] = ((g * g).sum(1) / g00)[:, None] * 1.0001
    c = cert.ShorCertificate(scale=c.scale, lam=c.lam, Q=c.Q, Psi3=c.Psi3, Gam=arrow, zeta=c.zeta, xi=c.xi, Xbar=c.Xbar)
    v, df = root.bound(cert, c, want_defects=True)
    assert np.isfinite(v) and df["v_residual"] == 0.0 and df["gam_min_eig"] >= 0.0
    for s in (0.5, 3.0):
        D = np.diag([s, 1.0, 1.0, 1.0, 1.0])
        cs = cert.ShorCertificate(scale=c.scale, lam=s * s * c.lam, Q=c.Q, Psi3=s * s * c.Psi3, Gam=D[None] @ c.Gam @ D[None], zeta=c.zeta,
                                  xi=s * c.xi, Xbar=s * c.Xbar)
        assert cert.shor_dual_bound(s * root.A, root.mask, GAMMA, [], "linear", root.minors, None, cs) == pytest.approx(s * s * v, rel=1e-11)
        ct = cert.ShorCertificate(scale=c.scale / s, lam=c.lam, Q=c.Q, Psi3=c.Psi3, Gam=c.Gam, zeta=c.zeta, xi=c.xi, Xbar=c.Xbar)
        assert cert.shor_dual_bound(s * root.A, root.mask, GAMMA, [], "linear", root.minors, None, ct) == pytest.approx(s * s * v, rel=1e-13)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        cb = cert.ShorCertificate(scale=bad, lam=c.lam, Q=c.Q, Psi3=c.Psi3, Gam=c.Gam, zeta=c.zeta, xi=c.xi, Xbar=c.Xbar)
        assert root.bound(cert, cb) == -math.inf


# ---- 5. column types ----------------------------------------------------------------------------------------------------------------------------
def test_column_types(root, orc, sh, cert):
    assert (cert.shor_structure(12, 14, root.mask, root.minors, None).ctype == 0).all()
    A, mask = orc.make_instance(6, 7, 1, n_indices=42, seed=7, noise=0.1)
    assert mask.all()
    inst = orc.Instance(A, mask, GAMMA, 1)
    allm = orc.shor_constraints_indexes(mask, [4])
    assert len(allm) == 15 * 21
    thin = [q for q in allm if q[1] <= 4]                                                 # rows 5 and 6 stay outside the minors
    for minors, ctype in ((allm, 2), (thin, 1)):
        mi, soc = sh.driver_shor_lists(mask, minors=minors)
        st = cert.shor_structure(6, 7, mask, mi, None)
        ref = sh.ShorStructure(6, 7, mi, soc, mask)
        assert (st.ctype == ctype).all() and (ref.ctype == ctype).all()
        assert np.array_equal(st.inC, ref.inC) and np.array_equal(st.inS, ref.inS)
        ro, seen = captured_solve(sh, cert, inst, mi, soc, eps_gap=1e-6)
        assert ro["termination_status"] == 0
        s2 = ro["scale"] ** 2
        obj = float(ro["objective"])
        for c, v in seen[-3:]:
            raw = cert.evaluate_shor(A, mask, GAMMA, cert.node_rows(6, 1, [], "linear"), st, c)
            assert abs(raw - v / s2) <= 1e-12 * abs(v / s2)
            mine = cert.shor_dual_bound(A, mask, GAMMA, [], "linear", mi, None, c)
            assert mine <= obj + OBJ_REL * max(1.0, abs(obj)) and mine >= v / s2 - 1e-9 * abs(v / s2)
        rng = np.random.default_rng(ctype)
        for _ in range(5):
            assert cert.shor_dual_bound(A, mask, GAMMA, [], "linear", mi, None, perturbed(cert, seen[-1][0], rng)) <= obj + OBJ_REL * max(1.0, abs(obj))


def test_empty_minor_list_reduces_to_the_base_relaxation(orc, sh, cert):
    A, mask, inst = _instance(orc, 10, 12, 60, 1, 0.3)
    minors, soc = sh.driver_shor_lists(mask, minors=[])
    ro, seen = captured_solve(sh, cert, inst, minors, soc, eps_gap=1e-6)
    base_obj = float(orc.sdp_relaxation(inst, params=orc.RelaxParams(rho_scale=4.0))["objective"])
    c, v = seen[-1]
    assert c.Gam.shape == (0, 5, 5)
    mine = cert.shor_dual_bound(A, mask, GAMMA, [], "linear", [], None, c)
    assert abs(mine - v / ro["scale"] ** 2) <= 1e-12 * abs(mine)                          # no blocks: nothing for the sanitiser to change
    assert mine <= base_obj + OBJ_REL * max(1.0, abs(base_obj))
    assert mine >= base_obj - 1e-4 * abs(base_obj)                                        # and it is the base relaxation's value, not a loose bound


# ---- 6. plan and symbols ------------------------------------------------------------------------------------------------------------------------
def test_plan_and_symbols(omc, cert):
    lib = omc.load()
    for s in ("omc_relax_keep_shor_certificates", "omc_shor_certificate_plan", "omc_relax_fetch_shor_certificate"):
        assert hasattr(lib, s) and s in omc.EXPORTS
    n, m, k, nqs, cuts, box = 12, 14, 1, 152, 2, 3
    out = np.zeros(10, np.int64)
    assert lib.omc_shor_certificate_plan(n, m, k, C.c_int64(nqs), cuts, box, out.ctypes.data_as(C.c_void_p)) == 0
    Rmax = 1 + 1 + 3 + 2 * 3                      # trace, the default box row, 3 more box rows, 2 cuts of 2 k + 1 rows
    rmax = 1 + 3 + 2
    psi = (rmax + 1) ** 2
    assert list(out[:7]) == [Rmax, n * rmax, psi, 15 * nqs, m, n * m, n * m]
    per = 15 * nqs + m + 2 * n * m + Rmax + psi
    assert out[7] == 8 * (1 + per) + 8 and out[8] == 8 * (2 + per) + 8 and out[9] == rmax
    assert out[7] == 120 * nqs + 8 * (2 * n * m + m + Rmax + psi) + 16                    # 120 bytes per minor and node, the rest, the header
    p = cert.shor_plan(n, m, k, nqs, cuts, box)
    assert [p[key] for key in ("lam", "Q", "Psi3", "Gam", "zeta", "xi", "Xbar", "bytes_per_node", "bytes_per_slot", "rmax")] == list(out)
    assert omc.pkg.api.shor_certificate_plan(n, m, k, nqs, cuts, box) == p
    # config 3: 632 732 minors, 200 x 200 -> about 76 MB per node
    assert 75e6 < cert.shor_plan(200, 200, 1, 632732)["bytes_per_node"] < 77e6
    assert lib.omc_shor_certificate_plan(n, m, 2, C.c_int64(nqs), 0, 0, out.ctypes.data_as(C.c_void_p)) == -4      # rank k > 1: unsupported
    assert lib.omc_shor_certificate_plan(0, m, 1, C.c_int64(nqs), 0, 0, out.ctypes.data_as(C.c_void_p)) == -3


def test_pack_and_unpack_gam(cert):
    rng = np.random.default_rng(3)
    G = rng.standard_normal((7, 5, 5)); G = G + np.transpose(G, (0, 2, 1))
    P = cert.pack_gam(G, stride=9)
    assert P.shape == (15, 9) and (P[:, 7:] == 0).all()
    assert P[0, 2] == G[2, 0, 0] and P[1, 2] == G[2, 0, 1] and P[2, 2] == G[2, 1, 1] and P[4, 2] == G[2, 1, 2] and P[8, 2] == G[2, 2, 3]
    assert P[11, 2] == G[2, 1, 4] and P[13, 2] == G[2, 3, 4] and P[14, 2] == G[2, 4, 4]
    assert np.array_equal(cert.unpack_gam(P, 7), G)
