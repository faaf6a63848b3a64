"""The Shor-mode relaxation after t iterations (csrc/omc_shor_relax.hip: k_shor_minor_pre, k_shor_vkeys, k_shor_cols, k_shor_minor_post, k_shor_reduce,
k_shor_rescale, k_shor_harvest, with k_global's Shor flag and the big cone) against the float64 oracle at the same t, array by array.  Run on
the MI355X box: `pytest -m gpu`.  Cases: tests/shor_iter_cases.py; reference and its own error e_ref: oracle/omc_shor_iter_ref.py,
tests/test_shor_iter_cpu.py.  Every run is Engine.matrix_completion_SDP_relaxation(..., add_Shor_valid_inequalities=True, want_Theta=True,
want_V=True) with max_iters = t and eps_gap = 1e-12, one slot.

Compared: iters == t; X, W (the completed W of k_shor_harvest, with Theta_jj = sum_i W_ij to 1e-12), Theta, Y, U, V1 / V2 / V3 (the engine's
per-minor V mapped through the keys k12 / k34 / k13 / k24); objective; rp, rd (omc_debug_residuals); the dual bound where the reference's bound
of that check is finite (a disagreement in finiteness is printed); rho of omc_last_solver_info in case C (see below).

Bound per array S (u = 2^-53; the factor 4 is the project's convention):
    ||S_gpu - S_ref||_F <= 4 max(e_ref(S), u sqrt(size) ||S_ref||_F) + L_S d(t),        scalars the same with |.|
    d(t) = relax t (J(1e-10, n + m, ||In0||_F) + J(1e-10, n, ||In1||_F) + J(1e-14, r + 1, ||In3||_F)),   J(tau, N, f) = (tau / 2)(1.5 N + sqrt N) f
d(t) is the stop term, in the scaled variables.  The big cone (orders 18, 26, 261 and 517 here) and the clip (orders 4 .. 257) are projected by
k_cone_ws at every order up to 1024 (omc_layout.h: ws_geometry gives lanes per pair for all of them; in LDS at 18 and 26, on the global slab
with 16 lanes per pair at 261 and 517; the multi-workgroup kernels start at OMC_CONE_MULTI_MIN = 1025), the small cone of order r + 1 by
k_small.  Both are one-sided Jacobi on the columns of A V, A = M + sigma I with the shift sigma = 1.5 ||M||_F (A is positive definite, its
eigenvalues a_p lie in [0.5, 2.5] ||M||_F).  k_cone_ws leaves a pair of columns alone once their cross product is below tau = 1e-10 times the
product of their norms (omc_device.hip, "rotation threshold"; it ends after a sweep in which no cross product exceeded sqrt(tau)); k_small sweeps to
1e-14.  V is a product of rotations, exactly orthogonal, and the column norms are the a_p, so what is left is |v_p' A^2 v_q| <= tau a_p a_q, that
is an off-diagonal E of A in the basis V with |E_pq| <= tau a_p a_q / (a_p + a_q) <= tau sqrt(a_p a_q) / 2.  The kernel returns P_+(M - E), and
P_+ is non-expansive: per call ||P - P_+(M)||_F <= ||E||_F <= (tau / 2) tr A = (tau / 2)(N sigma + tr M) <= J(tau, N, ||M||_F).  The threshold
is relative to the SHIFTED columns, pair by pair, so the figure grows with the order: the issue's sketch (tau ||input||_F per call) leaves the
shift out.  Measured against that sketch the runs below reach 0.52 of it at order 18, 3.6 times it at order 261 and 41 times it at order
517 (Y of F-257x260 at t = 3: 5.8e-7 for ||In1||_F = 8.8); against J they stay below 0.1.  J was derived from the kernel before any run.
At t = 1 from the cold start the three inputs are diagonal, nothing is rotated or left, and d(1) = 0: those runs are pinned at rounding level.
A projection's error enters the next iterate times the over-relaxation (T = relax P + ...); the other projections are non-expansive, the global
step is an average and the dual updates are differences of those, so the term adds up: relax t times the per-call figures, with
In0 = G - D0, In1 = Y - D1, In3 the small cone's input, their largest Frobenius norms over the t iterations taken from the reference
(cone_inputs), never from the device.  The order-5 projections (cyclic Jacobi to 1e-32 off / diag) and the paraboloid's Newton loop (1e-16) end
at rounding level and add nothing.
L_S carries d(t) to what is returned: 1 / scale for X, 1 / scale^2 for Theta and V; for the completed W (2 + sqrt n)(1 / scale^2 + 2 max|X| / scale):
X^2 on the SOC entries and the column's slack, a sum over the column; 1 for Y; for U = Y Q (Q'YQ)^+ Vt the derivative's norm
||S^+|| (||Vt|| + ||YQ|| ||S^+|| ||Vt|| + ||YQ||), S = Q'YQ, applied to the whole allowance of Y and Vt (U is formed from them at the harvest; at
t = 1 with cuts that is 1e-15 where U's own rounding is 1e-16); for the objective the norm of its gradient in the scaled point over scale^2; 6 for
rp and rd (norms of at most 8 stacked differences, each moving by 2 d at most); for the dual bound, which has no closed form in the point,
the first-order figure omc_shor_iter_ref.sensitivity measures on the reference.  Nothing is sized from the device's output.
The identity Theta_jj = sum_i W_ij holds to max(1e-12, 4 n u sum_i |W_ij|): 1e-12 as in the other Shor tests wherever the rounding of two
n-term sums in different orders is below it, which is every case but the two F shapes (column sums of 2000 and more: 1e-12 is 2 ulps there).

Tracked blocks (k_cone_sub): cones of order 48 and more have one (the F cases; it is seeded at the first iteration).  In runs of three
iterations it serves none: asserted for every run through omc_last_shor_subspace_stats and omc_last_subspace_stats (calls - fallbacks == 0
for the big cone and for the clip), so no run needs OMC_SHOR_NO_SUBSPACE and no term of the block enters the bound.

omc_last_solver_info reports the penalty the batch was staged with, not a slot's bumped one: in case C it must equal the start value, and the
bump itself is pinned by the state at t = 3, 4, 6 (tests/test_shor_iter_cpu.py: the reference without the bump is 1e-3 away and more).

DEFECT FOUND AND FIXED with this module: omc_relax_solve checked only at multiples of check_every, so a cap off that grid (every t here
but none of the suite's Shor caps before) ran on to the next multiple -- max_iters = 1 returned iters = 25 and the state of iteration 25.  The
oracle checks at it % check_every == 0 or it == max_iters.  In Shor mode the loop now also checks at a node's own cap, and k_check_final
leaves a slot alone at a check that is neither on its grid nor its cap.

MEASURED below: worst error over bound per array over all runs (every run prints its own line)."""
import numpy as np
import pytest

import shor_iter_cases as C
import omc_shor_iter_ref as R

pytestmark = pytest.mark.gpu
U_RND = R.U_RND
TAU_WS = 1e-10        # k_cone_ws: rotation threshold on the relative cross product
TAU_SMALL = 1e-14     # k_small: jacobi_sweeps_wave16
RELAX = 1.6           # over-relaxation of the splitting (ShorParams.relax, the engine's default)
KEYS = R.ARRAYS + ("objective", "rp", "rd")
MEASURED = """
worst error over bound per array, product library, MI355X (31 runs of 13 cases and the batch; a value of 1 would be a failure):
              t = 1 (rounding level, d = 0)                 t >= 2 (stop term)
  X           0.034  E-half-soc       5.3e-15 / 1.6e-13     0.040   F-257x260-t3   4.9e-06 / 1.3e-04
  W           0.057  A                5.9e-14 / 1.0e-12     0.0003  E-empty-t3     1.2e-08 / 4.3e-05
  Theta       0.093  E-empty          2.5e-14 / 2.7e-13     0.059   F-257x260-t3   1.1e-04 / 2.0e-03
  Y           0.568  B-depth1         6.8e-16 / 1.2e-15     0.072   F-257x260-t3   5.8e-07 / 8.1e-06
  U           0.178  B-depth2         1.1e-15 / 6.1e-15     4e-05   B-depth1-t3    3.0e-10 / 7.3e-06
  V1, V2, V3  exactly 0 on both sides                       3e-05   D-256 .. D-513 2.6e-11 / 9.3e-07
  objective   0.099  D-256            2.1e-14 / 2.2e-13     0.0001  E-half-soc-t3  2.0e-09 / 1.5e-05
  rp          0.499  E-s0             3.6e-15 / 7.1e-15     0.0001  batch node 1   1.4e-10 / 1.7e-06
  rd          0.849  F-257x260        7.1e-15 / 8.4e-15     0.0004  E-half-soc-t3  6.5e-10 / 1.8e-06
  dual bound  finite on both sides at t = 1 in every case and at t = 3 in F-4x257, -inf on both sides elsewhere; error 8.9e-15 (A) .. 3.7e-10
              (F-257x260) at t = 1 and 8.9e-08 at F-4x257-t3, 0.001 of the bound at most
  From t = 2 on the bound is the stop term: k_cone_ws's threshold 1e-10 is what separates the device from the oracle (1e-9 in X, 1e-8 in
  Theta at order 18), and V, W, U and the scalars, which the cones reach only through X and Theta, stay 1e3 - 1e4 below it.  The t = 1 runs
  are the sharp ones for k_shor_minor_pre, k_shor_vkeys, k_shor_cols, k_shor_minor_post, k_shor_reduce and k_shor_harvest; k_shor_rescale,
  the keys with V3 != 0 and the warm-started cone run from t = 2 on.
  Tracked blocks: (0, 0) iterations served in every run (seeded in the F cases).  rho of omc_last_solver_info: 0.05 in C at t = 2, 3, 4, 6.
  Whole module: 7 s.
Mutants (each built once, never committed): runs of this module that fail (of 32) / of the 57 Shor GPU tests the suite had before
(test_gpu_shor*.py and the Shor-mode tests of test_cone_multi.py).  The module's column was measured with d(1) and U's allowance as first
written (looser than now at t = 1).
  k_shor_vkeys reads only entry 11 for V3               19 / 15 and 25 fixture errors   (every run with t >= 2 and the batch; at t = 1 the two copies are equal)
  k_shor_minor_post weights off-diagonals by 1 in r2    30 / 0    (every run with minors: rp)
  k_shor_rescale skips Tq                                3 / 4    (C-t3, C-t4, C-t6)
  k_shor_cols drops rd2's W term                        30 / 0    (every run with minors: rd)
  k_shor_cols uses cnt of the previous row in wbar      30 / 6 of the first 8, then the run was ended at a failure text naming a HIP error
                                                                  (config 3) and not repeated
"""


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


def _residuals(omc, eng, nslots):
    rp = np.zeros(nslots); rd = np.zeros(nslots)
    omc.pkg._lib.check(eng._lib.omc_debug_residuals(eng._h, omc.pkg._lib.ptr(rp), omc.pkg._lib.ptr(rd)))
    return rp, rd


def _keyed(st, V):
    """the engine's per-minor V (nq, 5) as the oracle's V1, V2, V3; every copy of a key must hold the key's value"""
    V1 = np.zeros(st.nv1); V2 = np.zeros(st.nv2)
    V1[st.k12] = V[:, 0]; V1[st.k34] = V[:, 1]; V2[st.k13] = V[:, 2]; V2[st.k24] = V[:, 3]
    if st.nq:
        assert np.array_equal(V1[st.k12], V[:, 0]) and np.array_equal(V1[st.k34], V[:, 1])
        assert np.array_equal(V2[st.k13], V[:, 2]) and np.array_equal(V2[st.k24], V[:, 3])
    return V1, V2, V[:, 4].copy()


def _solve(omc, A, mask, nodes, info, t, params, slots=1, knobs=()):
    """returns the results, rp, rd, the iterations the tracked blocks served (big cone, clip), omc_last_solver_info"""
    eng = omc.Engine(A, mask, C.GAMMA, 1)
    try:
        for kb in knobs:
            eng.tuning_set(kb, "1")
        P = omc.default_params(eps_gap=1e-12, max_iters=int(t), slots=slots, **params)
        out = eng.matrix_completion_SDP_relaxation(nodes, "linear", P, add_Shor_valid_inequalities=True, shor_info=info, want_Theta=True, want_V=True)
        rp, rd = _residuals(omc, eng, slots)
        big, clip = eng.shor_subspace_stats(), eng.subspace_stats()
        return out, rp, rd, (big["calls"] - big["fallbacks"], clip["calls"] - clip["fallbacks"]), eng.solver_info()
    finally:
        eng.close()


def _gpu_state(omc, c, t, knobs=()):
    out, rp, rd, sub, info = _solve(omc, c.A, c.mask, [c.cuts], [(c.minors, c.soc_gpu)], t, c.params, knobs=knobs)
    r = out[0]
    V1, V2, V3 = _keyed(c.structure, r["V"])
    g = dict(X=r["X"], W=r["W"], Theta=r["Theta"], Y=r["Y"], U=r["U"], V1=V1, V2=V2, V3=V3, objective=r["objective"], rp=float(rp[0]), rd=float(rd[0]),
             dual_bound=r["dual_bound"], iters=r["iters"], rho=float(info["rho"]), status=r["status_code"])
    return g, sub


def stop_factors(c, ref):
    """L_S of the module docstring, from the reference alone"""
    st = ref["structure"]; sc = ref["scale"]; s2 = sc * sc
    n, m = c.n, c.m
    mask = c.mask
    Xs = ref["X"] * sc
    cX = np.where(mask, -c.A * sc, 0.0)
    qX = np.where(mask & st.inS & (st.ctype == 0)[None, :], 1.0, 0.0)
    cW = np.where(mask & st.inC, 0.5, 0.0) - np.where(st.inC & (st.ctype == 1)[None, :], 0.5, 0.0)
    cT = 1.0 / (2.0 * C.GAMMA) + np.where(st.ctype == 1, 0.5, 0.0)
    L = dict(X=1.0 / sc, Theta=1.0 / s2, V1=1.0 / s2, V2=1.0 / s2, V3=1.0 / s2, Y=1.0, rp=6.0, rd=6.0)
    L["W"] = (2.0 + np.sqrt(n)) * (1.0 / s2 + 2.0 * float(np.abs(ref["X"]).max()) / sc)
    L["objective"] = (np.linalg.norm(cX + qX * Xs) + np.linalg.norm(cW) + np.linalg.norm(cT)) / s2
    Q = C.orc.row_subspace(ref["rows"], n, 1)
    if Q.shape[1]:
        S = Q.T @ ref["Y"] @ Q
        w = np.linalg.eigvalsh(0.5 * (S + S.T))
        keep = w[w > 1e-12 * max(1.0, w[-1])]      # the pseudo-inverse of recover_U
        si = 1.0 / keep[0] if len(keep) else 0.0
        Vt = Q.T @ ref["U"]; YQ = np.linalg.norm(ref["Y"] @ Q, 2)
        L["U"] = si * (np.linalg.norm(Vt) + YQ * si * np.linalg.norm(Vt) + YQ)
    else:
        L["U"] = 0.0
    return L


def jacobi_term(tau, order, fro):
    """(tau / 2) tr(M + sigma I) <= (tau / 2)(1.5 N + sqrt N) ||M||_F: what a one-sided Jacobi with the shift sigma = 1.5 ||M||_F leaves (docstring)"""
    return 0.5 * tau * (1.5 * order + np.sqrt(order)) * fro


def stop_term(c, t, ref):
    in0, in1, in3 = ref["cone_inputs"]
    r = C.orc.row_subspace(ref["rows"], c.n, 1).shape[1]
    return RELAX * t * (jacobi_term(TAU_WS, c.n + c.m, in0) + jacobi_term(TAU_WS, c.n, in1) + jacobi_term(TAU_SMALL, r + 1, in3))


def bounds(c, t, ref, e_ref):
    """{array: bound}, d.  t = 1 from the cold start: the three cones are handed diagonal matrices (diag(I k / n, 0), I k / n, diag(Q'Q k / n, 1)),
    no cross product is above zero and no rotation is made or skipped, so the state carries no stop term there and the pin is at rounding level."""
    d = 0.0 if t == 1 else stop_term(c, t, ref)
    L = stop_factors(c, ref)
    out = {}
    for key in KEYS:
        v = np.asarray(ref[key], float)
        out[key] = 4.0 * max(e_ref[key], U_RND * np.sqrt(v.size) * float(np.linalg.norm(v))) + L[key] * d
    # U is formed at the harvest from the returned Y and Vt = Q'U, so it inherits their whole allowance (not only d) through recover_U's derivative
    Q = C.orc.row_subspace(ref["rows"], c.n, 1)
    vt = float(np.linalg.norm(Q.T @ ref["U"])) if Q.shape[1] else 0.0
    out["U"] = 4.0 * max(e_ref["U"], U_RND * np.sqrt(c.n) * float(np.linalg.norm(ref["U"]))) + L["U"] * (out["Y"] + 4.0 * U_RND * np.sqrt(max(Q.shape[1], 1)) * vt)
    # the objective is a sum of |Omega| + m terms that cancel (1/2 sum A^2 against the rest): its rounding scales with the terms, not with the result
    terms = int(c.mask.sum()) + c.m
    out["objective"] = 4.0 * max(e_ref["objective"], U_RND * np.sqrt(terms) * (0.5 * float((c.A[c.mask] ** 2).sum()) + abs(ref["objective"]))) + L["objective"] * d
    return out, d


def compare(c, t, g, ref, e_ref, label):
    """prints the line of the run, then asserts; returns {array: error / bound}"""
    bd, d = bounds(c, t, ref, e_ref)
    err = {key: R.distance(g[key], ref[key]) for key in KEYS}
    ratio = {key: (err[key] / bd[key] if bd[key] > 0 else (0.0 if err[key] == 0 else np.inf)) for key in KEYS}
    print(label, "iters", g["iters"], "error / bound:", " ".join("%s %.2e/%.2e=%.3f" % (key, err[key], bd[key], ratio[key]) for key in KEYS), "| stop term d %.2e" % d)
    assert g["iters"] == t == ref["iters"], (label, g["iters"], ref["iters"])
    ident = np.abs(np.diag(g["Theta"]) - g["W"].sum(0))
    assert (ident <= np.maximum(1e-12, 4.0 * c.n * U_RND * np.abs(g["W"]).sum(0))).all(), (label, float(ident.max()))
    for key in KEYS:
        assert err[key] <= bd[key], (label, key, err[key], bd[key])
    return ratio


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_state_after_t_iterations(have_gpu, omc, run):
    name, t = run
    c = C.cases()[name]
    ref = C.reference(name, t); e_ref = C.e_ref(name, t)
    g, served = _gpu_state(omc, c, t)
    label = C.run_id(run)
    print(label, "iterations served by the tracked blocks (big cone, clip):", served)
    assert served == (0, 0), (label, served)      # every projection of these runs came from the full kernel
    compare(c, t, g, ref, e_ref, label)
    # the dual bound of the check at the cap, where the reference's is finite
    if np.isfinite(ref["dual_bound"]) and g["dual_bound"] > -1e299:
        kappa = R.sensitivity(c.inst, c.minors, c.soc, c.cuts, t, ref=ref, **c.params)
        d = stop_term(c, t, ref)      # the check's own eigenvalues come from k_cone_ws on a matrix that is not diagonal, at t = 1 too
        bd = 4.0 * max(e_ref["dual_bound"], U_RND * abs(ref["dual_bound"])) + kappa * d
        e = abs(g["dual_bound"] - ref["dual_bound"])
        print(label, "dual bound %.12g reference %.12g error / bound %.2e/%.2e=%.3f" % (g["dual_bound"], ref["dual_bound"], e, bd, e / bd))
        assert e <= bd, (label, g["dual_bound"], ref["dual_bound"], bd)
    elif np.isfinite(ref["dual_bound"]) != (g["dual_bound"] > -1e299):
        print(label, "dual bound: finiteness differs, engine", g["dual_bound"], "reference", ref["dual_bound"])
    if c.params:      # case C.  omc_last_solver_info reports the penalty the batch was staged with; a slot's bumped penalty shows in its state only
        print(label, "rho of omc_last_solver_info", g["rho"], "reference: start", C.sh.ShorParams().rho, "end", ref["rho"], "bumps", ref["n_bumps"])
        assert g["rho"] == C.sh.ShorParams().rho, (label, g["rho"])


def _same(a, b):
    for key in ("X", "W", "Theta", "Y", "U", "V"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    for key in ("objective", "dual_bound", "iters", "status_code"):
        assert a[key] == b[key], (key, a[key], b[key])


def test_batch_through_two_slots_equals_solo_runs(have_gpu, omc):
    """A's list, the empty list and D's 257 minors as one batch through two slots at t = 3 (the third node takes the slot of the first to
    finish, at an iteration that is no multiple of check_every): every node equals its solo run bit for bit, the batch repeats bit for
    bit, and every node holds the bound against the oracle."""
    D, lists = C.batch_lists()
    t = C.BATCH_T
    info = [(mi, None) for mi, _ in lists]
    out, _, _, _, _ = _solve(omc, D.A, D.mask, [[]] * 3, info, t, {}, slots=2)
    again, _, _, _, _ = _solve(omc, D.A, D.mask, [[]] * 3, info, t, {}, slots=2)
    for i, (mi, soc) in enumerate(lists):
        _same(out[i], again[i])
        solo, rp, rd, _, _ = _solve(omc, D.A, D.mask, [[]], [(mi, None)], t, {})
        _same(out[i], solo[0])
        ref = R.shor_state(D.inst, mi, soc, (), t)
        sp = R.perturbation_spread(D.inst, mi, soc, (), t, ref=ref); fl = R.representation_floor(ref)
        e_ref = {key: max(sp[key], fl[key]) for key in sp}
        cc = C.Case("batch-%d" % i, D.A, D.mask, mi, soc, (t,))
        V1, V2, V3 = _keyed(cc.structure, solo[0]["V"])
        g = dict(solo[0], V1=V1, V2=V2, V3=V3, rp=float(rp[0]), rd=float(rd[0]))
        compare(cc, t, g, ref, e_ref, "batch node %d (%d minors)" % (i, len(mi)))
