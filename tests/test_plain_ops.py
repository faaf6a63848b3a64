"""The plain device operations the branch-and-bound drivers call around the relaxation -- omc_separation_batch, omc_round_Y_batch,
omc_left_singular_batch, omc_evaluate_objective -- against the references of oracle/omc_plain_ref.py, at every order at which the cold
eigen-kernel k_cone (modes CONE_SEP, CONE_TOPK) takes another path: the sweep inside one wave (order up to 16), jacobi_sweeps_t<16> and
<8>, the generic sweep with 4, 2 and 1 lanes per pair, the matrix in LDS (up to order 134) and on the global slab (from 135); and at the
edges of the Gram product under omc_left_singular_batch (fewer than 16 columns, a remainder of 1 - 3 columns, partial 16-row tiles).
Order 514 (above 512 the generic sweep has one lane per pair) is left out: a one-matrix separation call took 2.05 s there, the 20 calls of
the families under both rules 41 s; that sweep stays uncompared in these two modes.

Bounds (u = 1.1e-16, tau = 1e-14 the kernel's rotation threshold).  Per input, e_ref is the larger error, against long-double eigenvalues
of the same input, of a float64 restatement of the kernel's algorithm and of LAPACK on the shifted matrix; it is computed here below
order 200 and read from tests/golden/plain_ops_error_units.json (tools/record_plain_ops_error_units.py) from there on.
  eigenvalues   |lambda - lambda_ref| <= 4 e_ref   (the 4 covers another summation order: DPP group sums, fma contraction, pair order)
  vectors       | ||x|| - 1 | <= 8 u sqrt(N);   residual ||M x - lambda x|| <= rb = (sqrt(N) tau + 4 e_ref / ||M||_F) 2.5 ||M||_F
                (what the stop rule leaves, and the eigenvalue's own error; 2.5 ||M||_F bounds ||M + sigma I||_2)
  with a gap    ||x - x_ref|| <= 2 rb / gap after the canonical sign (up to sign where the two largest |entries| of x_ref tie to 1e-6)
  eigenspaces   ||(I - P P') x|| <= 2 rb / (gap to the rest of the spectrum)
  weighted x    (smallest_2_eigvec, lambda_2 < -1e-10)  w1 2 rb / gap_1 + w2 2 rb / gap_2 + 16 e_ref / ||(l1, l2)|| (the weights' own
                error), and | ||x|| - 1 | <= 8 u sqrt(N) + tau (two columns the sweep left orthogonal to tau)
  U' U = I      rounding: to 8 u sqrt(N) k.  Left singular vectors: the diagonal to that, the off-diagonal to that + tau -- the sweep stops
                with every pair of columns orthogonal to tau = 1e-14 relative and no better (measured: 0.87 tau at (15, 20)), so nothing
                tighter follows from the algorithm; the rounding inputs stay below 0.3 of the tighter bound.
                U U' against the reference projector to 2 sqrt(k) rb / gap + k times the U' U bound (Davis-Kahan per column)
  objective     relative (ceil(n m / 256) + 16) u: every term is non-negative; a thread's serial partial sum, then the block reduction
The exact zero matrix (Y = U U' on coordinate vectors, Y = 0, X = 0): eigenvalues 0 to 1e-290, feasible, finite unit x, finite
orthonormal U.  Negative and zero batch counts: OMC_ERR_ARGUMENT from all four entry points, and the handle goes on working.

Instances need n <= m (OMC.jl:249-254), so the eigen tests use m = n, the shapes (255, 1), (135, 40), (300, 7) and every (n, m) of the
Gram grid with m < n are asserted refused (OMC_ERR_DIMENSION) -- (135, 135) and (300, 303) stand in for the slab and the large Gram
product -- and a one-column X (m = 1) cannot be reached through the interface except at n = 1, which is left out.

Measured on an MI355X, worst error over bound per dispatch class: MEASURED below (every run prints its own figures, one line per order)."""
import ctypes as C
import json
import math
import os
import time

import numpy as np
import pytest

import omc_plain_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "optimalmatrixcompletion.jl_amd", "csrc")
GAMMA = 80.0
U = R.U_RND
LD = np.longdouble
ERR_DIMENSION, ERR_ARGUMENT = -2, -3
MEASURED = """
worst over the orders of each dispatch class, product library, MI355X:
  sweep                      orders               matrix  eigenvalue error / e_ref  residual / rb  vector / (2 rb / gap)  U'U - I / bound
  jacobi_sweeps_wave16       2, 3, 15, 16         LDS     2.38   (bound 4)           0.083          0.041                  0.52
  jacobi_sweeps_t<16>        17, 18, 33, 63, 64   LDS     1.24                       0.080          0.027                  0.30
  jacobi_sweeps_t<8>         65, 66, 127, 128     LDS     1.41                       0.075          0.012                  0.22
  generic, 4 lanes per pair  129, 134             LDS     1.14                       0.059          0.017                  0.21
  generic, 4 lanes per pair  135, 200, 255, 256   slab    1.16                       0.069          0.028                  0.13
  generic, 2 lanes per pair  257, 300             slab    1.12                       0.064          0.026                  0.19
  largest cosine between two returned columns: 0.90 tau (rounding, order 134, k = 8), 0.87 tau (left singular vectors, (15, 20))
  objective scan: 2.95 u at worst, 0.17 of its bound
With the rotation threshold of these modes at 1e-7 instead of 1e-14, 63 of the 133 cases fail; with the second-smallest eigenvalue of
CONE_SEP not tracked, 20 (every order of test_separation); with the last m mod 4 columns of the Gram product dropped, the 23 shapes of
test_left_singular_vectors_and_gram_product with m mod 4 != 0."""


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(HERE, "golden", "plain_ops_error_units.json")) as f:
        return json.load(f)["cases"]


def _engine(omc, n, m, k):
    """An instance for the operations that read only (n, m, k): one observed entry per column."""
    A = np.zeros((n, m)); mask = np.zeros((n, m), bool)
    mask[np.arange(m) % n, np.arange(m)] = True; A[mask] = 1.0
    return omc.Engine(A, mask, GAMMA, k)


_refs = {}


def _ref(gold, key, order, M, M_ld):
    """Reference of one input, computed once: long-double eigenvalues (ascending), LAPACK's vectors, e_ref, ||M||_F."""
    if key not in _refs:
        lam, V = R.rayleigh_eigvals(M_ld() if callable(M_ld) else M_ld)
        f = R.fro(M)
        if order >= R.RECORDED_FROM:
            rec = gold[key]
            assert abs(f - rec["fro"]) <= 1e-9 * max(f, rec["fro"]), "%s: the recorded error units belong to another input" % key
            e = rec["units"] * U * f
        else:
            e = R.reference_error(M, lam)[0]
        _refs[key] = dict(lam=lam, V=V, e=e, fro=f, M=M)
    return _refs[key]


def _ratio(err, ref):
    err = float(err)
    return 0.0 if err == 0.0 else (err / ref if ref > 0.0 else float("inf"))


def _rb(N, ref):
    return (math.sqrt(N) * R.TAU + 4.0 * ref["e"] / ref["fro"]) * 2.5 * ref["fro"]


def _dist_after_sign(x, xr):
    return float(np.linalg.norm(x - xr)) if R.sign_is_decided(xr) else float(min(np.linalg.norm(x - xr), np.linalg.norm(x + xr)))


def _report(op, N, stats):
    print("plain_ops %s N=%d class=%s %s  " % (op, N, R.dispatch_class(N), "lds" if R.cone_in_lds(N) else "slab")
          + "  ".join("%s=%.3g" % kv for kv in sorted(stats.items())))


def _bump(stats, name, v):
    stats[name] = max(stats.get(name, 0.0), v)


def test_coverage_claim_from_the_layout():
    """Which orders are LDS and which slab, and the sweep each takes, from the arithmetic of csrc/omc_layout.h and eig_frontend mirrored in
    oracle/omc_plain_ref.py; the mirrored lines must stand verbatim in the sources, so the claim fails rather than goes stale."""
    assert R.layout_lines_missing(CSRC) == []
    assert R.cone_bytes(134) <= R.OMC_MAX_DYN_LDS < R.cone_bytes(135)
    assert [N for N in R.SEP_ORDERS if R.cone_in_lds(N)] == [2, 3, 15, 16, 17, 18, 63, 64, 65, 66, 127, 128, 129, 134]
    assert {R.dispatch_class(N) for N in R.SEP_ORDERS if R.cone_in_lds(N)} == {"wave16", "t16", "t8", "generic4"}
    assert {R.dispatch_class(N) for N in R.SEP_ORDERS if not R.cone_in_lds(N)} == {"generic4", "generic2"}
    assert {R.dispatch_class(N) for N in R.ROUND_ORDERS} == {"wave16", "t16", "t8", "generic4", "generic2"}


# ---- 1. separation ------------------------------------------------------------------------------------------------------------------------
def _check_sep(N, fam, rule, ref, ev, x, fe, stats):
    sq = math.sqrt(N)
    assert np.isfinite(ev).all() and np.isfinite(x).all(), fam
    if fam == "e":
        assert np.abs(ev).max() <= 1e-290 and fe, (fam, ev, fe)
        assert abs(np.linalg.norm(x) - 1.0) <= 8 * U * sq, fam
        return
    lam, V, e, M = ref["lam"], ref["V"], ref["e"], ref["M"]
    tol, rb = 4.0 * e, _rb(N, ref)
    d = [abs(LD(ev[0]) - lam[0]), abs(LD(ev[1]) - lam[1])]
    _bump(stats, "eig", max(_ratio(d[0], e), _ratio(d[1], e)))
    assert d[0] <= tol and d[1] <= tol, (fam, rule, [float(v) for v in d], tol)
    l1, l2 = float(lam[0]), float(lam[1])
    assert abs(l1 - R.FEAS_TOL) > tol, "builder: lambda_1 sits on the feasibility threshold"
    assert bool(fe) == (l1 >= R.FEAS_TOL), (fam, l1, fe)
    if fam == "b_out":
        assert not fe
    if fam == "b_in":
        assert fe
    two = rule == "smallest_2_eigvec" and l2 < R.TWO_TOL
    if rule == "smallest_2_eigvec":
        assert abs(l2 - R.TWO_TOL) > tol, "builder: lambda_2 sits on the switch of smallest_2_eigvec"
        if fam in ("c_two", "c_one"):
            assert two == (fam == "c_two")
    gap1 = l2 - l1
    gap_rest = float(lam[2]) - l2 if N > 2 else float("inf")
    nx = abs(np.linalg.norm(x) - 1.0)
    if fam == "d":                                   # double smallest eigenvalue: x lies in its eigenspace, whatever the rule
        assert nx <= 8 * U * sq + (R.TAU if two else 0.0), (fam, rule, nx)
        P = V[:, :2]
        out = float(np.linalg.norm(x - P @ (P.T @ x)))
        if N > 2:                                    # at N = 2 the eigenspace is the whole space
            _bump(stats, "space", _ratio(out, 2.0 * rb / gap_rest))
            assert out <= 2.0 * rb / gap_rest, (fam, rule, out, rb, gap_rest)
        return
    if not two:
        _bump(stats, "norm", nx / (8 * U * sq))
        assert nx <= 8 * U * sq, (fam, rule, nx)
        res = float(np.linalg.norm(M @ x - ev[0] * x))
        _bump(stats, "res", res / rb)
        assert res <= rb, (fam, rule, res, rb)
        if fam[0] in "acfg":
            dv = _dist_after_sign(x, R.canon(V[:, 0]))
            _bump(stats, "vec", _ratio(dv, 2.0 * rb / gap1))
            assert dv <= 2.0 * rb / gap1, (fam, rule, dv, rb, gap1)
        return
    # the weighted combination (OMC.jl:2471-2473) of the two canonical eigenvectors
    assert nx <= 8 * U * sq + R.TAU, (fam, rule, nx)
    nn = math.hypot(l1, l2)
    w1, w2 = abs(l1) / nn, abs(l2) / nn
    v1, v2 = R.canon(V[:, 0]), R.canon(V[:, 1])
    gap2 = min(gap1, gap_rest)
    bound = w1 * 2.0 * rb / gap1 + w2 * 2.0 * rb / gap2 + 16.0 * e / nn
    s1s = (1.0,) if R.sign_is_decided(v1) else (1.0, -1.0)
    s2s = (1.0,) if R.sign_is_decided(v2) else (1.0, -1.0)
    dv = min(float(np.linalg.norm(x - (a * w1 * v1 + b * w2 * v2))) for a in s1s for b in s2s)
    _bump(stats, "vec2", _ratio(dv, bound))
    assert dv <= bound, (fam, rule, dv, bound)


@pytest.mark.parametrize("N", R.SEP_ORDERS)
def test_separation(have_gpu, omc, gold, N):
    """All families (a)-(g) at order N under both breakpoint rules, one batch per rule."""
    k = min(R.SEP_K, N)
    cases = R.sep_cases(N)
    ins = [R.sep_input(fam, N, k, seed) for _, fam, seed in cases]
    refs = [None if fam == "e" else _ref(gold, key, N, R.sep_matrix(Y, Uu), lambda Y=Y, Uu=Uu: R.sep_matrix_ld(Y, Uu))
            for (key, fam, _), (Y, Uu) in zip(cases, ins)]
    eng = _engine(omc, N, N, k)
    stats = {}
    for rule in ("smallest_1_eigvec", "smallest_2_eigvec"):
        t0 = time.perf_counter()
        x, ev, fe = eng.breakpoint_vectors([Y for Y, _ in ins], [Uu for _, Uu in ins], rule)
        stats["seconds_" + rule[9]] = time.perf_counter() - t0
        for b, (key, fam, _) in enumerate(cases):
            _check_sep(N, fam, rule, refs[b], ev[b], x[b], fe[b], stats)
    eng.close()
    _report("sep", N, stats)


# ---- 2. rounding and 3. left singular vectors: the k dominant eigenvectors ---------------------------------------------------------------
def _check_topk(N, k, fam, ref, lam_desc, Vd, Ug, stats, what, off=0.0):
    """Ug (N x k) against the eigenvectors Vd (columns, eigenvalues lam_desc descending) of ref['M'].  off: what the off-diagonal of U' U is
    allowed beyond 8 u sqrt(N) k."""
    sq = math.sqrt(N)
    orth = 8 * U * sq * k
    assert np.isfinite(Ug).all(), what
    E = Ug.T @ Ug - np.eye(k)
    dev, devo = float(np.abs(np.diag(E)).max()), float(np.abs(E - np.diag(np.diag(E))).max())
    _bump(stats, "orth", max(dev / orth, devo / (orth + off)))
    _bump(stats, "cos", devo / R.TAU)
    assert dev <= orth and devo <= orth + off, (what, dev, devo, orth, off)
    if fam == "zero":
        return
    M, rb = ref["M"], _rb(N, ref)
    res = max(float(np.linalg.norm(M @ Ug[:, j] - (Ug[:, j] @ M @ Ug[:, j]) * Ug[:, j])) for j in range(k))
    _bump(stats, "res", res / rb)
    assert res <= rb, (what, res, rb)
    if fam == "projector":                           # eigenvalue 1 three times: the answer is a subspace of that eigenspace
        r = min(3, N)
        P = Vd[:, :r]
        gap = float(lam_desc[r - 1] - lam_desc[r]) if N > r else float("inf")
        out = float(np.linalg.norm(Ug - P @ (P.T @ Ug)))
        if N > r:                                    # at N <= 3 the eigenspace is the whole space
            _bump(stats, "space", _ratio(out, 2.0 * math.sqrt(k) * rb / gap))
            assert out <= 2.0 * math.sqrt(k) * rb / gap, (what, out, rb, gap)
        return
    P = Vd[:, :k]
    gap = float(lam_desc[k - 1] - lam_desc[k]) if k < N else float("inf")
    dp = float(np.linalg.norm(Ug @ Ug.T - P @ P.T))
    bound = 2.0 * math.sqrt(k) * rb / gap + k * (orth + off)
    _bump(stats, "proj", dp / bound)
    assert dp <= bound, (what, dp, bound)
    for j in range(k):                               # entry-wise after the sign rule: the top k are separated by construction
        gj = min(float(lam_desc[j - 1] - lam_desc[j]) if j > 0 else float("inf"), float(lam_desc[j] - lam_desc[j + 1]) if j + 1 < N else float("inf"))
        dv = _dist_after_sign(Ug[:, j], R.canon(Vd[:, j]))
        _bump(stats, "vec", _ratio(dv, 2.0 * rb / gj))
        assert dv <= 2.0 * rb / gj, (what, j, dv, rb, gj)


@pytest.mark.parametrize("N", R.ROUND_ORDERS)
def test_rounding(have_gpu, omc, gold, N):
    """omc_round_Y_batch at order N: k = 1, 2 (k = n at n = 2), k = 8 at the orders beside the wave and the LDS thresholds."""
    stats = {}
    for k in R.round_ranks(N):
        cases = R.round_cases(N, k)
        Ys = [R.round_input(fam, N, k, seed) for _, fam, seed in cases]
        eng = _engine(omc, N, N, k)
        got = eng.round_Y(Ys)
        eng.close()
        for (key, fam, _), Y, Ug in zip(cases, Ys, got):
            if fam == "zero":
                _check_topk(N, k, fam, None, None, None, Ug, stats, key)
                continue
            ref = _ref(gold, key, N, R.sym(Y), lambda Y=Y: R.sym_ld(Y))
            _check_topk(N, k, fam, ref, np.asarray(ref["lam"], float)[::-1], ref["V"][:, ::-1], Ug, stats, key)
    _report("round", N, stats)


@pytest.mark.parametrize("n,m", R.SVD_SHAPES)
def test_left_singular_vectors_and_gram_product(have_gpu, omc, gold, n, m):
    """omc_left_singular_batch at (n, m), k = 2, against numpy's SVD of X itself; the bound is the eigenvector bound on G = X X' with
    ||G||_F and the gaps of the squared singular values."""
    k = R.SEP_K
    if not R.svd_shape_accepted(n, m, k):
        with pytest.raises(omc.OmcError) as err:
            _engine(omc, n, m, k)
        assert err.value.code == ERR_DIMENSION
        return
    cases = R.svd_cases(n, m, k)
    Xs = [R.svd_input(fam, n, m, k, seed) for _, fam, seed in cases]
    eng = _engine(omc, n, m, k)
    got = eng.left_singular(Xs)
    eng.close()
    stats = {}
    for (key, fam, _), X, Ug in zip(cases, Xs, got):
        if fam == "zero":
            _check_topk(n, k, fam, None, None, None, Ug, stats, key, R.TAU)
            continue
        ref = _ref(gold, key, n, X @ X.T, lambda X=X: R.gram_ld(X))
        Uf, sv, _ = np.linalg.svd(X, full_matrices=True)
        s2 = np.zeros(n); s2[: sv.size] = sv ** 2
        _check_topk(n, k, fam, ref, s2, Uf, Ug, stats, key, R.TAU)
    _report("svd m=%d" % m, n, stats)


# ---- 4. objective scan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["empty", "full", "random"])
@pytest.mark.parametrize("n,m", [(2, 2), (3, 5), (15, 17), (16, 16), (255, 1), (1, 257), (37, 53), (300, 300)])
def test_objective_scan(have_gpu, omc, n, m, mask_kind):
    """B = 1 and B = 33 matrices of entries between 1e-8 and 1e+8 in magnitude against math.fsum over long-double products."""
    rng = np.random.default_rng(1000 * n + m)
    mixed = lambda shape: rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-8.0, 8.0, shape)
    A = mixed((n, m))
    mask = {"empty": np.zeros((n, m), bool), "full": np.ones((n, m), bool), "random": rng.random((n, m)) < 0.4}[mask_kind]
    if n > m:
        with pytest.raises(omc.OmcError) as err:
            omc.Engine(A, mask, GAMMA, 1)
        assert err.value.code == ERR_DIMENSION       # OMC.jl:249-254
        return
    eng = omc.Engine(A, mask, GAMMA, 1)
    bound = (math.ceil(n * m / 256) + 16) * U
    worst = 0.0
    for B in (1, 33):
        Xs = mixed((B, n, m))
        got = eng.evaluate_objective(Xs)
        for b in range(B):
            ref = R.objective_ref(Xs[b], A, mask, GAMMA)
            rel = float(abs(LD(got[b]) - ref) / ref)
            worst = max(worst, rel)
            assert rel <= bound, (B, b, got[b], float(ref), rel, bound)
    eng.close()
    print("plain_ops objective (%d, %d) %s: worst relative error %.3g u, bound %.0f u" % (n, m, mask_kind, worst / U, bound / U))


# ---- 5. independence of batch and slot -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [17, 135])
def test_batch_and_slot_independence(have_gpu, omc, N):
    """Matrix i of a batch of 5 different matrices equals its one-matrix call bit for bit, and a repeated call repeats (LDS and slab)."""
    k = R.SEP_K
    eng = _engine(omc, N, N + 3, k)
    ins = [R.sep_input(f, N, k, 77 + i) for i, f in enumerate(["a", "g", "b_in", "d", "c_two"])]
    Ys, Us = [Y for Y, _ in ins], [Uu for _, Uu in ins]
    for rule in ("smallest_1_eigvec", "smallest_2_eigvec"):
        x, ev, fe = eng.breakpoint_vectors(Ys, Us, rule)
        x2, ev2, fe2 = eng.breakpoint_vectors(Ys, Us, rule)
        assert np.array_equal(x, x2) and np.array_equal(ev, ev2) and np.array_equal(fe, fe2)
        for i in range(5):
            x1, ev1, fe1 = eng.breakpoint_vectors([Ys[i]], [Us[i]], rule)
            assert np.array_equal(x1[0], x[i]) and np.array_equal(ev1[0], ev[i]) and fe1[0] == fe[i]
    Yr = [R.round_input(f, N, k, 90 + i) for i, f in enumerate(["top", "projector", "top_small", "top_big", "top"])]
    got = eng.round_Y(Yr); again = eng.round_Y(Yr)
    for i in range(5):
        assert np.array_equal(got[i], again[i]) and np.array_equal(eng.round_Y([Yr[i]])[0], got[i])
    Xs = [R.svd_input(f, N, N + 3, k, 60 + i) for i, f in enumerate(["product", "sparse", "product", "sparse", "product"])]
    got = eng.left_singular(Xs); again = eng.left_singular(Xs)
    for i in range(5):
        assert np.array_equal(got[i], again[i]) and np.array_equal(eng.left_singular([Xs[i]])[0], got[i])
    eng.close()


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors(have_gpu, omc):
    """B = 0 and B = -1 on the four entry points: OMC_ERR_ARGUMENT, nothing thrown through the C interface, and the handle still works;
    the enum and dimension errors as before."""
    n, m, k = 12, 14, 2
    eng = _engine(omc, n, m, k)
    lib = omc.load()
    Y, Uu = R.sep_input("a", n, k, 5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    Yb = np.ascontiguousarray(Y.ravel(order="F")); Ub = np.ascontiguousarray(Uu.ravel(order="F")); Xb = np.zeros(n * m)
    ev = np.zeros(2); x = np.zeros(n); fe = np.zeros(1, np.int32); Uo = np.zeros(n * k); obj = np.zeros(1)
    before = eng.breakpoint_vectors([Y], [Uu])
    for B in (0, -1):
        assert lib.omc_separation_batch(eng._h, B, 1, p(Yb), p(Ub), p(ev), p(x), p(fe)) == ERR_ARGUMENT
        assert lib.omc_round_Y_batch(eng._h, B, p(Yb), p(Uo)) == ERR_ARGUMENT
        assert lib.omc_left_singular_batch(eng._h, B, p(Xb), p(Uo)) == ERR_ARGUMENT
        assert lib.omc_evaluate_objective(eng._h, B, p(Xb), p(obj)) == ERR_ARGUMENT
    after = eng.breakpoint_vectors([Y], [Uu])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert len(eng.round_Y([Y])) == 1 and len(eng.left_singular([np.ones((n, m))])) == 1 and np.isfinite(eng.evaluate_objective(np.ones((n, m))))
    with pytest.raises(ValueError):
        eng.breakpoint_vectors([Y], [Uu], "largest_eigvec")                 # OMC.jl:2440-2446
    assert lib.omc_separation_batch(eng._h, 1, 7, p(Yb), p(Ub), p(ev), p(x), p(fe)) == -1      # OMC_ERR_INVALID_ENUM
    with pytest.raises(ValueError):
        eng.evaluate_objective(np.zeros((n, m + 1)))                        # OMC.jl:2337-2348
    with pytest.raises(ValueError):
        eng.left_singular([np.zeros((n + 1, m))])
    eng.close()
