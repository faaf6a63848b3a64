"""The references of tests/test_plain_ops.py (oracle/omc_plain_ref.py) checked on their own, without a GPU: the long-double Rayleigh
eigenvalues against mpmath at 40 digits, the float64 restatement of the kernel's Jacobi (it converges in fewer than 30 sweeps on every
input the GPU module uses, its error in units of u ||M||_F grows no faster than the order), the objective reference against exact
rational arithmetic, the input builders against their own conditions in the high-precision values (so no vector comparison of the GPU
module is ever left out for want of a gap), the recorded error units of the large orders against the inputs they were recorded for, and
the mirror of the kernel's layout and dispatch arithmetic against the sources."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import omc_plain_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "optimalmatrixcompletion.jl_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "plain_ops_error_units.json")
LD = np.longdouble
SMALL_ORDERS = [N for N in R.SEP_ORDERS if N < R.RECORDED_FROM]


def test_long_double_is_wide():
    assert np.finfo(LD).eps < 1e-18


@pytest.mark.parametrize("N", [3, 16, 33])
def test_rayleigh_values_against_mpmath(N):
    """Bound: the quotient is N^2 long-double products summed in long double, (2 N + 4) eps_ld ||M||_F; the eigenvector error enters squared."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    for fam in ("a", "g", "c_two"):
        Y, U = R.sep_input(fam, N, 2, 900 + N)
        Ml = R.sep_matrix_ld(Y, U)
        lam, _ = R.rayleigh_eigvals(Ml)

        def mpf(x):
            hi = float(x)
            return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))

        A = mp.matrix(N, N)
        for i in range(N):
            for j in range(N):
                A[i, j] = mpf(Ml[i, j])
        ref = sorted(mp.eigsy(A, eigvals_only=True))
        err = max(abs(mpf(lam[i]) - ref[i]) for i in range(N))
        bound = (2 * N + 4) * float(np.finfo(LD).eps) * R.fro(Ml)
        print(f"N={N} {fam}: max |rayleigh - mpmath| = {float(err):.3e}, bound {bound:.3e}")
        assert err <= bound


def test_objective_reference_against_rationals():
    rng = np.random.default_rng(4)
    n, m, gamma = 5, 7, 80.0
    A = rng.standard_normal((n, m)) * 10.0 ** rng.uniform(-8, 8, (n, m))
    X = rng.standard_normal((n, m)) * 10.0 ** rng.uniform(-8, 8, (n, m))
    mask = rng.random((n, m)) < 0.5
    exact = Fraction(0)
    for i in range(n):
        for j in range(m):
            x = Fraction(float(X[i, j]))
            exact += x * x / (2 * Fraction(gamma))
            if mask[i, j]:
                exact += (x - Fraction(float(A[i, j]))) ** 2 / 2
    got = R.objective_ref(X, A, mask, gamma)
    hi = float(got)
    rel = abs(Fraction(hi) + Fraction(float(got - LD(hi))) - exact) / exact
    assert rel <= 4 * float(np.finfo(LD).eps)      # the products and (X - A) round once each in long double, the sums are exact


# ---- per-order measurements, shared --------------------------------------------------------------------------------------------------
_cache = {}


def _measured(key, build):
    if key not in _cache:
        M, Ml = build()
        lam, _ = R.rayleigh_eigvals(Ml)
        e, ej, el, sw = R.reference_error(M, lam)
        f = R.fro(M)
        _cache[key] = dict(lam=lam, e=e, ej=ej, el=el, sweeps=sw, fro=f)
    return _cache[key]


def _sep(N, fam, seed):
    def build():
        Y, U = R.sep_input(fam, N, min(R.SEP_K, N), seed)
        return R.sep_matrix(Y, U), R.sep_matrix_ld(Y, U)
    return build


def _rnd(N, k, fam, seed):
    def build():
        Y = R.round_input(fam, N, k, seed)
        return R.sym(Y), R.sym_ld(Y)
    return build


def _svd(n, m, fam, seed):
    def build():
        X = R.svd_input(fam, n, m, R.SEP_K, seed)
        return X @ X.T, R.gram_ld(X)
    return build


@pytest.mark.parametrize("N", SMALL_ORDERS)
def test_restatement_converges_on_every_small_input(N):
    """Fewer than 30 sweeps on every separation and rounding input below the recorded orders, and the restatement's own vectors are
    eigenvectors to the stop rule: || M v - lambda v || <= sqrt(N) tau 2.5 ||M||_F + 4 e_ref."""
    worst = 0
    for key, fam, seed in R.sep_cases(N):
        worst = max(worst, _measured(key, _sep(N, fam, seed))["sweeps"])
    for k in R.round_ranks(N):
        for key, fam, seed in R.round_cases(N, k):
            worst = max(worst, _measured(key, _rnd(N, k, fam, seed))["sweeps"])
    print(f"N={N}: most sweeps {worst}")
    assert worst < R.MAX_SWEEPS
    Y, U = R.sep_input("a", N, min(R.SEP_K, N), 100 * N)
    M = R.sep_matrix(Y, U)
    lam, V, _ = R.jacobi_restated(M)
    m0 = _measured("sep/%d/a" % N, _sep(N, "a", 100 * N))
    res = np.linalg.norm(M @ V - V * lam, axis=0).max()
    assert res <= math.sqrt(N) * R.TAU * 2.5 * m0["fro"] + 4 * m0["e"]
    assert np.abs(V.T @ V - np.eye(N)).max() <= 8 * R.U_RND * math.sqrt(N) + R.TAU


def test_restatement_converges_on_the_svd_inputs():
    worst = 0
    for n, m in R.SVD_SHAPES:
        if not R.svd_shape_accepted(n, m, R.SEP_K) or n >= R.RECORDED_FROM:
            continue
        for key, fam, seed in R.svd_cases(n, m, R.SEP_K):
            worst = max(worst, _measured(key, _svd(n, m, fam, seed))["sweeps"])
    assert worst < R.MAX_SWEEPS


def test_recorded_orders_converged_and_match_their_inputs():
    """tests/golden/plain_ops_error_units.json (tools/record_plain_ops_error_units.py): every case of the orders from 200 on is there, was
    recorded for the input the builder gives today (||M||_F to 1e-9 relative) and took fewer than 30 sweeps."""
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["u"] == R.U_RND
    cases = gold["cases"]
    want = {}
    for N in R.SEP_ORDERS:
        if N >= R.RECORDED_FROM:
            for key, fam, seed in R.sep_cases(N):
                want[key] = (seed, lambda N=N, fam=fam, seed=seed: R.sep_matrix(*R.sep_input(fam, N, R.SEP_K, seed)))
    for N in R.ROUND_ORDERS:
        if N >= R.RECORDED_FROM:
            for k in R.round_ranks(N):
                for key, fam, seed in R.round_cases(N, k):
                    want[key] = (seed, lambda N=N, k=k, fam=fam, seed=seed: R.sym(R.round_input(fam, N, k, seed)))
    for n, m in R.SVD_SHAPES:
        if n >= R.RECORDED_FROM and R.svd_shape_accepted(n, m, R.SEP_K):
            for key, fam, seed in R.svd_cases(n, m, R.SEP_K):
                want[key] = (seed, lambda n=n, m=m, fam=fam, seed=seed: (lambda X: X @ X.T)(R.svd_input(fam, n, m, R.SEP_K, seed)))
    assert sorted(want) == sorted(cases)
    for key, (seed, build) in want.items():
        rec = cases[key]
        assert rec["seed"] == seed and rec["sweeps"] < R.MAX_SWEEPS, key
        f = R.fro(build())
        assert abs(f - rec["fro"]) <= 1e-9 * max(f, rec["fro"]), key


def test_restatement_error_grows_no_faster_than_the_order():
    """The table of the restatement's error in units of u ||M||_F on U U' - B B'/N inputs (family g).  It grows with N -- the cancellation
    in norm - sigma -- which is why the GPU module's bounds are multiples of this measured error and not c u ||M||; as a check on the
    reference itself, from one order to the next it grows by no more than twice the ratio of the orders."""
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    rows = []
    for N in (17, 64, 130):
        key, fam, seed = R.sep_cases(N)[R.SEP_FAMILIES.index("g")]
        m = _measured(key, _sep(N, fam, seed))
        rows.append((N, m["ej"] / (R.U_RND * m["fro"]), m["el"] / (R.U_RND * m["fro"]), m["sweeps"]))
    for N in (200, 300):
        rec = cases["sep/%d/g" % N]
        rows.append((N, rec["units"], float("nan"), rec["sweeps"]))
    print("   N   restatement   LAPACK shifted   sweeps   (units of u ||M||_F; from 200 on the larger of the two, as recorded)")
    for r in rows:
        print("%4d   %11.1f   %14.1f   %6d" % r)
    for (n1, u1, _, _), (n2, u2, _, _) in zip(rows, rows[1:]):
        assert u2 <= 2.0 * (n2 / n1) * u1, (n1, u1, n2, u2)
    assert rows[0][1] >= 1.0      # and it is a measurable error, not zero


@pytest.mark.parametrize("N", R.SEP_ORDERS)
def test_builders_keep_their_conditions(N):
    """In the high-precision eigenvalues of the matrix the kernel is given (formed from the stored Y and U): the thresholds of (b) and (c)
    lie on the intended side with a margin of at least 0.4 of the threshold, the gap of (a) and of its scaled copies is at least 0.25 (times
    the scale), the double eigenvalue of (d) is double and separated, (e) is exactly zero, ||M||_F of (b) is at most 10."""
    k = min(R.SEP_K, N)
    lam = {}
    for key, fam, seed in R.sep_cases(N):
        if fam == "g":
            continue
        Y, U = R.sep_input(fam, N, k, seed)
        lam[fam] = (R.rayleigh_eigvals(R.sep_matrix_ld(Y, U))[0], R.fro(R.sep_matrix(Y, U)))
    assert lam["a"][0][1] - lam["a"][0][0] >= 0.25
    assert lam["f_small"][0][1] - lam["f_small"][0][0] >= 0.25e-12 and lam["f_big"][0][1] - lam["f_big"][0][0] >= 0.25e12
    assert lam["b_out"][0][0] <= 1.4 * R.FEAS_TOL and 0.6 * R.FEAS_TOL <= lam["b_in"][0][0] < 0.0
    assert lam["b_out"][1] <= 10.0 and lam["b_in"][1] <= 10.0
    if N > 1:
        assert lam["b_out"][0][1] >= -1.5e-7 and lam["b_in"][0][1] >= -1.5e-7
        for fam in ("c_two", "c_one"):
            assert abs(lam[fam][0][0] + 1e-3) <= 1e-9 and (N < 3 or lam[fam][0][2] >= 0.999e-3)
        assert lam["c_two"][0][1] <= 1.4 * R.TWO_TOL and 0.6 * R.TWO_TOL <= lam["c_one"][0][1] < 0.0
        assert abs(lam["d"][0][1] - lam["d"][0][0]) <= 1e-14 and (N < 3 or lam["d"][0][2] - lam["d"][0][1] >= 0.5)
    assert lam["e"][1] == 0.0
    # rounding: the k-th and (k+1)-th eigenvalues of 'top' are 0.5 apart, the top k at least 0.2 / 7 apart; the projector's are 1, 1, 1, 0, ..
    for kk in (R.round_ranks(N) if N in R.ROUND_ORDERS else []):
        w = np.asarray(R.rayleigh_eigvals(R.sym_ld(R.round_input("top", N, kk, R.round_cases(N, kk)[0][2])))[0], float)[::-1]
        if kk < N:
            assert w[kk - 1] - w[kk] >= 0.49
        if kk > 1:
            assert np.diff(w[:kk]).max() <= -0.028
    if N >= 3:
        w = np.asarray(R.rayleigh_eigvals(R.sym_ld(R.round_input("projector", N, 2, 5)))[0], float)[::-1]
        assert np.abs(w[:3] - 1.0).max() <= 1e-14 and np.abs(w[3:]).max(initial=0.0) <= 1e-14


def test_svd_builders_keep_the_singular_value_ratio():
    for n, m in R.SVD_SHAPES:
        if not R.svd_shape_accepted(n, m, R.SEP_K):
            continue
        for key, fam, seed in R.svd_cases(n, m, R.SEP_K):
            X = R.svd_input(fam, n, m, R.SEP_K, seed)
            sv = np.linalg.svd(X, compute_uv=False)
            if fam == "zero":
                assert not X.any()
            else:
                assert sv[R.SEP_K - 1] > 0.1 and (len(sv) == R.SEP_K or sv[R.SEP_K - 1] >= 2.0 * sv[R.SEP_K]), key
            if fam == "sparse" and n * m >= 64:
                assert (X == 0.0).mean() >= 0.1, key


def test_layout_and_dispatch_mirror_is_current():
    """The classes the GPU module claims to cover, from the arithmetic of csrc/omc_layout.h and eig_frontend mirrored in
    oracle/omc_plain_ref.py; the mirrored definitions must still stand verbatim in the sources, so a changed layout fails here."""
    assert R.layout_lines_missing(CSRC) == []
    assert R.cone_bytes(134) == 147416 and R.cone_bytes(134) <= R.OMC_MAX_DYN_LDS < R.cone_bytes(135)
    assert [N for N in R.SEP_ORDERS if not R.cone_in_lds(N)] == [135, 200, 255, 256, 257, 300]
    classes = {N: R.dispatch_class(N) for N in R.SEP_ORDERS}
    assert classes == {2: "wave16", 3: "wave16", 15: "wave16", 16: "wave16", 17: "t16", 18: "t16", 63: "t16", 64: "t16", 65: "t8", 66: "t8",
                       127: "t8", 128: "t8", 129: "generic4", 134: "generic4", 135: "generic4", 200: "generic4", 255: "generic4",
                       256: "generic4", 257: "generic2", 300: "generic2"}
    assert R.dispatch_class(514) == "generic1"      # above 512: one lane per pair, not covered (see SEP_ORDERS)
