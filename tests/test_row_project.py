"""The row projection of k_global on its own (omc_row_project_batch, Engine.row_project): the routines k_global runs (which = 1:
wave_nnqp_g, wave_cholesky_fwd_g, wave_chol_back_g in csrc/omc_wave.h) against the ones they were derived from (which = 0: wave_nnqp,
wave_cholesky, wave_chol_solve, which the alternating-minimisation kernels keep).  The derived routines change no operand, no order of a
sum and no tree of a reduction, so multipliers and overflow flag are equal -- np.array_equal, tolerance zero -- on every input, the rare
branches included, which no solve-level test reaches: the step towards the solve with compaction of the passive list, "drop the newest
index" after a failed factorisation, the overflow of the passive set.

Inputs, all seeded: G = A A' with A of R x 2R standard normals, c standard normal, R in {1, 2, 3, 17, 35, 64, 65, 70}; the warm start
taken four ways (zeros; the solution's support; the support and further rows; every row positive); the last two rows identical; R = 70
with 66 positive warm multipliers and a solution that is positive in every row.

Sanity, not the criterion: on the well-conditioned inputs the result meets the KKT conditions of min 1/2 l'Gl - c'l, l >= 0, computed in
numpy and scaled by max |c|: the largest of max(w, 0) over all rows and |w| over the rows with l > 0, w = c - G l.  which = 0 measured
2.535e-14 at most on these inputs (KKT_MEASURED; every figure is printed by the tests: 4.5e-15 at R = 2 to 2.5e-14 at R = 17, 2.4e-14 at
R = 64 -- the ridge of 1e-14 max diag that the passive system carries); the bound asserted for both is twice that, 5.07e-14 (KKT_BOUND)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDERS = (1, 2, 3, 17, 35, 64, 65, 70)
SEEDS = (0, 1, 2)
KKT_MEASURED = 2.535e-14      # which = 0 on the device: the largest over every input below (R = 17, warm start on the support)
KKT_BOUND = 2.0 * KKT_MEASURED      # 5.07e-14


@pytest.fixture(scope="module")
def eng(omc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, 8, 10, 40, seed=1)
    e = omc.Engine(A, mask, 80.0, 1)
    yield e
    e.close()


def _gram(R, seed):
    rng = np.random.default_rng(1000 * R + seed)
    A = rng.standard_normal((R, 2 * R))
    return A @ A.T, rng.standard_normal(R), rng


def _both(eng, G, c, lam0):
    a, ova = eng.row_project(G, c, lam0, which=0)
    b, ovb = eng.row_project(G, c, lam0, which=1)
    assert np.array_equal(ova, ovb), (ova, ovb)
    assert np.array_equal(a, b), np.argwhere(a != b)[:8]
    return a, ova


def _kkt(G, c, lam):
    w = c - np.einsum("brs,bs->br", G, lam)
    viol = np.maximum(np.maximum(w, 0.0).max(axis=1), np.where(lam > 0, np.abs(w), 0.0).max(axis=1))
    return float((viol / np.abs(c).max(axis=1)).max())


@pytest.fixture(scope="module")
def cold(eng):
    """The cold solves every warm start is derived from: R -> (G, c, lam) over the seeds, computed once and left unchanged."""
    out = {}
    for R in ORDERS:
        Gs, cs = zip(*[_gram(R, s)[:2] for s in SEEDS])
        G, c = np.stack(Gs), np.stack(cs)
        lam, ov = _both(eng, G, c, None)
        assert not ov.any() and (lam >= 0).all()
        out[R] = (G, c, lam)
    return out


@pytest.mark.parametrize("R", ORDERS)
def test_cold_and_kkt(eng, cold, R):
    G, c, lam = cold[R]
    v = _kkt(G, c, lam)
    print("R = %d: KKT violation / max|c| of which = 0 (= which = 1): %.3e" % (R, v))
    assert v <= KKT_BOUND


@pytest.mark.parametrize("R", ORDERS)
def test_warm_starts(eng, cold, R):
    G, c, sol = cold[R]
    sup = sol > 0
    rng = np.random.default_rng(77 + R)
    extra = sup | (rng.random(sup.shape) < 0.5)
    extra[:, R - 1] = True
    warm = dict(support=np.where(sup, 1.0, 0.0), support_values=sol.copy(), support_and_more=np.where(extra, 0.5 + rng.random(sup.shape), 0.0),
                all_rows=np.full(sup.shape, 1.0), with_negative=np.where(extra, 1.0, -1.0))
    for name, lam0 in warm.items():
        lam, ov = _both(eng, G, c, lam0)
        assert (lam >= 0).all() and (R > 64 or not ov.any()), name
        if R <= 64:      # above 64 rows a warm start may fill the passive set; the flag then says so
            v = _kkt(G, c, lam)
            print("R = %d, warm start %s: KKT violation / max|c| %.3e" % (R, name, v))
            assert v <= KKT_BOUND, name
    # support_and_more, all_rows: a warm row outside the support has no positive multiplier in the solve over the warm set (G is positive
    # definite, the minimiser unique), so the step towards the solve and the compaction of the list run before the support is reached
    if R <= 64:
        assert (extra & ~sup).any() or sup.all()


def _identical_rows(R, seed, lower):
    """The last two rows identical (G's last two rows and columns equal bit for bit); `lower` ridge units (1e-14 max diag) taken off the
    last diagonal entry on top, which puts the last pivot of the warm factorisation below zero whatever the rounding does."""
    rng = np.random.default_rng(5000 + 10 * R + seed)
    A = rng.standard_normal((R, 2 * R))
    A[R - 1] = A[R - 2]
    G = A @ A.T
    G[R - 1, :] = G[R - 2, :]; G[:, R - 1] = G[:, R - 2]; G[R - 1, R - 1] = G[R - 2, R - 2]
    G[R - 1, R - 1] -= lower * 1e-14 * G.diagonal().max()
    c = rng.standard_normal(R)
    c[R - 1] = c[R - 2] = abs(c[R - 2]) + 1.0
    return G, c


@pytest.mark.parametrize("R", (2, 3, 17, 64))
def test_identical_rows_drop_the_newest_index(eng, R):
    """Warm start on every row, so the duplicate is the newest index of the list.  Where the factorisation fails at it, the row leaves the
    list with its warm multiplier untouched -- a solve would have overwritten it, a step scaled it: that value in which = 0's output says
    the branch ran.  Exactly identical rows leave it to the rounding; with four ridge units off the diagonal it must run."""
    cases = [_identical_rows(R, s, lower) for lower in (0.0, 4.0) for s in range(4)]
    G, c = np.stack([g for g, _ in cases]), np.stack([v for _, v in cases])
    lam0 = np.full(c.shape, 1.0); lam0[:, R - 1] = 0.8125
    lam, ov = _both(eng, G, c, lam0)
    ran = lam[:, R - 1] == 0.8125
    print("R = %d: drop-the-newest ran on %s (exact duplicates: first four)" % (R, ran.astype(int).tolist()))
    assert ran[4:].all()
    cold_lam, _ = _both(eng, G, c, None)
    assert (cold_lam >= 0).all()


def test_overflow_of_the_passive_set(eng):
    R = 70
    Gs, cs, l0 = [], [], []
    for s in SEEDS:
        G, _, rng = _gram(R, s)
        Gs.append(G); cs.append(G @ (1.0 + rng.random(R)))      # the minimiser is positive in every row: 70 > 64 passive rows
        w = np.zeros(R); w[rng.permutation(R)[:66]] = 0.5 + rng.random(66); l0.append(w)
    G, c, lam0 = np.stack(Gs), np.stack(cs), np.stack(l0)
    lam, ov = _both(eng, G, c, lam0)
    assert (ov == 1).all() and ((lam > 0).sum(axis=1) <= 64).all()
    lam, ov = _both(eng, G, c, None)
    assert (ov == 1).all()
