"""k_colprox_block (csrc/omc_colprox_block.hip: one workgroup per column, blocked MFMA Cholesky) and omc_column_prox_batch: the column prox
on its own against numpy in both modes and every storage class, independence of slot and batch, the solver through the new path against
the path without it (OMC_COLPROX_BLOCK_MIN above every column) and the oracle, and the mixed dispatch pair / wide / block.

Bounds of the prox on its own, per column, from the reference's spectrum (u = 1.1e-16, lam_min = b_min + cp s, kappa = (b_max + cp s) /
lam_min): mode 0  ||alpha - ref|| / ||ref|| <= 16 c u kappa + 4 cp 1e-13 max(1, s) / lam_min  (forward error of two Cholesky solves with
backward error gamma_{3c+1}, a factor ~5 of room; the stop rule's ds carried through d alpha / ds) and |s - ref| <= 4e-13 max(1, ref);
mode 1  16 c u kappa on alpha and kappa times that on objcol and c0col.  Solver comparisons: the bounds
test_colprox_pair_kernel_against_one_column_kernel uses for "different arithmetic for the same prox" (objective rel 1e-9, dual bound
rel 1e-8 / abs 1e-8, Y atol 1e-9 at equal iteration counts) and the project's OBJ_REL = 2e-6 against the oracle."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GAMMA = 80.0
OBJ_REL = 2e-6
U_RND = 1.1e-16
COUNTS = [1, 15, 16, 17, 33, 64, 65, 80, 97, 112, 113, 128, 176, 177, 200, 208]


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


def _ref_column(Yb, a, al_old, gamma, rho_f, mode):
    """One column of oracle/omc_oracle.py:_prox_columns: eigh of B, 200 bisection steps on the secular function.  Returns alpha, s, b_min, b_max."""
    c = a.size
    if mode == 1:
        b, Q = np.linalg.eigh(np.eye(c) + gamma * Yb)
        return Q @ ((Q.T @ a) / b), 0.0, b[0], b[-1]
    cp = gamma * gamma / (2.0 * rho_f)
    b, Q = np.linalg.eigh(np.eye(c) + gamma * (Yb - gamma / (2.0 * rho_f) * np.outer(al_old, al_old)))
    qa2 = (Q.T @ a) ** 2
    phi = lambda s_: (qa2 / (b + cp * s_) ** 2).sum() - s_
    lo = max(0.0, -b[0] / cp) * (1.0 + 1e-12)
    hi = max(2.0 * lo + 1.0, 1.0)
    while phi(hi) > 0:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if phi(mid) > 0:
            lo = mid
        else:
            hi = mid
    s = 0.5 * (lo + hi)
    return Q @ ((Q.T @ a) / (b + cp * s)), s, b[0], b[-1]


@pytest.fixture(scope="module")
def prob():
    """The instance of T1 / T2 and its references, computed once."""
    n = m = 208; k = 2
    rng = np.random.default_rng(0)
    counts = np.array(COUNTS + [0] + list(rng.integers(5, 21, size=m - len(COUNTS) - 1)))
    mask = np.zeros((n, m), bool)
    for j, cj in enumerate(counts):
        mask[rng.choice(n, size=int(cj), replace=False), j] = True
    A = (rng.standard_normal((n, k)) @ rng.standard_normal((k, m)) + 0.05 * rng.standard_normal((n, m))) * mask
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.zeros(n); lam[:2] = (0.95, 0.8); lam[2:8] = np.geomspace(0.1, 1e-3, 6)
    Y = (Q * lam) @ Q.T; Y = 0.5 * (Y + Y.T)
    E = rng.standard_normal((n, n)); E = 0.5 * (E + E.T)
    Yp = Y + 1e-2 * E / np.linalg.norm(E, 2)
    Yx = 2.0 * Y - Yp
    rho_f = 0.1 * 4.0 * GAMMA / 2.0 * (A ** 2).sum() / (m * (1.0 + GAMMA * k / n) ** 2)
    cols = [np.nonzero(mask[:, j])[0] for j in range(m)]

    def reference(Yin, al_old, mode):
        al = np.zeros((n, m)); s = np.zeros(m); bmin = np.ones(m); bmax = np.ones(m)
        for j, idx in enumerate(cols):
            if idx.size:
                al[idx, j], s[j], bmin[j], bmax[j] = _ref_column(Yin[np.ix_(idx, idx)], A[idx, j], al_old[idx, j], GAMMA, rho_f, mode)
        return dict(alpha=al, s=s, bmin=bmin, bmax=bmax)

    r1 = reference(Yx, np.zeros((n, m)), 0)
    r2 = reference(Yx, r1["alpha"], 0)
    rx = reference(Y, np.zeros((n, m)), 1)
    return dict(n=n, m=m, k=k, A=A, mask=mask, Y=Y, Yx=Yx, rho_f=rho_f, cp=GAMMA ** 2 / (2.0 * rho_f), counts=counts, cols=cols, r1=r1, r2=r2, rx=rx)


def _errors(p, got, ref, mode):
    """Per non-empty column: (alpha error / bound, s error / bound) in mode 0, (alpha, objcol, c0col errors / bounds) in mode 1."""
    out = {}
    for j, idx in enumerate(p["cols"]):
        c = idx.size
        if c == 0:
            continue
        ar = ref["alpha"][idx, j]; ag = got["alpha"][0][idx, j]
        ea = np.linalg.norm(ag - ar) / np.linalg.norm(ar)
        if mode == 0:
            s = ref["s"][j]
            lmin = ref["bmin"][j] + p["cp"] * s
            kap = (ref["bmax"][j] + p["cp"] * s) / lmin
            ba = 16 * c * U_RND * kap + 4 * p["cp"] * 1e-13 * max(1.0, s) / lmin
            out[j] = (ea / ba, abs(got["s"][0][j] - s) / (4e-13 * max(1.0, s)))
        else:
            kap = ref["bmax"][j] / ref["bmin"][j]
            ba = 16 * c * U_RND * kap
            a = p["A"][idx, j]
            oc = 0.5 * a @ ar; c0 = a @ ar - 0.5 * ar @ ar
            out[j] = (ea / ba, abs(got["objcol"][0][j] - oc) / abs(oc) / (kap * ba), abs(got["c0col"][0][j] - c0) / abs(c0) / (kap * ba))
    return out


def test_prox_alone_against_numpy_every_storage_class(have_gpu, omc, prob):
    """T1.  Lengths 1, 15-17, 33, 64 / 65, whole tiles (80, 112, 128, 176), one past (113, 177), the LDS / slab boundary (176 / 177) and the
    longest (200, 208), then short columns.  Round 1: alpha_old = 0, cold s.  Round 2: alpha_old = the reference's round-1 alpha, which makes
    B indefinite at s = 0 for every listed length (b_min -3.2 .. -22: the failed-factorization branch runs), cold and from the round-1 s.  Mode 1 on the PSD Y.  algo 2 (block kernel
    everywhere) and algo 0 (the solver's dispatch) are held to the bounds of the module docstring; algo 1 (the path without the block kernel)
    is printed beside them.  algo 0 equals algo 2 bit for bit from 65 rows on and algo 1 bit for bit below."""
    p = prob
    assert p["rho_f"] == pytest.approx(202.2, rel=0.1) and list(p["counts"][:17]) == COUNTS + [0]
    eng = omc.Engine(p["A"], p["mask"], GAMMA, p["k"])
    rounds = [("mode0 round1", 0, p["Yx"], None, None, p["r1"]),
              ("mode0 round2 cold", 0, p["Yx"], p["r1"]["alpha"], None, p["r2"]),
              ("mode0 round2 warm", 0, p["Yx"], p["r1"]["alpha"], p["r1"]["s"][None], p["r2"]),
              ("mode1", 1, p["Y"], None, None, p["rx"])]
    bad = []
    for name, mode, Yin, ao, s0, ref in rounds:
        if mode == 0:
            assert (ref["bmin"][:len(COUNTS)] < 0).all() == (ao is not None)      # the listed columns: indefinite at s = 0 in round 2
        got = {al: eng.column_prox(Yin, alpha_old=None if ao is None else ao[None], rho_f=p["rho_f"], s0=s0, mode=mode, algo=al) for al in (0, 1, 2)}
        err = {al: _errors(p, got[al], ref, mode) for al in (0, 1, 2)}
        for j in sorted(err[2]):
            c = len(p["cols"][j])
            if j < len(COUNTS):
                print(f"{name} c={c:3d} block: " + " ".join(f"{x:.3f}" for x in err[2][j]) + f" nfact={got[2]['nfact'][0][j]}"
                      + " | without: " + " ".join(f"{x:.3f}" for x in err[1][j]) + f" nfact={got[1]['nfact'][0][j]}")
            for al in (0, 2):
                if not all(x <= 1.0 for x in err[al][j]):
                    bad.append((name, al, j, c, err[al][j]))
            assert 1 <= got[2]["nfact"][0][j] <= 61
            assert got[1]["nfact"][0][j] == -1 or 1 <= got[1]["nfact"][0][j] <= 61
            same = 2 if c >= 65 else 1
            keys = ("alpha", "s") if mode == 0 else ("alpha", "objcol", "c0col")
            for key in keys:
                x = got[0][key][0][..., j]; y = got[same][key][0][..., j]
                assert np.array_equal(x, y), (name, key, j, c)
        worst = {al: np.max([max(v) for v in err[al].values()]) for al in (0, 1, 2)}
        print(f"{name}: worst error / bound  dispatch {worst[0]:.3f}  without block {worst[1]:.3f}  block {worst[2]:.3f}")
        je = len(COUNTS)                                   # the empty column: no kernel counts it, mode 1 reports zero terms
        for al in (0, 1, 2):
            assert got[al]["nfact"][0][je] == -1
            if mode == 1:
                assert got[al]["objcol"][0][je] == 0.0 and got[al]["c0col"][0][je] == 0.0
    eng.close()
    assert not bad, bad


def test_prox_result_independent_of_slot_and_batch(have_gpu, omc, prob):
    """T2.  Three identical batch entries give three bit-identical results, equal to the one-entry call, and a second call repeats the first."""
    p = prob
    eng = omc.Engine(p["A"], p["mask"], GAMMA, p["k"])
    for mode, Yin, ao in ((0, p["Yx"], p["r1"]["alpha"]), (1, p["Y"], None)):
        keys = ("alpha", "s", "nfact") if mode == 0 else ("alpha", "objcol", "c0col")
        one = eng.column_prox(Yin, alpha_old=None if ao is None else ao[None], rho_f=p["rho_f"], mode=mode, algo=2)
        three = eng.column_prox(np.stack([Yin] * 3), alpha_old=None if ao is None else np.stack([ao] * 3), rho_f=p["rho_f"], mode=mode, algo=2)
        again = eng.column_prox(np.stack([Yin] * 3), alpha_old=None if ao is None else np.stack([ao] * 3), rho_f=p["rho_f"], mode=mode, algo=2)
        for key in keys:
            for b in range(3):
                assert np.array_equal(three[key][b], one[key][0]), (mode, key, b)
            assert np.array_equal(three[key], again[key]), (mode, key)
    eng.close()


def _env_run(eng, nodes, P, env):
    """One relaxation of `nodes` with the tuning knobs `env` set on the instance (the pattern of tests/test_gpu_parity.py)."""
    for k_, v in env.items():
        eng.tuning_set(k_, v)
    try:
        return eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False)
    finally:
        for k_ in env:
            eng.tuning_set(k_, None)


def _same_prox_other_arithmetic(a, b, iters):
    for x, y in zip(a, b):
        assert x["iters"] == y["iters"] == iters
        assert x["objective"] == pytest.approx(y["objective"], rel=1e-9) and x["dual_bound"] == pytest.approx(y["dual_bound"], rel=1e-8, abs=1e-8)
        assert np.allclose(x["Y"], y["Y"], atol=1e-9)


def _dense_instance(n, m, frac, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, m)) < frac
    mask[0, :] = True; mask[:, 0] = True
    A = (rng.standard_normal((n, 1)) @ rng.standard_normal((1, m)) + 0.01 * rng.standard_normal((n, m))) * mask
    return A, mask


@pytest.mark.parametrize("n,m,frac,lds", [(130, 132, 0.97, True), (200, 204, 0.95, False)])
def test_solver_through_block_kernel_against_path_without_it(have_gpu, omc, n, m, frac, lds):
    """T3.  A root and one depth-2 cut node at a fixed iteration count (300), default knob against OMC_COLPROX_BLOCK_MIN=100000; on the
    130 x 132 root also a run to the certificate against the oracle.
    Which depth-2 node: two arithmetics of one prox can only be compared on a node where 300 iterations of the ADMM map do not themselves blow
    round-off up to the bounds.  That was measured on the path WITHOUT the block kernel alone, as the change of its Y when A is multiplied by
    1 + 1e-13 N(0, 1) entrywise: 200 x 204 grandchildren 0 .. 3: 1.3e-7, 6.7e-15, 6.6e-15 (dual bound 1.0e-8), 2.9e-8; 130 x 132: below 1.1e-14
    on all four.  Grandchild 1 is the first that reproduces itself; the block kernel against the other path there: Y 1.1e-16, dual bound
    1.2e-11 (200 x 204), Y 1.1e-16, dual bound 1.1e-13 (130 x 132).  On grandchild 0 of 200 x 204 the two paths differ by 1.2e-7 in Y --
    what the perturbed input does to either path alone (1.3e-7, 1.5e-7) -- and agree to 7e-17 after 100 iterations, which the test asserts
    (grandchild 0 at 100 iterations, the same bounds): the divergence there comes from the iterations between 100 and 300, not from the prox."""
    A, mask = _dense_instance(n, m, frac, seed=5)
    cmax = int(mask.sum(0).max())
    plan = omc.pkg.api.colprox_plan(n, cmax)
    assert plan["block"] and (plan["slab_doubles"] == 0) == lds
    eng = omc.Engine(A, mask, GAMMA, 1)
    kids, _ = omc.pkg.bnb.expand_frontier(eng, 2, "linear", params=omc.default_params(rho_scale=4.0, max_iters=100))
    assert len(kids) == 4 and len(kids[1]) == 2
    nodes = [[], kids[1]]
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    a = _env_run(eng, nodes, P, {})
    b = _env_run(eng, nodes, P, {"OMC_COLPROX_BLOCK_MIN": "100000"})
    for x, y in zip(a, b):
        print(f"{n}x{m} cuts={len(nodes[a.index(x)])}: objective {x['objective']:.12e} / {y['objective']:.12e}  dual bound {x['dual_bound']:.12e} / {y['dual_bound']:.12e}")
    _same_prox_other_arithmetic(a, b, 300)
    P100 = omc.default_params(rho_scale=4.0, max_iters=100, eps_gap=1e-14)
    _same_prox_other_arithmetic(_env_run(eng, [kids[0]], P100, {}), _env_run(eng, [kids[0]], P100, {"OMC_COLPROX_BLOCK_MIN": "100000"}), 100)
    if lds:
        got = eng.matrix_completion_SDP_relaxation([[]], "linear", params=omc.default_params(rho_scale=4.0))[0]
        # orc.sdp_relaxation(orc.Instance(A, mask, GAMMA, 1), [], "linear", params=orc.RelaxParams(rho_scale=4.0)), minutes on a CPU: recorded by
        # tools/make_golden.py colprox, with the instance's checksums
        ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colprox_block_root_130x132.json")))
        assert ref["nnz"] == int(mask.sum()) and ref["sum_A"] == pytest.approx(float(A.sum()), rel=1e-12) and ref["rho_scale"] == 4.0
        assert got["status_code"] == 0 and ref["termination_status"] == 0
        assert got["objective"] == pytest.approx(ref["objective"], rel=OBJ_REL) and got["dual_bound"] == pytest.approx(ref["dual_bound"], rel=OBJ_REL)
    eng.close()


def test_mixed_dispatch_pair_wide_block(have_gpu, omc, orc):
    """T4.  40 x 45 with column densities 0.15 / 0.5 / 0.95, an empty column and odd m (the instance of
    test_colprox_pair_kernel_against_one_column_kernel) under OMC_COLPROX_BLOCK_MIN=33: pair, wide and block columns side by side.  The certified
    root against the oracle; the same knob without the pair kernel at a fixed iteration count."""
    rng = np.random.default_rng(11)
    n, m = 40, 45
    dens = rng.choice([0.15, 0.5, 0.95], size=m)
    mask = rng.random((n, m)) < dens[None, :]
    mask[:, 7] = False                                   # an empty column
    mask[0, :7] = True; mask[1, 8:] = True               # every row observed somewhere
    U0 = rng.standard_normal((n, 1)); V0 = rng.standard_normal((1, m))
    A = (U0 @ V0 + 0.01 * rng.standard_normal((n, m))) * mask
    cnt = mask.sum(0)
    paired = np.array([j + 1 - 2 * (j % 2) < m and cnt[j] <= 32 and cnt[j + 1 - 2 * (j % 2)] <= 32 for j in range(m)])
    assert (paired & (cnt > 0)).any() and (~paired & (cnt > 0) & (cnt <= 32)).any() and (cnt >= 33).any()      # pair, wide and block columns
    eng = omc.Engine(A, mask, GAMMA, 1)
    inst = orc.Instance(A, mask, GAMMA, 1)
    env = {"OMC_COLPROX_BLOCK_MIN": "33"}
    got = _env_run(eng, [[]], omc.default_params(rho_scale=4.0), env)[0]
    ref = orc.sdp_relaxation(inst, [], "linear", params=orc.RelaxParams(rho_scale=4.0))
    assert got["status_code"] == 0 and ref["termination_status"] == 0
    assert got["objective"] == pytest.approx(ref["objective"], rel=OBJ_REL) and got["dual_bound"] == pytest.approx(ref["dual_bound"], rel=OBJ_REL)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    a = _env_run(eng, [[]], P, env)
    b = _env_run(eng, [[]], P, dict(env, OMC_NO_COLPROX_PAIR="1"))
    _same_prox_other_arithmetic(a, b, 300)
    eng.close()
