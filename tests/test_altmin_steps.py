"""One V-step and one U-step of alternating_minimization (k_altmin, k_altmin_k, k_altmin_w) against the references of
oracle/omc_altmin_ref.py, which share no algorithm with the kernels: every call is alternating_minimization(..., max_iters = 1), whose V
is the V-step of the start, whose U is the U-step for that V and whose objectives[0] is model_U's value.  Run on the MI355X box:
`pytest -m gpu`.  Cases: tests/altmin_step_cases.py (ranks 1 - 8 with all three cut types, own masks with empty / full / one-entry rows
and columns, start scales 0.3, 1, 3, no / one / two cuts; the stride and lane-group edges 255 - 257 rows, 31 - 33 rows, n = k, k + 1).

Bounds (u = 1.1e-16; e_ref is always the error of float64 restatements against the long-double value of the same input):
  V           per column ||v - v_ref|| <= 4 max(e_ref, k u ||v_ref||); e_ref is the largest error of np.linalg.solve and of the unpivoted
              Gauss-Jordan restatement on the normal equations summed by numpy, entry after entry, in the opposite order, and entry after
              entry with fused multiply-adds (which order a correct implementation sums in is its own business; with numpy's order
              alone the rank-1 shapes with 51-entry columns missed the bound by up to 2.2 times)
  U           ||U - U_ref||_F <= 4 ||U_oracle - U_ref||_F + first_order_stop_term, U_ref for the V the device returned.  The stop term is
              what the kernels' stop rules leave, to first order, through the reference's own derivatives: Newton residual 1e-12,
              bisection width 1e-15 max(1, theta), and wave_nnqp's 1e-13 max |C u0 - d| on the rows it leaves out; AM_FEAS_TOL = 1e-6
              plays no part
  rows        every row's violation <= 4 (the oracle's for that row) + 8 u n ||row||
  quadratic   q_c <= 1e-12 + 8 u n r_c
  objectives  objectives[0] and master_objective within 4 e_ref of their long-double values at the returned (U, V); e_ref over the
              summation orders of omc_altmin_ref.objectives_ref (1/2 sum A^2 entry after entry, as the host adds it, is the largest
              part at 257 x 260) and not below one rounding of the result, u (|u'Hu| / 2 + |g'u| + sum A^2 / 2) resp. u |value|: without
              that floor a correctly rounded result, one ulp from another correctly computed one, failed at rank 3
  state       n_iters = 1, converged false; a problem alone equals the same problem in a batch bit for bit; a repeated call repeats; dynamic
              LDS and the global slab (OMC_ALTMIN_NOLDS) agree bit for bit
  degenerate  starts with a zero column / two equal columns (ranks 2, 3, 5): V finite and, per column, ||U0 v - U0 v_ref|| <=
              4 ||U0||_2 max(E, k u ||v_ref||) with E the largest e_ref of the regular start of the same shape: the component in the null
              space of the normal equations does not reach U0 V, and on the range the system is as conditioned as the regular one.  Before
              the null-pivot rule in ak_inv / aw_inv8 these starts gave V = 0 in every non-empty column (error in U0 V: the whole product).
              The U-step behind such a V is not pinned (model_U is not strictly convex there): it must return, finite or converged = false.
The whole loop at ranks 4 and 7 (12 iterations) is compared with the oracle as tests/test_gpu_altmin_wide.py does for 5, 6 and 8.

MEASURED below: worst error over bound per rank and kernel (every run prints its own, one line per shape)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):      # the child process below starts without conftest.py
    if _p not in sys.path:
        sys.path.insert(0, _p)

import altmin_step_cases as C      # noqa: E402
import omc_altmin_ref as R         # noqa: E402

pytestmark = pytest.mark.gpu
LD = np.longdouble
U_RND = R.U_RND
MAX_ITERS_LOOP = 12
ALL = C.REGULAR + C.STRIDE
NOLDS_SHAPES = [C.REGULAR[0], C.REGULAR[3], C.REGULAR[7]]      # one per kernel: ranks 1, 4, 8
MEASURED = """
worst error over bound per rank, product library, MI355X (31 shapes, 117 problems; a value of 1 would be a failure):
  rank  kernel      V-step  U-step (largest ||U - U_ref||_F)  quadratic q / bound  model_U objective  master objective
  1     k_altmin    0.640   0.289 (4.1e-16)                   0.000                0.264              0.253
  2     k_altmin_k  0.521   0.060 (2.6e-13)                   0.321                0.250              0.506
  3     k_altmin_k  0.250   0.004 (7.8e-14)                   0.036                0.230              0.131
  4     k_altmin_k  0.386   0.033 (5.3e-13)                   0.684                0.322              0.780
  5     k_altmin_w  0.529   0.020 (2.4e-14)                   0.056                0.234              0.125
  6     k_altmin_w  0.252   0.002 (5.3e-15)                   0.011                0.148              0.118
  7     k_altmin_w  0.308   0.002 (1.0e-15)                   0.001                0.174              0.033
  8     k_altmin_w  0.350   0.012 (3.5e-12)                   0.722                0.262              0.440
  rows: the largest violation stays 3.5e-15 below its bound.  Degenerate starts: ||U0 (V - V_ref)|| <= 1.2e-14 per column, 0.16 of the bound
  (|U0 V_ref| up to 10.3).  The same library without the null-pivot rule returns V = 0 there; without the refinement step in wave_nnqp
  it leaves rows up to 2.3e-13 beyond their bound (17 of the 31 test_u_step cases failed on that build).
  Address space: k_altmin_w runs on the global slab at rank 8 from 31 x 33 on and at rank 5 for 257 x 260, in dynamic LDS otherwise;
  k_altmin and k_altmin_k in LDS at every shape here (107 KB at rank 4, 257 x 260); the OMC_ALTMIN_NOLDS repeats are bit-identical.
Mutants (each built once, never committed): cases of this module that fail / of the 20 altmin tests the suite had before
  V-step without U'U / gamma                                  39 / 17
  U-step quantities only for rows below 256                   12 / 1   (only the shapes with 257 rows; test_altmin_global_slab_variant)
  Newton loop ends at 1e-6                                    29 / 12
  symmetry-breaking rows start one row lower                  26 / 16
  k_altmin_w: right-hand side read from lane c of the wave    18 / 9
"""


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


_runs = {}


def _call(omc_mod, S, idx=None, nolds=False, max_iters=1):
    eng = omc_mod.Engine(S.A, S.mask, C.GAMMA, S.k)
    idx = range(len(S.starts)) if idx is None else idx
    if nolds:
        eng.tuning_set("OMC_ALTMIN_NOLDS", "1")
    try:
        out = eng.alternating_minimization([S.starts[p] for p in idx], [S.node_sets[p] for p in idx], S.cut_type, max_iters=max_iters)
    finally:
        if nolds:
            eng.tuning_set("OMC_ALTMIN_NOLDS", None)
        eng.close()
    return out


def _run(omc_mod, spec):
    """the batch of one shape, run once per module"""
    if spec not in _runs:
        S = C.shape(spec)
        eng = omc_mod.Engine(S.A, S.mask, C.GAMMA, S.k)
        plan = eng.altmin_plan(max_cuts=2)
        eng.close()
        print(C.shape_id(spec), "altmin_plan", plan)
        _runs[spec] = _call(omc_mod, S)
    return _runs[spec]


def _fro(x):
    return float(np.sqrt((np.asarray(x, LD) ** 2).sum()))


def _same(a, b):
    for g, h in zip(a, b):
        assert g["n_iters"] == h["n_iters"] and g["converged"] == h["converged"]
        assert np.array_equal(g["objectives"], h["objectives"], equal_nan=True)
        assert np.array_equal(np.float64(g["master_objective"]), np.float64(h["master_objective"]), equal_nan=True)
        assert np.array_equal(g["U"], h["U"], equal_nan=True) and np.array_equal(g["V"], h["V"], equal_nan=True)


@pytest.mark.parametrize("spec", ALL, ids=C.shape_id)
def test_v_step(have_gpu, omc, spec):
    S = C.shape(spec)
    got = _run(omc, spec)
    worst = 0.0
    for p, g in enumerate(got):
        r = S.v_ref(p)
        assert (r["rank"] == S.k).all()                      # regular starts: every column's system is nonsingular
        err = np.sqrt(((np.asarray(g["V"], LD) - r["V"]) ** 2).sum(0)).astype(np.float64)
        bound = 4.0 * np.maximum(r["e_ref"], S.k * U_RND * np.sqrt((r["V"] ** 2).sum(0)).astype(np.float64))
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(ratio.max()))
    print(C.shape_id(spec), "V-step: worst error / bound %.3f" % worst)
    for p, g in enumerate(got):
        r = S.v_ref(p)
        err = np.sqrt(((np.asarray(g["V"], LD) - r["V"]) ** 2).sum(0)).astype(np.float64)
        bound = 4.0 * np.maximum(r["e_ref"], S.k * U_RND * np.sqrt((r["V"] ** 2).sum(0)).astype(np.float64))
        assert (err <= bound).all(), (S.labels[p], int(np.argmax(err - bound)), float((err - bound).max()))


@pytest.mark.parametrize("spec", ALL, ids=C.shape_id)
def test_u_step(have_gpu, omc, spec):
    S = C.shape(spec)
    got = _run(omc, spec)
    n, k = S.n, S.k
    lines = []
    for p, g in enumerate(got):
        assert g["n_iters"] == 1 and g["converged"] is False and len(g["objectives"]) == 1, (S.labels[p], g["n_iters"], g["converged"])
        r = S.u_ref(p, g["V"])
        assert r["stationarity"] <= 1e-17 and max(r["row_violation"], r["quad_violation"]) <= 1e-13 and r["complementarity"] <= 1e-10, \
            (S.labels[p], r["stationarity"], r["row_violation"], r["quad_violation"], r["complementarity"])
        D = r["data"]
        d_or = _fro(np.asarray(r["seed"], LD) - r["U"])
        stop = R.first_order_stop_term(r)
        d_gpu = _fro(np.asarray(g["U"], LD) - r["U"])
        bound_U = 4.0 * d_or + stop
        Cl = np.asarray(D["C"], LD)
        rv_gpu = np.asarray(Cl @ np.asarray(g["U"], LD).ravel() - np.asarray(D["d"], LD), np.float64) if len(D["d"]) else np.zeros(0)
        rv_or = np.asarray(Cl @ np.asarray(r["seed"], LD).ravel() - np.asarray(D["d"], LD), np.float64) if len(D["d"]) else np.zeros(0)
        rb = 4.0 * np.maximum(rv_or, 0.0) + 8.0 * U_RND * n * np.sqrt((D["C"] ** 2).sum(1)) if len(D["d"]) else np.zeros(0)
        q_gpu = np.asarray(((np.asarray(g["U"], LD) @ np.asarray(D["W"], LD).T) ** 2).sum(0) - np.asarray(D["rad"], LD), np.float64)
        qb = 1e-12 + 8.0 * U_RND * n * D["rad"]
        lines.append((S.labels[p], d_gpu, bound_U, d_or, stop, float((rv_gpu - rb).max()) if len(rb) else -0.0, float((q_gpu / qb).max())))
    for (lab, d_gpu, bound_U, d_or, stop, rex, qr) in lines:
        print(C.shape_id(spec), lab, "U-step: ||U - U_ref|| %.2e bound %.2e (oracle %.2e, stop term %.2e) ratio %.3f; row violation - bound %.1e; "
              "q / bound %.3f" % (d_gpu, bound_U, d_or, stop, d_gpu / bound_U if bound_U > 0 else float(d_gpu > 0), rex, qr))
    for (lab, d_gpu, bound_U, d_or, stop, rex, qr) in lines:
        assert d_gpu <= bound_U, (lab, d_gpu, bound_U)
        assert rex <= 0.0, (lab, rex)
        assert qr <= 1.0, (lab, qr)


@pytest.mark.parametrize("spec", ALL, ids=C.shape_id)
def test_objectives(have_gpu, omc, spec):
    S = C.shape(spec)
    got = _run(omc, spec)
    res = []
    for p, g in enumerate(got):
        assert len(g["objectives"]) == 1, (S.labels[p], g["n_iters"], g["converged"])
        o = R.objectives_ref(S.inst, g["U"], g["V"])
        res.append((S.labels[p], abs(float(LD(g["objectives"][0]) - LD(o["model_U"]))), 4.0 * o["model_U_e_ref"],
                    abs(float(LD(g["master_objective"]) - LD(o["master"]))), 4.0 * o["master_e_ref"]))
    ratio = lambda e, b: e / b if b > 0 else float(e > 0) * np.inf
    print(C.shape_id(spec), "objectives: worst error / bound, model_U %.3f master %.3f" % (
        max(ratio(e, b) for _, e, b, _, _ in res), max(ratio(e, b) for _, _, _, e, b in res)))
    for lab, e1, b1, e2, b2 in res:
        assert e1 <= b1, (lab, "model_U", e1, b1)
        assert e2 <= b2, (lab, "master", e2, b2)


@pytest.mark.parametrize("spec", C.REGULAR + [s for s in C.STRIDE if s[2] == 257 and s[0] in (1, 4, 8)], ids=C.shape_id)
def test_slot_and_batch_independence(have_gpu, omc, spec):
    """problem i alone equals problem i of the batch, bit for bit, and the batch repeats"""
    S = C.shape(spec)
    got = _run(omc, spec)
    _same(got, _call(omc, S))
    for p in range(len(S.starts)):
        _same([got[p]], _call(omc, S, idx=[p]))


@pytest.mark.parametrize("spec", NOLDS_SHAPES, ids=C.shape_id)
def test_lds_and_slab_agree(have_gpu, omc, spec):
    S = C.shape(spec)
    eng = omc.Engine(S.A, S.mask, C.GAMMA, S.k)
    a, b = eng.altmin_plan(max_cuts=2), eng.altmin_plan(max_cuts=2, nolds=True)
    eng.close()
    print(C.shape_id(spec), "plan", a, "nolds", b)
    assert a["lds_bytes"] > 0 and a["slab_bytes"] == 0 and b["slab_bytes"] > 0
    _same(_run(omc, spec), _call(omc, S, nolds=True))


@pytest.mark.parametrize("k,kind", C.DEGENERATE, ids=lambda x: str(x))
def test_degenerate_start(have_gpu, omc, k, kind):
    S = C.shape(C.REGULAR[k - 1])
    Ud = C.degenerate_start(S.U0, kind)
    eng = omc.Engine(S.A, S.mask, C.GAMMA, k)
    g = eng.alternating_minimization([Ud], [[]], S.cut_type, max_iters=1)[0]
    eng.close()
    r = R.v_step_ref(S.A, S.mask, C.GAMMA, Ud)
    assert (r["rank"] < k).all()
    assert np.isfinite(g["V"]).all()
    E = float(np.nanmax(S.v_ref(S.labels.index("s1-c0") if "s1-c0" in S.labels else 1)["e_ref"]))
    Ul = np.asarray(Ud, LD)
    err = np.sqrt(((Ul @ (np.asarray(g["V"], LD) - r["V"])) ** 2).sum(0)).astype(np.float64)
    bound = 4.0 * float(np.linalg.norm(Ud, 2)) * np.maximum(E, k * U_RND * np.sqrt((r["V"] ** 2).sum(0)).astype(np.float64))
    print("k", k, kind, "largest |U0 V_ref| %.3f, ||U0 (V - V_ref)|| per column: worst %.2e, worst error / bound %.3f" % (
        float(np.abs(Ul @ r["V"]).max()), float(err.max()), float((err / bound).max())))
    assert (err <= bound).all(), (int(np.argmax(err / bound)), float(err.max()))
    assert g["n_iters"] == 1
    assert g["converged"] is False or (np.isfinite(g["U"]).all() and np.isfinite(g["objectives"]).all())


# ---- the whole loop at the two ranks no other test runs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,cut_type,n,m,frac", [(4, "linear2", 16, 22, 0.6), (7, "linear", 20, 26, 0.75)])
def test_whole_loop_matches_oracle(have_gpu, omc, orc, k, cut_type, n, m, frac):
    """rank 4 is the top of k_altmin_k (AK_KMAX, all 16 quadratic constraints), rank 7 a rank of k_altmin_w that is no power of two; instance,
    starts, node sets and assertions as in tests/test_gpu_altmin_wide.py"""
    import test_gpu_altmin_wide as wide
    c = wide.Case()
    c.k, c.cut_type, c.n, c.m = k, cut_type, n, m
    c.A, c.mask = orc.make_instance(n, m, k, seed=70 + k, kind="lowrank", n_indices=int(frac * n * m))
    c.inst = orc.Instance(c.A, c.mask, wide.GAMMA, k)
    c.U0 = orc.svd_rounding(np.where(c.mask, c.A, 0.0), k)
    rng = np.random.default_rng(2)
    dirs = orc.child_directions(cut_type, k)
    x1 = np.linalg.qr(rng.standard_normal((n, 1)))[0][:, 0]; x2 = np.linalg.qr(rng.standard_normal((n, 1)))[0][:, 0]
    c.node_sets = [[], [(x1, c.U0 * 0.6, list(dirs[1]))], [(x1, c.U0 * 0.6, list(dirs[-1])), (x2, -c.U0 * 0.3, list(dirs[0]))]]
    c.starts = [c.U0, c.U0, c.U0 + 0.05 * rng.standard_normal((n, k))]
    eng = omc.Engine(c.A, c.mask, wide.GAMMA, k)
    got = eng.alternating_minimization(c.starts, c.node_sets, cut_type, max_iters=MAX_ITERS_LOOP)
    eng.close()
    for node, g in enumerate(got):
        r = orc.alternating_minimization(c.inst, c.starts[node], c.node_sets[node], cut_type, max_iters=MAX_ITERS_LOOP)
        print("k", k, "node", node, "n_iters", g["n_iters"], r["n_iters"], "objective", g["objectives"][-1:], r["objectives"][-1:],
              "max|UV - UV_oracle|", float(np.abs(g["U"] @ g["V"] - r["U"] @ r["V"]).max()))
        wide._assert_matches(orc, c, g, r)


# ---- against another build --------------------------------------------------------------------------------------------------------------
def _flat(omc_mod, specs):
    out = {}
    for spec in specs:
        for p, g in enumerate(_call(omc_mod, C.shape(spec))):
            for s in ("U", "V", "objectives", "master_objective", "n_iters", "converged"):
                out["%s/%d/%s" % (C.shape_id(spec), p, s)] = np.asarray(g[s])
    return out


def test_steps_against_another_build(have_gpu, omc, tmp_path):
    """With OMC_PARENT_LIB naming another build of the library, every regular and stride case runs there in a child process.  V, n_iters
    and converged must be bit-identical: the null-pivot rule of the V-step changes nothing where every pivot is above its threshold.
    With OMC_PARENT_EXACT=1 so must U and the objectives (a build with the same U-step; against a build whose NNQP leaves the ridge's
    residual on the rows they differ by about 1e-14 |multiplier|, which is printed).  Without OMC_PARENT_LIB the reference comparisons
    above are the check and this test has nothing to add."""
    parent = os.environ.get("OMC_PARENT_LIB")
    if not parent:
        return
    out = str(tmp_path / "parent.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, OMC_AMD_LIB=parent), timeout=300)
    z = np.load(out)
    mine = _flat(omc, ALL)
    assert set(mine) == set(z.files)
    exact = os.environ.get("OMC_PARENT_EXACT") == "1"
    worst = 0.0
    for key, val in mine.items():
        if exact or key.rsplit("/", 1)[1] in ("V", "n_iters", "converged"):
            assert np.array_equal(val, z[key], equal_nan=True), key
        elif val.size:
            worst = max(worst, float(np.abs(val - z[key]).max()))
    print("against", os.path.basename(os.path.dirname(parent)), ":", len(mine), "arrays,", "all" if exact else "V and the loop state", "bit-identical;",
          "largest difference elsewhere %.2e" % worst)


if __name__ == "__main__":      # child process of test_steps_against_another_build: the same cases on the library OMC_AMD_LIB names
    import omc_amd
    np.savez(sys.argv[1], **_flat(omc_amd, ALL))
