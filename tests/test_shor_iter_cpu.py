"""CPU side of tests/test_shor_iter.py: the cases bite, and the reference knows its own error.

  structure     every case of tests/shor_iter_cases.py meets the structural conditions it states (three column types, shared V1 / V2 keys,
                a coordinate in 7 minors or more, minor counts 255 / 256 / 257 / 513, columns whose paraboloid is empty, the last row / column
                in C, more than 256 rows / columns, the bump at the check of iteration 2 in the reference and none at a cap of 2)
  checks        the oracle checks at it % check_every == 0 and at it == max_iters: a cap of 26 has checks at 25 and 26
  case C        the reference with the bump differs from the one without by far more than any bound of the GPU test: a solver that
                ignores the bump parameters, or rescales nothing, cannot pass there
  e_ref         per case, t and array: the perturbation spread (oracle/omc_shor_iter_ref.py), not below the rounding of the state to float64
  high precision  case A at the root, t = 1, 2, 3: the float64 oracle is within 4 x the spread-based e_ref of the 50-digit restatement
                (shor_state_mp) for X, W, Theta, Y, U, V1, V2, V3, objective, rp and rd.  It holds, so e_ref stays the spread-based figure.

RECORDED (distance of the float64 oracle to the 50-digit state / spread-based e_ref, case A; the module prints them):
  t = 1   X 7.0e-16/4.0e-15  W 3.4e-14/1.4e-13  Theta 9.3e-16/1.4e-14  Y 0/2.0e-17  U, V1, V2, V3 0/0  objective 7.2e-15/4.3e-14  rp 1.6e-15/1.8e-15  rd 1.8e-15/1.8e-15
  t = 2   X 6.9e-15/1.2e-14  W 8.1e-15/1.5e-14  Theta 1.4e-14/2.3e-14  Y 4.1e-15/3.4e-15  U 0/0  V1 2.9e-17/4.7e-17  V2 4.6e-17/1.5e-16  V3 2.4e-17/4.5e-17
          objective 1.7e-14/2.8e-14  rp 4.3e-15/5.3e-15  rd 4.9e-16/1.8e-15
  t = 3   X 5.0e-15/6.8e-15  W 5.0e-14/1.0e-13  Theta 3.0e-14/4.9e-14  Y 1.9e-15/1.9e-15  U 0/0  V1 1.7e-16/2.3e-16  V2 4.7e-16/9.9e-16  V3 1.1e-16/1.3e-16
          objective 1.3e-14/4.6e-14  rp 4.9e-15/5.3e-15  rd 2.3e-15/5.8e-15
The worst ratio is 1.2 (Y at t = 2): the oracle is within the factor 4 everywhere, so e_ref is the spread-based figure in every case.  Over all
cases the spread stays below 3e-13 on the 8 x 10 and 12 x 14 instances and reaches 1.6e-11 (Theta, 257 x 260, t = 3, ||Theta||_F of order 1e4)."""
import numpy as np
import pytest

import shor_iter_cases as C
import omc_shor_iter_ref as R


@pytest.mark.parametrize("name", C.NAMES)
def test_case_structure(name):
    c = C.cases()[name]
    C.check_structure(c)
    assert c.ts == C.TS[name]
    # the engine's shorthand "every coordinate outside the minors" is the list the oracle is given
    if c.soc_gpu is None:
        assert c.soc == C.sh.driver_shor_lists(c.mask, minors=c.minors)[1]


def test_batch_lists_structure():
    D, lists = C.batch_lists()
    assert [len(mi) for mi, _ in lists] == [34, 0, 257]
    for mi, soc in lists:
        C.sh.ShorStructure(D.n, D.m, mi, soc, D.mask)      # valid on D's instance


def test_reference_checks_on_the_grid_and_at_the_cap():
    assert C.reference("A", 26)["check_iters"] == [25, 26]
    for t in (1, 2, 3, 7):
        r = C.reference("A", t)
        assert r["iters"] == t and r["check_iters"] == [t]
    assert np.isfinite(C.reference("A", 1)["dual_bound"]) and C.reference("A", 2)["dual_bound"] == -np.inf


def test_case_C_bump_moves_the_state():
    c = C.cases()["C"]
    for t in (3, 4, 6):
        r = C.reference("C", t)
        flat = R.shor_state(c.inst, c.minors, c.soc, (), t, **dict(c.params, bump_max=0))
        assert r["n_bumps"] == 1 and flat["n_bumps"] == 0
        for key in ("X", "Theta", "Y"):
            assert R.distance(r[key], flat[key]) >= 1e-3 * np.linalg.norm(r[key]), (t, key)


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_e_ref_is_at_rounding_level(run):
    """the t-step map does not amplify rounding: every spread stays below 1e-10 relative (the F shapes reach 1e-12 at t = 3)"""
    name, t = run
    r = C.reference(name, t); e = C.e_ref(name, t)
    for key in R.ARRAYS + ("objective", "rp", "rd"):
        scale = max(float(np.linalg.norm(np.asarray(r[key], float))), 1.0)
        assert np.isfinite(e[key]) and e[key] <= 1e-10 * scale, (name, t, key, e[key], scale)
    print(C.run_id(run), "e_ref", " ".join("%s %.1e" % (key, e[key]) for key in R.ARRAYS + R.SCALARS))


@pytest.mark.parametrize("t", [1, 2, 3])
def test_oracle_against_50_digits(t):
    c = C.cases()["A"]
    r = C.reference("A", t); e = C.e_ref("A", t)
    hp = R.shor_state_mp(c.inst, c.minors, c.soc, t)
    dist = R.distance_to_mp(r, hp)
    print("A t=%d distance to the 50-digit state / spread-based e_ref:" % t, " ".join("%s %.1e/%.1e" % (key, dist[key], e[key]) for key in dist))
    for key, dv in dist.items():
        assert dv <= 4.0 * e[key], (t, key, dv, e[key])
