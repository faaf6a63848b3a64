"""The references of oracle/omc_altmin_ref.py checked on the CPU, on the cases tests/test_altmin_steps.py runs on the device
(tests/altmin_step_cases.py), with the V-step reference rounded to float64 as the U-step's input.

  * u_step_ref against scipy's SLSQP on the same QP (the oracle's method="slsqp"), ranks 2 and 3 at 8 x 12 (the oracle has no SLSQP path
    at rank 1): an independent solver;
  * every case's certificate: U_ref is stationary by construction (it minimises the Lagrangian of its multipliers in long double), so what
    certifies it is feasibility and complementarity;
  * coverage: every rank has a case without an active quadratic constraint, with an active ball, with an active pair cone (k >= 2), with
    an active cut row and with an active symmetry-breaking row -- read from the reference's multipliers;
  * no case sits on a stalled Newton loop of the oracle (kkt_residual <= 1e-12);
  * the reference discriminates: moving U_oracle by 1e-9 relative moves its distance to U_ref by as much.

THRESHOLDS are 4 x the largest value measured over all cases (MEASURED), none above the cap of 1e-10."""
import numpy as np
import pytest

import altmin_step_cases as C
import omc_altmin_ref as R

LD = np.longdouble
# largest over the 117 problems of the 31 shapes (quad_violation: 2 x 24, rank 2, scale 3, where the polishing step is refused; below
# 3e-18 in the stride shapes); oracle_distance is ||U_oracle - U_ref||_F, the oracle's own error (its Newton loop stops at 1e-12); slsqp_distance over the
# six SLSQP problems (status 0 or 8: at ftol = 1e-14 its line search gives up at the solution)
MEASURED = dict(stationarity=9.8e-20, row_violation=1.1e-19, quad_violation=4.2e-15, complementarity=1.6e-15, oracle_distance=5.3e-13,
                slsqp_distance=2.5e-7)
THRESHOLDS = {key: 4.0 * v for key, v in MEASURED.items()}
CAP = 1e-10
ALL = C.REGULAR + C.STRIDE


def _fro(x):
    return float(np.sqrt((np.asarray(x, LD) ** 2).sum()))


def test_thresholds_are_below_the_cap():
    for key in ("stationarity", "row_violation", "quad_violation", "complementarity"):
        assert THRESHOLDS[key] <= CAP, key


@pytest.mark.parametrize("k", [2, 3])      # the oracle has no SLSQP path at rank 1
def test_u_step_ref_agrees_with_slsqp(orc, k):
    S = C.Shape((k, C.CUT_TYPES[k % 3], 8, 12, 0.7), all_pairs=False)
    worst = 0.0
    for p in range(len(S.starts)):
        r = S.u_ref(p)
        V = np.asarray(S.v_ref(p)["V"], np.float64)
        Us, _, info = orc.altmin_u_step(S.inst, V, S.node_sets[p], S.cut_type, method="slsqp")
        assert info["slsqp_status"] in (0, 8), info
        d = _fro(np.asarray(Us, LD) - r["U"])
        print("k", k, S.labels[p], "||U_slsqp - U_ref|| %.2e" % d)
        worst = max(worst, d)
    assert worst <= THRESHOLDS["slsqp_distance"]


@pytest.mark.parametrize("spec", ALL, ids=C.shape_id)
def test_certificates(spec):
    S = C.shape(spec)
    for p in range(len(S.starts)):
        r = S.u_ref(p)
        d = _fro(np.asarray(r["seed"], LD) - r["U"])
        print(C.shape_id(spec), S.labels[p], "stationarity %.1e row %.1e quad %.1e complementarity %.1e ||U_oracle - U_ref|| %.1e kkt_residual %.1e" % (
            r["stationarity"], r["row_violation"], r["quad_violation"], r["complementarity"], d, r["seed_info"].get("kkt_residual", 0.0)))
        for key in ("stationarity", "row_violation", "quad_violation", "complementarity"):
            assert r[key] <= THRESHOLDS[key], (S.labels[p], key, r[key])
        assert d <= THRESHOLDS["oracle_distance"], (S.labels[p], d)
        assert r["seed_info"].get("kkt_residual", 0.0) <= 1e-12, S.labels[p]       # rank 1 has no Newton loop
        assert (S.v_ref(p)["rank"] == S.k).all()


@pytest.mark.parametrize("k", range(1, 9))
def test_coverage(k):
    seen = dict(none=False, ball=False, cone=k == 1, cut=False, sym=False)
    for spec in ALL:
        if spec[0] != k:
            continue
        S = C.shape(spec)
        for p in range(len(S.starts)):
            r = S.u_ref(p)
            aq, ar, kinds = r["active_quad"], r["active_rows"], r["data"]["kinds"]
            seen["none"] |= not aq.any()
            seen["ball"] |= bool(aq[:k].any())
            seen["cone"] |= bool(aq[k:].any())
            seen["cut"] |= bool((ar & (kinds == "cut")).any())
            seen["sym"] |= bool((ar & (kinds == "sym")).any())
    assert all(seen.values()), seen


@pytest.mark.parametrize("spec", C.REGULAR, ids=C.shape_id)
def test_reference_discriminates(spec):
    S = C.shape(spec)
    rng = np.random.default_rng(5)
    for p in range(len(S.starts)):
        r = S.u_ref(p)
        Uo = r["seed"]
        Up = Uo * (1.0 + 1e-9 * rng.choice([-1.0, 1.0], Uo.shape))
        moved = 1e-9 * _fro(Uo)
        d0, d1 = _fro(np.asarray(Uo, LD) - r["U"]), _fro(np.asarray(Up, LD) - r["U"])
        assert abs(d1 - moved) <= d0 + 1e-3 * moved, (S.labels[p], d0, d1, moved)
