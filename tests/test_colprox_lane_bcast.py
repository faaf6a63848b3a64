"""k_colprox_pair with the sweep and the solves on lane-broadcast fmacs (the pivot row read from the registers of its lanes, no LDS reads)
against the staged body it replaces, bit for bit.  Both bodies live in one library: OMC_COLPROX_DPP=0 selects the staged one.  With
OMC_PARENT_LIB naming the parent commit's build the default arm is also compared with that library, each in a child process (this file as
a script, the library chosen by OMC_AMD_LIB); without it that part skips.  Every comparison is np.array_equal.

prox   Engine.column_prox(mode=0, algo=0) on n = 40, m = 41 with a hand-made mask.  Its first fourteen columns are the pairs
       (1, 16) one DPP row only; (16, 17) the exact row boundary; (17, 32) both rows; (32, 32) a full half; (0, 5) an empty column beside
       a live one; (31, 2) halves of unequal length; (33, 3) a 33-row column, which sends its pair to k_colprox.  The library refuses
       n > m, so the instance cannot have thirteen columns at n = 40 (a 33-row column needs n >= 33): columns 14 .. 39 are filler pairs
       of 2 .. 9 rows and column 40 is the unpaired last one (odd m).  B = 3 slots with rho_f = 0.5, 4, 40, Y random symmetric positive
       definite.  Three calls per arm: cold; warm from the first call's alpha and s; warm with s0 scaled by 1e-3 (s far below the answer:
       the not-positive-definite branch and more than one inversion -- the staged arm must have moved some column's s by more than 5e-3
       relative, which the series finish does not carry).
solve  the mixed-column instance of tests/test_colprox_placement.py (n = 70, 75 columns), one root, max_iters=300, eps_gap=1e-14."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0
HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = ((1, 16), (16, 17), (17, 32), (32, 32), (0, 5), (31, 2), (33, 3))
SOLVE_KEYS = ("objective", "dual_bound", "iters", "status_code", "Y")


def _set(eng, arm):
    if arm is not None:
        eng.tuning_set("OMC_COLPROX_DPP", arm)


def _unset(eng, arm):
    if arm is not None:
        eng.tuning_set("OMC_COLPROX_DPP", None)


def _prox_instance():
    rng = np.random.default_rng(21)
    n = 40
    counts = [c for pr in PAIRS for c in pr] + [2 + (j % 8) for j in range(26)] + [7]
    m = len(counts)
    assert m == 41
    mask = np.zeros((n, m), dtype=bool)
    for j, cnt in enumerate(counts):
        mask[rng.choice(n, size=cnt, replace=False), j] = True
    assert mask.any(1).all() and [int(c) for c in mask.sum(0)] == counts
    U0 = rng.standard_normal((n, 1)); V0 = rng.standard_normal((1, m))
    A = (U0 @ V0 + 0.01 * rng.standard_normal((n, m))) * mask
    Y = []
    for _ in range(3):
        G = rng.standard_normal((n, n))
        S = G @ G.T / n + 0.5 * np.eye(n)
        Y.append(0.5 * (S + S.T))
    return A, mask, np.stack(Y), np.array([0.5, 4.0, 40.0])


def _prox(omc, arm, flat, prefix):
    A, mask, Y, rho_f = _prox_instance()
    eng = omc.Engine(A, mask, GAMMA, 1)
    _set(eng, arm)
    try:
        cold = eng.column_prox(Y, None, rho_f, None, mode=0, algo=0)
        warm = eng.column_prox(Y, cold["alpha"], rho_f, cold["s"], mode=0, algo=0)
        far = eng.column_prox(Y, cold["alpha"], rho_f, 1e-3 * cold["s"], mode=0, algo=0)
    finally:
        _unset(eng, arm)
        eng.close()
    for name, out in (("cold", cold), ("warm", warm), ("far", far)):
        flat[prefix + name + "/alpha"] = out["alpha"]
        flat[prefix + name + "/s"] = out["s"]


def _solve_instance():
    rng = np.random.default_rng(5)
    n = 70
    counts = ([16, 17, 32, 33, 16, 17, 32, 32, 4, 5, 0, 20, 1, 12, 31, 40, 64, 45, 3] * 4)[:75]      # n <= m; m odd
    m = len(counts)
    mask = np.zeros((n, m), dtype=bool)
    for j, cnt in enumerate(counts):
        mask[rng.choice(n, size=cnt, replace=False), j] = True
    for i in np.flatnonzero(~mask.any(1)):
        mask[i, 0] = True
    U0 = rng.standard_normal((n, 1)); V0 = rng.standard_normal((1, m))
    return (U0 @ V0 + 0.01 * rng.standard_normal((n, m))) * mask, mask


def _run(eng, nodes, P, env):
    for k_, v in env.items():
        eng.tuning_set(k_, v)
    try:
        return eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False)
    finally:
        for k_ in env:
            eng.tuning_set(k_, None)


def _solve(omc, arms, flat, prefix):
    A, mask = _solve_instance()
    eng = omc.Engine(A, mask, GAMMA, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    for name, env in arms:
        out = _run(eng, [[]], P, env)
        assert len(out) == 1 and out[0]["iters"] > 0
        for key in SOLVE_KEYS:
            flat["%s%s/%s" % (prefix, name, key)] = np.asarray(out[0][key])
        if hasattr(eng._lib, "omc_kernel_residency"):      # of the body staged last: the arm's
            flat["%s%s/residency" % (prefix, name)] = np.array([eng.kernel_residency()["k_colprox_pair"]])
    eng.close()


def _equal(a, b, pre_a, pre_b, skip=("residency",)):
    keys = sorted(k[len(pre_a):] for k in a if k.startswith(pre_a) and not k.endswith(skip))
    assert keys and keys == sorted(k[len(pre_b):] for k in b if k.startswith(pre_b) and not k.endswith(skip))
    for key in keys:
        x, y = a[pre_a + key], b[pre_b + key]
        assert np.array_equal(x, y), (key, x, y)


@pytest.fixture(scope="module")
def arms(omc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    flat = {}
    _prox(omc, None, flat, "prox/new/")
    _prox(omc, "0", flat, "prox/old/")
    _solve(omc, (("new", {}), ("old", {"OMC_COLPROX_DPP": "0"}), ("again", {})), flat, "solve/")
    return flat


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    parent = os.environ.get("OMC_PARENT_LIB")
    if not parent:
        pytest.skip("OMC_PARENT_LIB is not set: no other build to compare with")
    out = {}
    for name, lib in (("this", None), ("parent", parent)):
        path = str(tmp_path_factory.mktemp("colprox_lane_bcast") / (name + ".npz"))
        env = dict(os.environ)
        env.pop("OMC_AMD_LIB", None)
        env.pop("OMC_COLPROX_DPP", None)
        if lib:
            env["OMC_AMD_LIB"] = lib
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=300)
        out[name] = dict(np.load(path))
    return out


@pytest.mark.parametrize("call", ("cold", "warm", "far"))
def test_prox_equals_the_staged_body(arms, call):
    _equal(arms, arms, "prox/new/%s/" % call, "prox/old/%s/" % call)


def test_the_far_start_took_more_than_the_series(arms):
    """the columns the pair kernel runs (the first six pairs): s0 = 1e-3 s is not within a series step of the answer"""
    s0 = 1e-3 * arms["prox/old/cold/s"][:, :12]
    s = arms["prox/old/far/s"][:, :12]
    moved = np.abs(s - s0) > 5e-3 * np.abs(s0)
    print("columns whose s moved by more than 5e-3 relative:", int(moved.sum()), "of", moved.size)
    assert moved.any()
    assert np.all(arms["prox/old/cold/s"][:, [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11]] > 0.0)      # the pair kernel wrote them (column 8 is empty)


def test_solve_equals_the_staged_body(arms):
    _equal(arms, arms, "solve/new/", "solve/old/")


def test_solve_is_deterministic(arms):
    _equal(arms, arms, "solve/new/", "solve/again/")


def test_residency_is_three_in_both_arms(arms):
    assert int(arms["solve/new/residency"][0]) == 3 and int(arms["solve/old/residency"][0]) == 3


@pytest.mark.parametrize("case", ("prox", "solve"))
def test_equal_to_the_parent_build(builds, case):
    _equal(builds["this"], builds["parent"], "%s/new/" % case, "%s/new/" % case)


if __name__ == "__main__":      # the default arm of both cases on the library OMC_AMD_LIB names (default: the tree's own)
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import omc_amd
    out_ = {}
    _prox(omc_amd, None, out_, "prox/new/")
    _solve(omc_amd, (("new", {}),), out_, "solve/")
    np.savez(sys.argv[1], **out_)
