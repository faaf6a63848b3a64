"""The rank-3, 4, 5 and 8 relaxation fixtures (tools/make_golden.py, RANK_K_CASES) carry what they were made for.  The conditions were checked
on the oracle when the fixtures were made; here they are asserted again from the stored arrays alone, without a solve.

1. Active cuts at every rank: at least two listed nodes whose oracle multipliers are positive (> 1e-9) on three or more rows other than the
   trace row and whose objective lies more than 1e-3 (relative) above the root's.  A path whose cut rows never carry a multiplier checks
   nothing about the rows.
2. Across the fixtures, a listed node beyond k_small's r <= 16 boundary (r >= 17), and a listed rank-8 node on its near side with at least two
   cuts, hence R >= 71 rows: more than wave_nnqp_g's 64-row passive set and, at n = 20, more than k_global stages of its Gram matrix.
3. Size: n <= 24, m <= 30, and no file above 32 KiB (the rank-1 and rank-2 fixtures have 6 to 10 KB; at rank 8 the nine n x k matrices of
   the cuts alone are 11.5 KB of incompressible doubles).

Every listed node is certified (status 0): the 2e-6 bound of test_hip_reproduces_golden holds for certified values only."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("lowrank_16x20_k3_linear", "lowrank_16x20_k4_linear3", "lowrank_16x20_k5_linear2", "lowrank_20x26_k8_linear2")
OLD_KEYS = ("A", "mask", "gamma", "k", "cut_type", "rho_scale", "cut_x", "cut_U", "cut_dir", "node_L", "objective", "dual_bound", "status",
            "iters", "lmin", "eval_obj")


def path_of(name):
    return os.path.join(HERE, "golden", name + ".npz")


@pytest.fixture(scope="module")
def fixtures():
    return {name: np.load(path_of(name), allow_pickle=False) for name in NAMES}


def rows_of(k, L):
    return 1 + k * (k + 1) // 2 + L * (2 * k + 1)


@pytest.mark.parametrize("name", NAMES)
def test_keys_shapes_and_row_counts(fixtures, name):
    z = fixtures[name]
    assert all(key in z.files for key in OLD_KEYS + ("R", "r", "n_active", "lam", "breakpoints", "reference_quirk_q1"))
    n, m = z["A"].shape
    k = int(z["k"]); B = len(z["node_L"]); Lmax = int(z["node_L"].max())
    assert z["mask"].shape == (n, m) and z["cut_x"].shape == (Lmax, n) and z["cut_U"].shape == (Lmax, n, k) and z["cut_dir"].shape == (Lmax, k)
    for key in ("objective", "dual_bound", "status", "iters", "lmin", "eval_obj", "R", "r", "n_active"):
        assert z[key].shape == (B,), key
    assert z["node_L"][0] == 0 and (np.diff(z["node_L"]) > 0).all()
    assert (z["status"] == 0).all()                                              # only certified prefixes are nodes
    assert np.array_equal(z["R"], [rows_of(k, int(L)) for L in z["node_L"]])
    assert np.array_equal(z["r"], [min(n, k + int(L)) for L in z["node_L"]])    # every cut vector adds a direction until the space is full
    assert z["lam"].shape == (B, int(z["R"].max()))
    for b in range(B):
        lam = z["lam"][b]
        assert (lam >= 0).all() and not lam[int(z["R"][b]):].any()
        assert int((lam[1:int(z["R"][b])] > 1e-9).sum()) == int(z["n_active"][b])   # row 0 is the trace row
    assert (np.abs(z["objective"] - z["dual_bound"]) <= 1e-6 * np.maximum(1.0, np.abs(z["objective"]))).all()


@pytest.mark.parametrize("name", NAMES)
def test_condition_1_active_cuts_and_a_moved_objective(fixtures, name):
    z = fixtures[name]
    root = float(z["objective"][0])
    moved = (z["n_active"] >= 3) & (z["objective"] > root * (1.0 + 1e-3))
    assert int(moved.sum()) >= 2, (z["node_L"], z["n_active"], z["objective"])


def test_condition_2_both_sides_of_the_r16_boundary(fixtures):
    nodes = [(int(z["k"]), int(L), int(r), int(R)) for z in fixtures.values() for L, r, R in zip(z["node_L"], z["r"], z["R"])]
    assert any(r >= 17 for _, _, r, _ in nodes)
    assert any(k == 8 and r <= 16 and L >= 2 and R >= 71 for k, L, r, R in nodes)
    assert sorted({k for k, _, _, _ in nodes}) == [3, 4, 5, 8]


@pytest.mark.parametrize("name", NAMES)
def test_condition_3_size(fixtures, name):
    z = fixtures[name]
    n, m = z["A"].shape
    assert n <= 24 and m <= 30
    assert os.path.getsize(path_of(name)) <= 32 * 1024


def test_coverage_of_cut_types_and_options(fixtures):
    assert {str(z["cut_type"]) for z in fixtures.values()} == {"linear", "linear2", "linear3"}
    assert any(str(z["breakpoints"]) == "smallest_2_eigvec" for z in fixtures.values())
    assert any(str(z["cut_type"]) == "linear3" and not bool(z["reference_quirk_q1"]) for z in fixtures.values())


@pytest.mark.parametrize("name", NAMES)
def test_cut_vectors_and_pieces_are_legal(fixtures, name, orc):
    """Each cut vector has unit norm and the pieces are legal for the cut type; a direction away from left / right needs |v-hat| > 0.05."""
    z = fixtures[name]
    legal = {orc.DIR_CODES[s] for s in orc.DIRECTIONS_OF[str(z["cut_type"])]}
    outer = {orc.DIR_CODES["left"], orc.DIR_CODES["right"]}
    for x, U, d in zip(z["cut_x"], z["cut_U"], z["cut_dir"]):
        assert abs(np.linalg.norm(x) - 1.0) < 1e-9
        assert set(int(c) for c in d) <= legal
        vhat = U.T @ x
        assert all(int(c) in outer or abs(v) > 0.05 for c, v in zip(d, vhat))
