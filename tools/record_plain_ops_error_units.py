#!/usr/bin/env python3
"""Writes tests/golden/plain_ops_error_units.json: for the inputs of tests/test_plain_ops.py at orders from 200 on (where the float64
restatement of the kernel's algorithm takes seconds per input), the seed, ||M||_F, e_ref / (u ||M||_F) and the restatement's sweeps.
e_ref is the larger error, against long-double eigenvalues, of the restatement and of LAPACK on the shifted matrix
(oracle/omc_plain_ref.py).  CPU only; run it again when a builder, a seed or the list of orders changes -- the test compares the
recorded ||M||_F with its own input and fails on a stale file.

    python tools/record_plain_ops_error_units.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import omc_plain_ref as R  # noqa: E402


def main():
    out = {}

    def put(key, seed, M, M_ld):
        rec = R.measure_case(M, M_ld); rec["seed"] = seed
        out[key] = rec
        print(key, rec, flush=True)

    for N in R.SEP_ORDERS:
        if N < R.RECORDED_FROM:
            continue
        for key, fam, seed in R.sep_cases(N):
            Y, U = R.sep_input(fam, N, R.SEP_K, seed)
            put(key, seed, R.sep_matrix(Y, U), R.sep_matrix_ld(Y, U))
    for N in R.ROUND_ORDERS:
        if N < R.RECORDED_FROM:
            continue
        for k in R.round_ranks(N):
            for key, fam, seed in R.round_cases(N, k):
                Y = R.round_input(fam, N, k, seed)
                put(key, seed, R.sym(Y), R.sym_ld(Y))
    for n, m in R.SVD_SHAPES:
        if n < R.RECORDED_FROM or not R.svd_shape_accepted(n, m, R.SEP_K):
            continue
        for key, fam, seed in R.svd_cases(n, m, R.SEP_K):
            X = R.svd_input(fam, n, m, R.SEP_K, seed)
            put(key, seed, X @ X.T, R.gram_ld(X))
    path = os.path.join(ROOT, "tests", "golden", "plain_ops_error_units.json")
    with open(path, "w") as f:
        json.dump({"u": R.U_RND, "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(out), "cases")


if __name__ == "__main__":
    main()
