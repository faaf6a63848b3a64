#!/usr/bin/env python3
"""Writes tests/golden/plain_multi_error_units.json: for every input of tests/test_plain_multi.py (tests/plain_multi_cases.py) the seed,
||M||_F, e_ref / (u ||M||_F) and the sweeps of the float64 restatement, in the format of plain_ops_error_units.json.  e_ref is the larger
error, against long-double Rayleigh quotients, of omc_plain_ref.jacobi_restated and of LAPACK on the shifted matrix.  CPU only.  The
order-1040 inputs take minutes each (the restatement is numpy, one round-robin step at a time); the inputs are spread over worker
processes and every entry is a function of its input alone, so the file does not depend on their number.  The tests only read the file
and fail on a stale one (the recorded ||M||_F is compared with the input's).

    python tools/record_plain_multi_error_units.py [--orders 145,160] [--jobs 8] [--print-only]"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import omc_plain_ref as R  # noqa: E402
import plain_multi_cases as PC  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "plain_multi_error_units.json")


def _measure(job):
    orders, idx = job
    key, seed, _, build = PC.all_inputs(orders)[idx]
    M, M_ld = build()
    rec = R.measure_case(M, M_ld); rec["seed"] = seed
    print(key, rec, flush=True)
    return key, rec


def record(orders=None, jobs=1):
    """{key: entry} of the inputs at `orders` (None: all of them)."""
    n = len(PC.all_inputs(orders))
    todo = [(orders, i) for i in sorted(range(n), key=lambda i: -PC.all_inputs(orders)[i][2])]      # the long ones first
    if jobs <= 1:
        return dict(_measure(j) for j in todo)
    with multiprocessing.Pool(jobs) as pool:
        return dict(pool.imap_unordered(_measure, todo))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", default=None, help="comma-separated orders (default: every order of the tests)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--print-only", action="store_true", help="do not write the file")
    a = ap.parse_args()
    orders = None if a.orders is None else [int(v) for v in a.orders.split(",")]
    out = record(orders, a.jobs)
    if a.print_only:
        return
    if orders is not None and os.path.exists(PATH):      # a partial run replaces its own entries
        with open(PATH) as f:
            old = json.load(f)["cases"]
        old.update(out); out = old
    with open(PATH, "w") as f:
        json.dump({"u": R.U_RND, "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", PATH, len(out), "cases")


if __name__ == "__main__":
    main()
