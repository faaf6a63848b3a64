"""Separation, rounding and the left singular vectors on the multi-workgroup eigen-kernels (omc_launch_cone_plain_mw) against a second
build of the library, the parent commit's, both loaded into this one process:

    python tools/gpu_plain_multi_ab.py /path/to/parent/libomc_hip.so [--orders 1040] [--low-orders 514,1000] [--new-orders 2000] [--pairs 3]

(1) Bit-identity of the clip path, whose thresholds became arguments of k_mw_round: Engine.psd_project(algo = 2) at orders 400 and 1040,
    P, eigenvalues and V np.array_equal between the two libraries.
(2) Time of a one-matrix breakpoint_vectors, round_Y and left_singular call (host clock around the call, which ends in a synchronise; every
    shape warmed on both sides first; PAIRS alternating pairs, median and range): at --orders with the default knob on both sides, at
    --low-orders with OMC_PLAIN_MULTI_MIN = 145 on the new side only (the parent has no such knob and runs its cold kernel).
    At --new-orders the new side alone is timed (a cold call of the parent takes minutes at order 2000).
    The new side's calls, sweeps and exhausted budgets (Engine.plain_multi_stats) stand beside the times.
--profile-call N: nothing but one warmed separation call at order N with this tree's library, for a rocprofv3 --kernel-trace --stats run.
Output: stdout and OUT (default profiles/r22_plain_multi.txt), from the line MARK on."""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import omc_plain_ref as R  # noqa: E402

MARK = "== tools/gpu_plain_multi_ab.py =="
KNOB = "OMC_PLAIN_MULTI_MIN"
K = 2


def load_package(name, lib):
    """The Python package bound to the library at `lib` (None: this tree's), as a module of its own: _lib.py keeps one library per module."""
    pkg = os.path.join(ROOT, "optimalmatrixcompletion.jl_amd")
    keep = os.environ.pop("OMC_AMD_LIB", None)
    if lib:
        os.environ["OMC_AMD_LIB"] = os.path.abspath(lib)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mod.load()
    finally:
        os.environ.pop("OMC_AMD_LIB", None)
        if keep is not None:
            os.environ["OMC_AMD_LIB"] = keep
    return mod


def engine(pkg, n, m):
    A = np.zeros((n, m)); mask = np.zeros((n, m), bool)
    mask[np.arange(m) % n, np.arange(m)] = True; A[mask] = 1.0
    return pkg.Engine(A, mask, 80.0, K)


def inputs(N):
    Y, U = R.sep_input("a", N, K, 7 * N)
    return dict(sep=(Y, U), round=R.round_input("top", N, K, 7 * N + 1), svd=R.svd_input("product", N, N, K, 7 * N + 2))


def call(eng, op, x):
    t0 = time.perf_counter()
    if op == "sep":
        out = eng.breakpoint_vectors([x[0]], [x[1]])
    elif op == "round":
        out = eng.round_Y([x])
    else:
        out = eng.left_singular([x])
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?", help="libomc_hip.so built from the parent commit")
    ap.add_argument("--orders", default="1040")
    ap.add_argument("--low-orders", default="514,1000")
    ap.add_argument("--new-orders", default="", help="orders timed on the new side alone, N (default knob) or N@knob: where a parent call takes minutes")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--profile-call", type=int, default=0)
    a = ap.parse_args()
    new = load_package("omc_amd_pkg", None)
    if a.profile_call:
        N = a.profile_call
        eng = engine(new, N, N)
        x = inputs(N)["sep"]
        call(eng, "sep", x)
        t, _ = call(eng, "sep", x)
        print("order %d separation call: %.2f ms, %s" % (N, 1e3 * t, eng.plain_multi_stats()))
        eng.close()
        return
    if not a.parent:
        sys.exit("the path of the parent commit's libomc_hip.so is needed")
    old = load_package("omc_amd_parent", a.parent)
    lines = []

    def emit(t):
        print(t, flush=True); lines.append(t)
    emit("-- (1) clip path, Engine.psd_project(algo = 2): this tree against the parent library, np.array_equal of (P, eigenvalues, V)")
    ea, eb = engine(new, 16, 16), engine(old, 16, 16)
    for N in (400, 1040):
        G = np.random.default_rng(N).standard_normal((N, N)); M = 0.5 * (G + G.T) / np.sqrt(N)
        ra = ea.psd_project(M, lo=0.0, hi=1.0, algo=2, want_evals=True, want_V=True)
        rb = eb.psd_project(M, lo=0.0, hi=1.0, algo=2, want_evals=True, want_V=True)
        same = [bool(np.array_equal(x, y)) for x, y in zip(ra, rb)]
        emit("order %4d: P %s  eigenvalues %s  V %s   sweeps %d | %d" % (N, same[0], same[1], same[2], ea.cone_multi_stats()["last_sweeps"], eb.cone_multi_stats()["last_sweeps"]))
    ea.close(); eb.close()
    emit("-- (2) one-matrix calls, ms (median, min .. max of %d alternating pairs): new | parent | parent / new ; new side: sweeps, exhausted budgets" % a.pairs)
    plan = ([(int(v), None, True) for v in a.orders.split(",") if v] + [(int(v), "145", True) for v in a.low_orders.split(",") if v]
            + [(int(v.split("@")[0]), (v.split("@") + [None])[1], False) for v in a.new_orders.split(",") if v])      # N or N@knob
    for N, knob, both in plan:
        x = inputs(N)
        ea, eb = engine(new, N, N), (engine(old, N, N) if both else None)
        ea.tuning_set(KNOB, knob)
        for op in ("sep", "round", "svd"):
            call(ea, op, x[op])      # warm: buffers, code objects
            if both:
                call(eb, op, x[op])
            ta, tb, st = [], [], None
            for _ in range(a.pairs):
                ta.append(call(ea, op, x[op])[0]); st = ea.plain_multi_stats()
                tb.append(call(eb, op, x[op])[0] if both else float("nan"))
            ta, tb = 1e3 * np.array(ta), 1e3 * np.array(tb)
            emit("order %4d %-5s knob %-7s: %9.2f (%.2f .. %.2f) | %9.2f (%.2f .. %.2f) | %7.2f ; calls %d sweeps %d exhausted %d device %.2f ms"
                 % (N, op, knob or "default", np.median(ta), ta.min(), ta.max(), np.median(tb), tb.min(), tb.max(), np.median(tb) / np.median(ta),
                    st["calls"], st["max_sweeps"], st["exhausted"], st["device_us"] / 1e3))
        ea.close()
        if both:
            eb.close()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r22_plain_multi.txt"))
    kept = open(out).read().split(MARK)[0].rstrip("\n") if os.path.exists(out) else ""
    with open(out, "w") as f:
        f.write((kept + "\n\n" if kept else "") + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
