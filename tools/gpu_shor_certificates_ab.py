"""Shor-mode certificates kept against not kept, in one call (the Shor sibling of gpu_certificates_ab.py).
(1) with PARENT_LIB=<libomc_hip.so built from the parent commit>: bench.py's default line (--gpus 1 --steps 2 --warmup 1, nothing kept) with
that library against this tree, PAIRS alternating pairs on one frontier file, the dumped outputs of every pair compared bit for bit.
(2) the cost with the switch on, same commit, switch off | on, PAIRS alternating pairs, OMC_NO_GRAPH=1 so that every launch is timed: the
12 x 14 root with its 152 class-4 minors (to its 1e-6 certificate) and the 100 x 100 root of BASELINE config 2 with its class-4 list (ITERS
iterations): solve milliseconds per check interval, milliseconds per launch of the check class (k_shor_cert_snapshot and k_cert_snapshot
run in it) and of the harvest class (k_shor_cert_harvest, k_cert_harvest), results compared bit for bit, bytes per node and per slot
against omc_shor_certificate_plan, and the shortfall of the sanitised numpy bound below the reported dual_bound.
Output: stdout and OUT (default profiles/r19_shor_certificates.txt), from the line MARK on."""
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import omc_amd  # noqa: E402

PAIRS = int(os.environ.get("PAIRS", 3))
ITERS = int(os.environ.get("ITERS", 400))
MARK = "== tools/gpu_shor_certificates_ab.py =="
KEYS = ("objective", "dual_bound", "iters", "status_code")


def bench_pairs(emit, parent):
    emit("-- (1) bench.py --gpus 1 --steps 2 --warmup 1 on one frontier file, nothing kept: parent library | this tree, %d alternating pairs" % PAIRS)
    tmp = tempfile.mkdtemp(prefix="shor_cert_ab_")
    rates = {"parent": [], "new": []}
    for pair in range(PAIRS):
        for key, lib in (("parent", parent), ("new", None)):
            env = dict(os.environ)
            env.pop("OMC_AMD_LIB", None)
            if lib:
                env["OMC_AMD_LIB"] = lib
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frontier-file",
                                    os.path.join(tmp, "frontier.pkl"), "--dump-outputs", os.path.join(tmp, f"{key}{pair}")], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
            except subprocess.TimeoutExpired:
                sys.exit("bench.py (%s) did not end within 300 s: nothing further is started on the GPU" % key)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("bench.py (%s) ended with status %d: nothing further is started on the GPU" % (key, r.returncode))
            res = json.loads(r.stdout.strip().splitlines()[-1])
            rates[key].append(round(float(res["value"]), 1))
            emit(f"    pair {pair} {key:<6} {res['value']:.1f} {res['unit']}, {res['ms_per_step']:.1f} ms per step, status {res['config']['status_counts']}, iterations median {res['config']['iters_median']} max {res['config']['iters_max']}")
        files = sorted(glob.glob(os.path.join(tmp, f"parent{pair}", "*.npy")))
        diff = [os.path.basename(f) for f in files
                if not (os.path.exists(os.path.join(tmp, f"new{pair}", os.path.basename(f))) and np.array_equal(np.load(f), np.load(os.path.join(tmp, f"new{pair}", os.path.basename(f))), equal_nan=True))]
        emit(f"    pair {pair} dumped outputs: {len(files)} arrays, bit-identical: {bool(files) and not diff}" + (f"  DIFFERENT: {diff}" if diff else ""))
    emit(f"    certified node-relaxations/s: parent {rates['parent']} | this tree {rates['new']}")


def cost(emit, name, A, mask, gamma, minors, P):
    cert = omc_amd.pkg.certificate
    n, m = A.shape
    eng = omc_amd.Engine(A, mask, gamma, 1)
    eng.tuning_set("OMC_NO_GRAPH", "1")
    if minors is None:
        minors = eng.generate_rank1_matrix_completion_Shor_constraints_indexes([4])
    emit(f"-- (2) {name}: {n} x {m}, {len(minors)} minors, eps_gap {P.eps_gap:g}, at most {P.max_iters} iterations: switch off | on, {PAIRS} alternating pairs")
    rec = {0: [], 1: []}; res = {}
    for _ in range(PAIRS):
        for on in (0, 1):
            eng.keep_shor_certificates(bool(on))
            res[on] = eng.matrix_completion_SDP_relaxation([[]], "linear", P, add_Shor_valid_inequalities=True, shor_info=[(minors, None)], want_Theta=True)[0]
            ks = eng.kernel_stats(); info = eng.solver_info()
            checks = max(ks["check"]["launches"], 1)
            rec[on].append((1e3 * info["solve_seconds"] / checks, ks["check"]["ms"] / checks, ks["harvest"]["ms"] / max(ks["harvest"]["launches"], 1), checks))
            print(f"   . switch {on}: {rec[on][-1]}", flush=True)
    a, b = res[0], res[1]
    same = all(a[key] == b[key] for key in KEYS) and all(np.array_equal(a[q], b[q]) for q in ("X", "W", "Theta", "Y", "U"))
    for idx, label in ((0, "solve ms per check interval"), (1, "check class, ms per check"), (2, "harvest class, ms per harvest")):
        off = np.array([r[idx] for r in rec[0]]); on = np.array([r[idx] for r in rec[1]])
        emit(f"    {label:32s} off {np.median(off):.4f} ({off.min():.4f}..{off.max():.4f}) | on {np.median(on):.4f} ({on.min():.4f}..{on.max():.4f})")
    emit(f"    check intervals per solve {rec[0][0][3]} | {rec[1][0][3]}   status {b['status_code']} iterations {b['iters']}   results bit-identical off | on: {same}")
    c = eng.fetch_shor_certificate([0])[0]
    val, df = cert.shor_dual_bound(A, mask, gamma, [], "linear", minors, None, c, want_defects=True)
    info = eng.solver_info()
    per = 15 * len(minors) + m + 2 * n * m + info["R_max"] + (info["r_max"] + 1) ** 2
    plan = eng.shor_certificate_plan(len(minors))
    emit(f"    bytes per node {8 * (1 + per) + 8}, per slot {8 * (2 + per) + 8} (Rmax {info['R_max']}, rmax {info['r_max']}); omc_shor_certificate_plan: {plan['bytes_per_node']}, {plan['bytes_per_slot']}")
    emit(f"    bound bit-identical to the reported one: {c.bound == b['dual_bound']}; shortfall of the sanitised numpy bound {b['dual_bound'] - val:.3e} (objective {b['objective']:.9g}); defects {df}")
    eng.close()


def main():
    lines = []

    def emit(t):
        print(t, flush=True); lines.append(t)
    parent = os.environ.get("PARENT_LIB")
    if parent:
        bench_pairs(emit, parent)
    import omc_oracle as orc
    A, mask = orc.make_instance(12, 14, 1, n_indices=70, seed=2, noise=0.1)
    cost(emit, "12 x 14 root", A, mask, 80.0, orc.shor_constraints_indexes(mask, [4]), omc_amd.default_params(eps_gap=1e-6, max_iters=6000))
    A, mask, gamma, c = omc_amd.pkg.data.config_instance(2, seed=0)
    cost(emit, "config 2 root", A, mask, gamma, None, omc_amd.default_params(eps_gap=1e-5, max_iters=ITERS))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r19_shor_certificates.txt"))
    kept = open(out).read().split(MARK)[0].rstrip("\n") if os.path.exists(out) else ""
    with open(out, "w") as f:
        f.write((kept + "\n\n" if kept else "") + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
