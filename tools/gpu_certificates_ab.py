"""Certificates kept against not kept, in one call.
(1) with PARENT_LIB=<libomc_hip.so built from the parent commit>: bench.py's default line (--gpus 1 --steps 2 --warmup 1, certificates off)
with that library against this tree, PAIRS alternating pairs on one frontier file, the dumped outputs of every pair compared bit for bit.
(2) the cost with certificates kept: the level-DEPTH frontier of BASELINE config 2 (100 x 100, rank 1; 2^DEPTH nodes, cold, at most ITERS
iterations, OMC_NO_GRAPH=1 so that every launch is timed), keep off | keep on, PAIRS alternating pairs: solve milliseconds per check
interval, milliseconds per launch of the check class (k_cert_snapshot runs in it) and of the harvest class (k_cert_harvest), the results of
both settings compared bit for bit, and the bytes per node and per slot.
Output: stdout and OUT (default profiles/r17_certificates.txt), from the line MARK on."""
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omc_amd  # noqa: E402

PAIRS = int(os.environ.get("PAIRS", 3))
DEPTH = int(os.environ.get("DEPTH", 6))
ITERS = int(os.environ.get("ITERS", 400))
MARK = "== tools/gpu_certificates_ab.py =="


def main():
    lines = []

    def emit(t):
        print(t, flush=True); lines.append(t)
    parent = os.environ.get("PARENT_LIB")
    if parent:
        emit("-- (1) bench.py --gpus 1 --steps 2 --warmup 1 on one frontier file, certificates off: parent library | this tree, %d alternating pairs" % PAIRS)
        tmp = tempfile.mkdtemp(prefix="cert_ab_")
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
    # ---- (2) the cost with certificates kept ----------------------------------------------------------------------------------------
    A, mask, gamma, c = omc_amd.pkg.data.config_instance(2, seed=0)
    k = c["k"]
    eng = omc_amd.Engine(A, mask, gamma, k)
    eng.tuning_set("OMC_NO_GRAPH", "1")
    P = omc_amd.default_params(rho_scale=4.0, max_iters=ITERS)
    level = [[]]
    for _ in range(DEPTH):      # the frontier, level by level (short solves: the cuts need not come from converged parents)
        out = eng.matrix_completion_SDP_relaxation(level, "linear", params=P, want_X=False, want_Y=True)
        level = [kid for cuts, r in zip(level, out) for kid in omc_amd.pkg.bnb.make_children(cuts, r, "linear", k)]
    emit(f"-- (2) config 2 ({A.shape[0]} x {A.shape[1]}, rank {k}), {len(level)} nodes of depth {DEPTH}, at most {ITERS} iterations, cold: keep off | keep on, {PAIRS} alternating pairs")
    rec = {0: [], 1: []}; res = {}
    for _ in range(PAIRS):
        for on in (0, 1):
            eng.keep_certificates(bool(on))
            res[on] = eng.matrix_completion_SDP_relaxation(level, "linear", params=P, want_X=False, want_Y=True)
            ks = eng.kernel_stats(); info = eng.solver_info()
            checks = max(ks["check"]["launches"], 1)
            rec[on].append((1e3 * info["solve_seconds"] / checks, ks["check"]["ms"] / checks, ks["harvest"]["ms"] / max(ks["harvest"]["launches"], 1), checks))
            print(f"   . keep {on}: {rec[on][-1]}", flush=True)
    same = all(all(a[key] == b[key] for key in ("objective", "dual_bound", "iters", "status_code")) and np.array_equal(a["Y"], b["Y"]) and np.array_equal(a["U"], b["U"])
               for a, b in zip(res[0], res[1]))
    for idx, name in ((0, "solve ms per check interval"), (1, "check class, ms per check"), (2, "harvest class, ms per harvest")):
        off = np.array([r[idx] for r in rec[0]]); on = np.array([r[idx] for r in rec[1]])
        emit(f"    {name:32s} off {np.median(off):.4f} ({off.min():.4f}..{off.max():.4f}) | on {np.median(on):.4f} ({on.min():.4f}..{on.max():.4f})")
    emit(f"    check intervals per solve {rec[0][0][3]} | {rec[1][0][3]}   results bit-identical off | on: {same}")
    certs = eng.fetch_certificate(range(len(level)))
    cert = omc_amd.pkg.certificate
    worst = max(r["dual_bound"] - cert.dual_bound(A, mask, gamma, k, node, "linear", cc) for r, node, cc in zip(res[1], level, certs))
    info = eng.solver_info()
    nnz = int(mask.sum()); per = nnz + info["R_max"] + (info["r_max"] + k) ** 2
    emit(f"    bytes per node {8 * (1 + per) + 4} (nnz {nnz}, Rmax {info['R_max']}, rmax {info['r_max']}; omc_certificate_plan: {eng.certificate_plan(DEPTH)['bytes_per_node']}), per slot {8 * (2 + per) + 8}")
    emit(f"    largest shortfall of the sanitised numpy bound below the reported dual_bound over the {len(level)} nodes: {worst:.3e}")
    eng.close()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r17_certificates.txt"))
    kept = open(out).read().split(MARK)[0].rstrip("\n") if os.path.exists(out) else ""
    with open(out, "w") as f:
        f.write((kept + "\n\n" if kept else "") + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
