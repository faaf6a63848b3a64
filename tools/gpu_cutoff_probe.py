"""The objective cutoff (Engine.set_cutoff, drivers' objective_cutoff) measured.  One script, three parts:

  --part bench     with PARENT_LIB=<libomc_hip.so built from the parent commit>: bench.py --gpus 1 --steps 2 --warmup 1 with that library
                   against this tree, PAIRS alternating pairs on one frontier file, the dumped outputs of every pair compared bit for bit,
                   medians and spread.  The claim to support is "no change with the cutoff off".
  --part drivers   bnb.branch_and_bound and bnb_stream.branch_and_bound_streaming with objective_cutoff off | on in alternating pairs on
                   INSTANCES (small: 14 x 18 noise 0.15; branching: data.branching_instance, 100 x 100; shor: the same with the iterative
                   Shor inequalities, classes 3 and 4): nodes relaxed, nodes_relax_feasible_pruned, nodes_relax_cutoff, total iterations,
                   wall-clock, final gap per run.
  --part one       one driver run, one JSON line (what --part drivers starts).

This process never opens the GPU for --part bench and --part drivers: every run is a child with a time limit of its own, and after a child
that fails or overruns nothing further is started.  Output: stdout and OUT (default profiles/objective_cutoff.txt), appended under a mark
per part."""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = int(os.environ.get("PAIRS", 3))
# per instance: time limit of a driver run (s), keywords of both drivers, keywords of the round-based / queue-driven driver alone
INSTANCES = {
    "small": (8.0, dict(rho_scale=8.0), dict(batch=64), dict(slots=64)),
    "branching": (15.0, dict(), dict(batch=256), dict(slots=1024)),
    "shor": (25.0, dict(add_Shor_valid_inequalities=True, add_Shor_valid_inequalities_iterative=True,
                        Shor_valid_inequalities_noisy_rank1_num_entries_present=(3, 4)), dict(batch=32), dict(slots=32)),
}


def child(args, limit, env=None):
    """One GPU step: its own process, its own time limit.  Returns its stdout; ends this script when the child failed or overran."""
    try:
        r = subprocess.run([sys.executable] + args, capture_output=True, text=True, cwd=ROOT, env=env, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("%s did not end within %d s: nothing further is started on the GPU" % (" ".join(args[:6]), limit))
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit("%s ended with status %d: nothing further is started on the GPU" % (" ".join(args[:6]), r.returncode))
    return r.stdout


def spread(v):
    v = np.asarray(v, float)
    return "median %.4g (%.4g .. %.4g)" % (np.median(v), v.min(), v.max())


def part_bench(emit):
    parent = os.environ.get("PARENT_LIB")
    if not parent:
        sys.exit("--part bench needs PARENT_LIB=<the parent commit's libomc_hip.so>")
    emit("-- bench.py --gpus 1 --steps 2 --warmup 1 on one frontier file: parent library | this tree (cutoff never set), %d alternating pairs" % PAIRS)
    tmp = tempfile.mkdtemp(prefix="cutoff_ab_")
    rates = {"parent": [], "new": []}
    same = []
    for pair in range(PAIRS):
        for key, lib in (("parent", parent), ("new", None)):
            env = dict(os.environ)
            env.pop("OMC_AMD_LIB", None)
            if lib:
                env["OMC_AMD_LIB"] = lib
            out = child([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frontier-file", os.path.join(tmp, "frontier.pkl"),
                         "--dump-outputs", os.path.join(tmp, f"{key}{pair}")], 300, env)
            res = json.loads(out.strip().splitlines()[-1])
            rates[key].append(float(res["value"]))
            emit(f"    pair {pair} {key:<6} {res['value']:.1f} {res['unit']}, {res['ms_per_step']:.1f} ms per step, status {res['config']['status_counts']}, iterations median {res['config']['iters_median']} max {res['config']['iters_max']}")
        files = sorted(glob.glob(os.path.join(tmp, f"parent{pair}", "*.npy")))
        diff = [os.path.basename(f) for f in files
                if not (os.path.exists(os.path.join(tmp, f"new{pair}", os.path.basename(f))) and np.array_equal(np.load(f), np.load(os.path.join(tmp, f"new{pair}", os.path.basename(f))), equal_nan=True))]
        same.append(bool(files) and not diff)
        emit(f"    pair {pair} dumped outputs: {len(files)} arrays, bit-identical: {same[-1]}" + (f"  DIFFERENT: {diff}" if diff else ""))
    emit(f"    parent {spread(rates['parent'])} | this tree {spread(rates['new'])} {res['unit']}; ratio of the medians {np.median(rates['new']) / np.median(rates['parent']):.4f}; outputs bit-identical in every pair: {all(same)}")


def part_one(a):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import omc_amd
    tl, kw, kw_round, kw_stream = INSTANCES[a.instance]
    if a.instance == "small":
        import omc_oracle as orc
        A, mask = orc.make_instance(14, 18, 1, seed=5, kind="lowrank", n_indices=int(0.35 * 14 * 18), noise=0.15)
    else:
        A, mask = omc_amd.pkg.data.branching_instance(seed=0)
    kw = dict(kw)
    if a.instance == "shor":
        kw["shor_params"] = omc_amd.default_params(rho_scale=1.0, eps_gap=1e-5, max_iters=3000, time_limit=15.0)
    eng = omc_amd.Engine(A, mask, 80.0, 1)
    t0 = time.time()
    if a.driver == "round":
        sol, inst = omc_amd.pkg.bnb.branch_and_bound(eng, A, mask, gap=1e-4, time_limit=a.tl or tl, objective_cutoff=bool(a.cutoff), **kw, **kw_round)
    else:
        sol, inst = omc_amd.pkg.bnb_stream.branch_and_bound_streaming(eng, A, mask, gap=1e-4, time_limit=a.tl or tl, objective_cutoff=bool(a.cutoff), **kw, **kw_stream)
    wall = time.time() - t0
    rd, log = inst["run_details"], inst["relax_log"]
    eng.close()
    print(json.dumps(dict(relaxed=len(log), pruned=rd["nodes_relax_feasible_pruned"], infeasible=rd["nodes_relax_infeasible"], cutoff=rd.get("nodes_relax_cutoff", 0),
                          iterations=int(sum(e[2] for e in log)), cutoff_iterations=int(sum(e[2] for e in log if e[3] == "cutoff")),
                          pruned_iterations=int(sum(e[2] for e in log if e[3] in ("pruned", "infeasible"))),
                          wall=round(wall, 2), gap=sol["gap"], lower=sol["lower_bound"], upper=sol["objective"]), default=float))


def part_drivers(emit, a):
    for name in a.instances.split(","):
        tl = a.tl or INSTANCES[name][0]
        for driver in a.drivers.split(","):
            emit(f"-- {name}, {'bnb.branch_and_bound' if driver == 'round' else 'bnb_stream.branch_and_bound_streaming'}, gap 1e-4, time limit {tl:g} s: objective_cutoff off | on, {PAIRS} alternating pairs")
            rec = {0: [], 1: []}
            for pair in range(PAIRS):
                for on in (0, 1):
                    out = child([os.path.abspath(__file__), "--part", "one", "--instance", name, "--driver", driver, "--cutoff", str(on), "--tl", str(tl)], int(3 * tl + 120))
                    r = json.loads(out.strip().splitlines()[-1])
                    rec[on].append(r)
                    emit(f"    pair {pair} {'on ' if on else 'off'}: relaxed {r['relaxed']}, pruned {r['pruned']} (cutoff {r['cutoff']}), infeasible {r['infeasible']}, iterations {r['iterations']} "
                         f"(of the pruned or infeasible nodes {r['pruned_iterations'] + r['cutoff_iterations']}), wall {r['wall']:.2f} s, gap {r['gap']:.3e}, lower {r['lower']:.9g}, upper {r['upper']:.9g}")
            for on in (0, 1):
                v = rec[on]
                share = [(r["pruned"] + r["infeasible"]) / max(r["relaxed"], 1) for r in v]
                emit(f"    {'on ' if on else 'off'}: pruned-or-infeasible share of the relaxed nodes {spread(share)}; iterations per relaxed node {spread([r['iterations'] / max(r['relaxed'], 1) for r in v])}; "
                     f"wall {spread([r['wall'] for r in v])} s; relaxed {spread([r['relaxed'] for r in v])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("bench", "drivers", "one"), required=True)
    ap.add_argument("--instances", default="small,branching,shor")
    ap.add_argument("--drivers", default="round,stream")
    ap.add_argument("--instance", default="small")
    ap.add_argument("--driver", default="round")
    ap.add_argument("--cutoff", type=int, default=0)
    ap.add_argument("--tl", type=float, default=0.0, help="time limit of a driver run in seconds (0: the instance's own)")
    a = ap.parse_args()
    if a.part == "one":
        return part_one(a)
    lines = []

    def emit(t):
        print(t, flush=True); lines.append(t)
    mark = f"== tools/gpu_cutoff_probe.py --part {a.part}" + (f" --instances {a.instances} --drivers {a.drivers}" if a.part == "drivers" else "") + " =="
    emit(mark)
    try:
        part_bench(emit) if a.part == "bench" else part_drivers(emit, a)
    finally:
        out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "objective_cutoff.txt"))
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
