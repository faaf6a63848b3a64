"""k_colprox_block against the path without it (OMC_COLPROX_BLOCK_MIN=100000), in one call: (1) the prox on its own -- the printed errors
and factorization counts of tests/test_colprox_block.py::test_prox_alone_against_numpy_every_storage_class; (2) milliseconds per launch of
the colprox class (Engine.kernel_stats; OMC_NO_GRAPH=1 so that every launch is timed) with the knob at its default against 100000, PAIRS
alternating pairs, on the 70 x 72 shape of test_dense_columns_and_deep_paths (c ~ 68), the config-4 root capped as
test_config4_shape_capped_iterations_properties caps it, and the config-5 node of test_config5_node_evaluation (100 iterations), with the
objectives and dual bounds of both settings side by side; (3) the slab bytes per slot of the column prox at config 5, before and after.
(4), with PARENT_LIB=<libomc_hip.so built from the parent commit>: bench.py's default line with that library against this tree and the
dumped outputs compared bit for bit.  SHAPES=70,4,5 restricts (2); SHAPES= skips it.  Output: stdout and OUT (default profiles/r15_colprox_block.txt), from the line MARK on."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omc_amd  # noqa: E402

PAIRS = 3
MARK = "== tools/gpu_colprox_block_ab.py =="
OFF = "100000"


def shape(name):
    if name == "70":
        rng = np.random.default_rng(3)
        n, m = 70, 72
        A = rng.standard_normal((n, 1)) @ rng.standard_normal((1, m)) + 0.05 * rng.standard_normal((n, m))
        mask = rng.random((n, m)) < 0.97
        return "70 x 72, c ~ 68", A, mask, 80.0, 1, "linear", omc_amd.default_params(rho_scale=8.0, max_iters=300, eps_gap=1e-14)
    A, mask, gamma, c = omc_amd.pkg.data.config_instance(int(name), seed=0)
    if name == "4":
        return "config 4 root, 100 iterations", A, mask, gamma, c["k"], "linear3", omc_amd.default_params(rho_scale=4.0, max_iters=100, breakpoints=2)
    return "config 5 node, 100 iterations", A, mask, gamma, 2, "linear", omc_amd.default_params(rho_scale=4.0, max_iters=100, check_every=25)


def main():
    lines = []

    def emit(t):
        print(t, flush=True); lines.append(t)
    emit("-- (1) the prox on its own: error / bound per listed length (alpha, s | alpha, objcol, c0col) and factorizations, block kernel | path without it")
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", os.path.join(ROOT, "tests", "test_colprox_block.py"), "-k", "prox_alone"],
                           capture_output=True, text=True, cwd=ROOT, timeout=300)
    except subprocess.TimeoutExpired:
        sys.exit("the prox-alone test did not end within 300 s: nothing further is started on the GPU")
    for ln in r.stdout.splitlines():
        if ln.startswith("mode") or "passed" in ln or "failed" in ln:
            emit(ln)
    if r.returncode != 0:      # a failure, a fault (134, 139, negative) or a time limit: stop here, with what the child said
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        sys.exit("the prox-alone test ended with status %d: nothing further is started on the GPU" % r.returncode)
    emit("-- (2) colprox class, ms per launch (launches), default knob | OMC_COLPROX_BLOCK_MIN=%s, %d alternating pairs" % (OFF, PAIRS))
    for name in [x for x in os.environ.get("SHAPES", "70,4,5").split(",") if x]:
        title, A, mask, gamma, k, cut, P = shape(name)
        eng = omc_amd.Engine(A, mask, gamma, k)
        eng.tuning_set("OMC_NO_GRAPH", "1")
        cmax = int(mask.sum(0).max())
        ms = {"on": [], "off": []}; res = {}
        for _ in range(PAIRS):
            for key, val in (("on", None), ("off", OFF)):
                eng.tuning_set("OMC_COLPROX_BLOCK_MIN", val)
                res[key] = eng.matrix_completion_SDP_relaxation([[]], cut, params=P, want_X=False, want_Y=False)[0]
                st = eng.kernel_stats()["colprox"]
                ms[key].append(st["ms"] / max(st["launches"], 1))
                print(f"   . {title} {key}: {ms[key][-1]:.4f} ms per launch over {st['launches']} launches", flush=True)
        on, off = np.array(ms["on"]), np.array(ms["off"])
        emit(f"{title} (longest column {cmax}): block {np.median(on):.4f} ms ({on.min():.4f}..{on.max():.4f}) | without {np.median(off):.4f} ms ({off.min():.4f}..{off.max():.4f})"
             f" | ratio {np.median(off) / np.median(on):.2f}, spread {max(np.ptp(on) / np.median(on), np.ptp(off) / np.median(off)):.3f}")
        emit(f"    objective {res['on']['objective']:.12e} | {res['off']['objective']:.12e}   dual bound {res['on']['dual_bound']:.12e} | {res['off']['dual_bound']:.12e}   iterations {res['on']['iters']} | {res['off']['iters']}")
        if name == "5":
            n, m = A.shape
            cnt = mask.sum(0)
            plan = eng.colprox_plan()
            before = m * (cmax * (cmax + 1) + 4 * cmax + 8) * 8
            after = int((cnt > plan["lds_cmax"]).sum()) * plan["slab_doubles"] * 8
            emit(f"-- (3) config 5, column-prox slab per slot: {before / 2**20:.1f} MiB before (m blocks of B, L and four vectors at c_max = {cmax}) | {after / 2**20:.1f} MiB after (L alone for the {int((cnt > plan['lds_cmax']).sum())} columns beyond the LDS)")
        eng.close()
    parent = os.environ.get("PARENT_LIB")
    if parent:      # (4) bench.py's default line, the parent commit's library (OMC_AMD_LIB) against this tree, dumped outputs compared array by array
        import glob
        import json
        import tempfile
        emit("-- (4) bench.py --gpus 1 --steps 2 --warmup 1 on one frontier file: parent library | this tree")
        tmp = tempfile.mkdtemp(prefix="colprox_ab_")
        res = {}
        for key, lib in (("parent", parent), ("new", None)):
            env = dict(os.environ)
            env.pop("OMC_AMD_LIB", None)
            if lib:
                env["OMC_AMD_LIB"] = lib
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frontier-file",
                                    os.path.join(tmp, "frontier.pkl"), "--dump-outputs", os.path.join(tmp, key)], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
            except subprocess.TimeoutExpired:
                sys.exit("bench.py (%s) did not end within 300 s: nothing further is started on the GPU" % key)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("bench.py (%s) ended with status %d: nothing further is started on the GPU" % (key, r.returncode))
            res[key] = json.loads(r.stdout.strip().splitlines()[-1])
            emit(f"    {key:<6} " + "  ".join(f"{k_}={v}" for k_, v in res[key].items() if isinstance(v, (int, float, str)))[:400])
        files = sorted(glob.glob(os.path.join(tmp, "parent", "*.npy")))
        diff = [os.path.basename(f) for f in files
                if not (os.path.exists(os.path.join(tmp, "new", os.path.basename(f))) and np.array_equal(np.load(f), np.load(os.path.join(tmp, "new", os.path.basename(f))), equal_nan=True))]
        emit(f"    dumped outputs: {len(files)} arrays, bit-identical: {bool(files) and not diff}" + (f"  DIFFERENT: {diff}" if diff else ""))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r15_colprox_block.txt"))
    kept = open(out).read().split(MARK)[0].rstrip("\n") if os.path.exists(out) else ""
    with open(out, "w") as f:
        f.write((kept + "\n\n" if kept else "") + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
