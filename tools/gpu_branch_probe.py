"""Children by reference (Engine.append_children) against children from their cut lists (Engine.append), on the GPU.

  python tools/gpu_branch_probe.py calls     (a) host time per appended child, Python call to return: 100 x 100 k = 1 at depths 1, 11, 30 and
                                                 500 x 500 k = 2 at depths 1, 20; medians over REPS calls of 64 children each, while the held
                                                 solve is still relaxing the children of the calls before (64 slots busy: a call then waits
                                                 for its copies and kernels to get onto the device)
  python tools/gpu_branch_probe.py quiet     the same with every call made into an idle solve (the children of the call before have finished)
  python tools/gpu_branch_probe.py driver    (b) the queue-driven driver on the branching 100 x 100 instance, device_branching off / on in
                                                 alternating pairs: node-relaxations/s and the share of the wall time inside the append calls
Output: stdout, and the file named by OUT if it is set (profiles/device_branching.txt keeps a copy of the three modes)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import omc_amd

data, bs = omc_amd.pkg.data, omc_amd.pkg.bnb_stream
MODE = sys.argv[1] if len(sys.argv) > 1 else "calls"
REPS = int(os.environ.get("REPS", "7"))
TL = float(os.environ.get("TL", "20"))
PAIRS = int(os.environ.get("PAIRS", "2"))
OUT = open(os.environ["OUT"], "w") if os.environ.get("OUT") else None


def say(*a):
    print(*a, flush=True)
    if OUT is not None:
        print(*a, file=OUT, flush=True)


def wait_for(eng, res, ids):
    deadline = time.time() + 120
    while any(i not in res for i in ids):
        got = eng.fetch_done()
        for o in got:
            res[o["node"]] = o
        if not got:
            if time.time() > deadline:
                raise RuntimeError("the held solve did not return the nodes")
            time.sleep(0.001)


def calls(cfg, depths, quiet):
    """A chain root -> ... -> a node of depth d - 1 in one held solve (20 iterations per node: the descriptors do not care how far a node
    got), then REPS calls of each kind that append 64 children of that node."""
    A, mask, gamma, c = data.config_instance(cfg, seed=0)
    n, k, ct = c["n"], c["k"], c["cut_type"]
    plan = omc_amd.pkg.bnb.child_directions(ct, k)
    eng = omc_amd.Engine(A, mask, gamma, k)
    P = omc_amd.default_params(rho_scale=4.0, max_iters=20, check_every=10, early_stop_factor=0.0, slots=64)
    dmax = max(depths)
    eng.reserve(dmax + 2 * REPS * 64 * len(depths) + 8, dmax)
    eng.stage([[]], ct, P)
    eng.hold(True); eng.submit()
    res = {}
    wait_for(eng, res, [0])
    node, cuts = 0, []
    for d in range(1, dmax + 1):
        # children of `node` have depth d
        if d in depths:
            o = res[node]
            kids_host = [cuts + [(o["breakpoint_vec"], o["U"], plan[q % len(plan)])] for q in range(64)]
            t_host, t_dev = [], []
            dirs64 = [plan[q % len(plan)] for q in range(64)]

            def drain():
                if quiet:
                    wait_for(eng, res, range(eng.poll()["nodes_total"]))
            for _ in range(REPS):
                drain()
                t0 = time.perf_counter(); eng.append(kids_host, ct); t_host.append(time.perf_counter() - t0)
                drain()
                t0 = time.perf_counter(); eng.append_children([node] * 64, dirs64); t_dev.append(time.perf_counter() - t0)
            mh, md = np.median(t_host) / 64 * 1e6, np.median(t_dev) / 64 * 1e6
            say(json.dumps(dict(solve="idle" if quiet else "busy", n=n, k=k, cut_type=ct, depth=d, calls=REPS, children_per_call=64, append_us_per_child=round(mh, 1),
                                append_children_us_per_child=round(md, 1), ratio=round(mh / md, 1),
                                append_us_all=[round(t / 64 * 1e6, 1) for t in t_host], append_children_us_all=[round(t / 64 * 1e6, 1) for t in t_dev])))
        if d < dmax:
            nxt = eng.append_children([node], [plan[0]])[0]
            wait_for(eng, res, [nxt])
            cuts = cuts + [(res[node]["breakpoint_vec"], res[node]["U"], plan[0])]
            node = nxt
    eng.hold(False); eng.wait(); eng.close()


def driver():
    A, mask = data.branching_instance(seed=0)
    for pair in range(PAIRS):
        for on in (False, True):
            eng = omc_amd.Engine(A, mask, 80.0, 1)
            t0 = time.time()
            sol, inst = bs.branch_and_bound_streaming(eng, A, mask, gap=1e-4, time_limit=TL, slots=int(os.environ.get("SLOTS", "1024")), device_branching=on)
            wall = time.time() - t0
            rd = inst["run_details"]
            say(json.dumps(dict(pair=pair, device_branching=on, seconds=round(wall, 1), explored=rd["nodes_explored"], relaxed=rd["nodes_relax_feasible"],
                                relax_s=round(rd["solve_time_relaxation"], 2), nodes_per_s=round(rd["nodes_relax_feasible"] / max(rd["solve_time_relaxation"], 1e-9), 1),
                                append_s=round(rd["append_seconds"], 3), append_share_of_wall=round(rd["append_seconds"] / wall, 4),
                                by_reference=rd.get("nodes_appended_by_reference", 0), epochs=rd["epochs"], gap=sol["gap"]), default=float))
            eng.close()


if MODE in ("calls", "quiet"):
    calls(2, (1, 11, 30), MODE == "quiet")
    calls(4, (1, 20), MODE == "quiet")
else:
    driver()
