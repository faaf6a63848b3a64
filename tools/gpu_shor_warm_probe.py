"""What the Shor-mode warm start buys (profiles/r10_shor_warm.txt).

  --part children   branching instance (100 x 100 rank 1, noise 0.3, 10 % observed; class-4 list, big cone of order 200): the Shor root,
                    then both children cold and from the root's pool entry, in one process: iterations, shor_bigcone ms, wall time.
  --part driver     config 1 with the class-4 Shor inequalities: bnb.branch_and_bound for a fixed time with shor_warm_start off and on,
                    alternating, two pairs: nodes relaxed and the bound.
Output: stdout, and the file given with --out (the two parts together are profiles/r10_shor_warm.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import omc_amd  # noqa: E402

bnb, data = omc_amd.pkg.bnb, omc_amd.pkg.data
ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("children", "driver"), required=True)
ap.add_argument("--seconds", type=float, default=60.0)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--max-iters", type=int, default=6000)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
OUT = None
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    OUT = open(args.out, "w")


def say(*a):
    print(*a, flush=True)
    if OUT:
        print(*a, file=OUT, flush=True)


def one(eng, name, cuts, mi, P, lf=None, sv=None):
    eng.stage_shor([cuts], [(mi, None)], "linear", P, load_from=lf, save_to=sv)
    t0 = time.time(); eng.solve(); t = time.time() - t0
    r = eng.fetch(want_Y=False, want_X=False)[0]
    ks = eng.kernel_stats()["shor_bigcone"]
    say(name, json.dumps(dict(iters=r["iters"], status=r["status_code"], objective=r["objective"], dual_bound=r["dual_bound"], wall_s=round(t, 3),
                              shor_bigcone_ms=round(ks["ms"], 1), ms_per_iter=round(1e3 * t / max(r["iters"], 1), 3), warm=eng.shor_warm_stats())))
    return r


if args.part == "children":
    A, mask = data.branching_instance(seed=0)
    eng = omc_amd.Engine(A, mask, 80.0, 1)
    mi = eng.generate_rank1_matrix_completion_Shor_constraints_indexes([4])
    say("branching instance", A.shape, "minors", len(mi), "big cone order", sum(A.shape))
    P = omc_amd.default_params(rho_scale=1.0, eps_gap=1e-5, max_iters=args.max_iters)
    eng.tuning_set("OMC_GRAPH_MAX", "0")      # eager launches: per-kernel event timing is not available inside a replayed graph
    eng.state_pool_create(4); eng.state_pool_reserve_shor(len(mi))
    root = one(eng, "root cold (saved)", [], mi, P, sv=[0])
    kids = bnb.make_children([], root, "linear", 1)
    for d, cuts in zip(("left", "right"), kids):
        c = one(eng, f"{d} cold", cuts, mi, P)
        w = one(eng, f"{d} warm", cuts, mi, P, lf=[0])
        say(f"{d}: |objective warm - cold| / max(1, |cold|) = {abs(w['objective'] - c['objective']) / max(1.0, abs(c['objective'])):.2e}")
    eng.close()
else:
    A, mask, _g, _c = data.config_instance(1, seed=0)
    eng = omc_amd.Engine(A, mask, 80.0, 1)
    say("config 1", A.shape, "class-4 minors", len(eng.generate_rank1_matrix_completion_Shor_constraints_indexes([4])))
    sp = omc_amd.default_params(rho_scale=1.0, eps_gap=1e-5, max_iters=3000, time_limit=15.0)
    for pair in range(2):
        for warm in (False, True):
            t0 = time.time()
            sol, inst = bnb.branch_and_bound(eng, A, mask, gap=1e-4, time_limit=args.seconds, batch=args.batch, add_Shor_valid_inequalities=True,
                                             Shor_valid_inequalities_noisy_rank1_num_entries_present=(4,), shor_params=sp, shor_warm_start=warm)
            rd = inst["run_details"]
            say(f"pair {pair} shor_warm_start={warm}", json.dumps(dict(
                seconds=round(time.time() - t0, 1), nodes_relaxed=rd["nodes_relax_feasible"] + rd["nodes_relax_infeasible"], nodes_explored=rd["nodes_explored"],
                lower=sol["lower_bound"], upper=sol["objective"], gap=sol["gap"], relax_s=round(rd["solve_time_relaxation"], 1),
                warm_started=rd.get("warm_started"), refused=rd.get("shor_warm_refused"), outgrown=rd.get("shor_warm_outgrown")), default=float))
    eng.close()
