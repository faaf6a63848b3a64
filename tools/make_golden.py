"""Generate tests/golden/*.npz: inputs (A, mask, gamma, k, cut lists) and the oracle's outputs.
The reference (Julia + Mosek) cannot run in this environment and ships no fixtures, so these vectors come from the
in-repo oracle (oracle/omc_oracle.py), each certified by its duality gap; they pin oracle and HIP path against
regressions and against each other."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import omc_oracle as orc

CASES = [
    dict(name="readme_20x24_k1_linear", n=20, m=24, k=1, kind="readme", seed=11, cut_type="linear", rho_scale=16.0, depth=4),
    dict(name="lowrank_24x28_k1_linear2", n=24, m=28, k=1, kind="lowrank", seed=12, cut_type="linear2", rho_scale=4.0, depth=4),
    dict(name="lowrank_16x20_k2_linear3", n=16, m=20, k=2, kind="lowrank", seed=13, cut_type="linear3", rho_scale=4.0, depth=3),
]

def main():
    out_dir = os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    for c in CASES:
        A, mask = orc.make_instance(c["n"], c["m"], c["k"], seed=c["seed"], kind=c["kind"],
                                    n_indices=None if c["kind"] == "readme" else int(0.4 * c["n"] * c["m"]))
        inst = orc.Instance(A, mask, 80.0, c["k"])
        rng = np.random.default_rng(c["seed"])
        dirs = orc.child_directions(c["cut_type"], c["k"])
        cuts = []; recs = []
        for d in range(c["depth"] + 1):
            r = orc.sdp_relaxation(inst, cuts, c["cut_type"], params=orc.RelaxParams(rho_scale=c["rho_scale"]))
            x, ev = orc.breakpoint_vector(r["Y"], r["U"])
            recs.append(dict(L=len(cuts), objective=r["objective"], dual_bound=r["dual_bound"], status=r["termination_status"],
                             iters=r["iters"], lmin=ev[0], eval_obj=orc.evaluate_objective(r["X"], A, mask, 80.0)))
            print(c["name"], d, recs[-1])
            # avoid the degenerate inner pieces when the parent's v-hat is ~0 (interval [-a, a] with a ~ 0: no Slater point)
            vhat = r["U"].T @ x
            ok = [d_ for d_ in dirs if all((abs(vhat[j]) > 0.05) or (d_[j] in ("left", "right")) for j in range(c["k"]))]
            dr = ok[int(rng.integers(len(ok)))]
            cuts = cuts + [(x, r["U"].copy(), dr)]
        L = len(cuts)
        np.savez_compressed(os.path.join(out_dir, c["name"] + ".npz"),
                            A=A, mask=mask, gamma=80.0, k=c["k"], cut_type=c["cut_type"], rho_scale=c["rho_scale"],
                            cut_x=np.stack([q[0] for q in cuts]), cut_U=np.stack([q[1] for q in cuts]),
                            cut_dir=np.array([[orc.DIR_CODES[s] for s in q[2]] for q in cuts], dtype=np.int8),
                            node_L=np.array([r["L"] for r in recs]), objective=np.array([r["objective"] for r in recs]),
                            dual_bound=np.array([r["dual_bound"] for r in recs]), status=np.array([r["status"] for r in recs]),
                            iters=np.array([r["iters"] for r in recs]), lmin=np.array([r["lmin"] for r in recs]),
                            eval_obj=np.array([r["eval_obj"] for r in recs]))

# Ranks 3 to 8 ("Rank-k relaxation fixtures").  Every case: make_instance(kind="lowrank", noise=0.1) with n_obs observed cells,
# GAMMA = 80.  `dir_seed` seeds the per-column draw of the pieces; `breakpoints` is the separation rule that made the cut vectors;
# `q1` is RelaxParams.reference_quirk_q1.  A prefix of the cut path becomes a node of the fixture only when the oracle certified it.
RANK_K_CASES = [
    dict(name="lowrank_16x20_k3_linear", n=16, m=20, k=3, n_obs=110, seed=21, cut_type="linear", rho_scale=4.0, depth=9,
         breakpoints="smallest_1_eigvec", q1=True, dir_seed=3),
    dict(name="lowrank_16x20_k4_linear3", n=16, m=20, k=4, n_obs=150, seed=21, cut_type="linear3", rho_scale=4.0, depth=8,
         breakpoints="smallest_1_eigvec", q1=False, dir_seed=3),
    dict(name="lowrank_16x20_k5_linear2", n=16, m=20, k=5, n_obs=200, seed=21, cut_type="linear2", rho_scale=4.0, depth=9,
         breakpoints="smallest_1_eigvec", q1=True, dir_seed=3),
    dict(name="lowrank_20x26_k8_linear2", n=20, m=26, k=8, n_obs=380, seed=21, cut_type="linear2", rho_scale=4.0, depth=9,
         breakpoints="smallest_2_eigvec", q1=True, dir_seed=3),
]


def rank_k_path(c, log=print):
    """Walk one cut path of `c["depth"]` levels with the oracle; returns (A, mask, cuts, recs), recs[d] = the node with the first d cuts."""
    A, mask = orc.make_instance(c["n"], c["m"], c["k"], seed=c["seed"], kind="lowrank", n_indices=c["n_obs"], noise=0.1)
    inst = orc.Instance(A, mask, 80.0, c["k"])
    rng = np.random.default_rng(c["dir_seed"])
    labels = orc.DIRECTIONS_OF[c["cut_type"]]
    P = orc.RelaxParams(rho_scale=c["rho_scale"], reference_quirk_q1=c["q1"])
    cuts = []; recs = []
    for d in range(c["depth"] + 1):
        r = orc.sdp_relaxation(inst, cuts, c["cut_type"], params=P, want_certificate=False)
        x, _ = orc.breakpoint_vector(r["Y"], r["U"], c["breakpoints"])
        _, ev = orc.breakpoint_vector(r["Y"], r["U"])
        kinds = np.array(r["rows"].kinds)
        recs.append(dict(L=len(cuts), R=len(r["rows"]), r=r["Q"].shape[1], n_active=int(((r["lam"] > 1e-9) & (kinds != "trace")).sum()),
                         lam=r["lam"].copy(), objective=r["objective"], dual_bound=r["dual_bound"], status=r["termination_status"],
                         iters=r["iters"], lmin=ev[0], eval_obj=orc.evaluate_objective(r["X"], A, mask, 80.0)))
        log(c["name"], {k_: v for k_, v in recs[-1].items() if k_ != "lam"})
        # one piece per column (the full product has up to 4^8 members); the inner pieces need |v-hat| away from 0, as in main()
        vhat = r["U"].T @ x
        dr = []
        for j in range(c["k"]):
            ok = [s for s in labels if abs(vhat[j]) > 0.05 or s in ("left", "right")]
            dr.append(ok[int(rng.integers(len(ok)))])
        cuts = cuts + [(x, r["U"].copy(), dr)]
    return A, mask, cuts[:-1], recs


def check_rank_k_conditions(name, recs):
    """Condition 1 of the rank-k fixtures (active cuts, a moved objective), on the oracle alone; returns the certified nodes.
    tests/test_rank_k_cpu.py asserts the conditions again from the stored arrays."""
    listed = [q for q in recs if q["status"] == 0]
    assert listed and listed[0]["L"] == 0, (name, "the root must certify")
    root = listed[0]["objective"]
    moved = [q for q in listed if q["n_active"] >= 3 and q["objective"] > root * (1.0 + 1e-3)]
    assert len(moved) >= 2, (name, "fewer than two certified nodes with active cut rows and a moved objective")
    return listed


def make_rank_k_golden(names=None):
    out_dir = os.path.join(ROOT, "tests", "golden")
    seen = []
    for c in RANK_K_CASES:
        if names and c["name"] not in names:
            continue
        A, mask, cuts, recs = rank_k_path(c)
        listed = check_rank_k_conditions(c["name"], recs)
        seen += [(c["k"], q["L"], q["r"], q["R"]) for q in listed]
        cuts = cuts[:listed[-1]["L"]]                    # cuts past the deepest certified node are of no use to a test
        Rmax = max(q["R"] for q in listed)
        lam = np.zeros((len(listed), Rmax))
        for b, q in enumerate(listed):
            lam[b, :q["R"]] = q["lam"]
        col = lambda key, src=listed: np.array([q[key] for q in src])
        np.savez_compressed(os.path.join(out_dir, c["name"] + ".npz"),
                            A=A, mask=mask, gamma=80.0, k=c["k"], cut_type=c["cut_type"], rho_scale=c["rho_scale"],
                            breakpoints=c["breakpoints"], reference_quirk_q1=c["q1"],
                            cut_x=np.stack([q[0] for q in cuts]), cut_U=np.stack([q[1] for q in cuts]),
                            cut_dir=np.array([[orc.DIR_CODES[s] for s in q[2]] for q in cuts], dtype=np.int8),
                            node_L=col("L"), objective=col("objective"), dual_bound=col("dual_bound"), status=col("status"),
                            iters=col("iters"), lmin=col("lmin"), eval_obj=col("eval_obj"),
                            R=col("R"), r=col("r"), n_active=col("n_active"), lam=lam,
                            path_status=col("status", recs), path_iters=col("iters", recs), path_objective=col("objective", recs),
                            path_n_active=col("n_active", recs))
    if not names:       # condition 2 spans the fixtures
        assert any(r_ >= 17 for _, _, r_, _ in seen), "no certified node beyond the r = 16 boundary of k_small"
        assert any(k_ == 8 and r_ <= 16 and L >= 2 and R >= 71 for k_, L, r_, R in seen), "no certified rank-8 node with r <= 16 and R >= 71"


def make_shor_golden():
    """Shor-minor fixtures (integer work): mask, X and the oracle's index lists / top violated minors."""
    out_dir = os.path.join(ROOT, "tests", "golden")
    rng = np.random.default_rng(77)
    n, m, k = 9, 13, 2
    mask = rng.random((n, m)) < 0.45
    mask[rng.integers(0, n, m), np.arange(m)] = True; mask[np.arange(n), rng.integers(0, m, n)] = True
    X3 = np.round(rng.standard_normal((k, n, m)) * 4) / 4          # quarter-integers: exact products, many tied scores
    rec = dict(mask=mask, X3=X3, A=rng.standard_normal((n, m)))
    for p in (4, 3, 2, 1, 0):
        rec["idx_%d" % p] = np.array(orc.shor_constraints_indexes(mask, [p]), dtype=np.int64).reshape(-1, 4)
    rec["idx_2_4"] = np.array(orc.shor_constraints_indexes(mask, [2, 4]), dtype=np.int64).reshape(-1, 4)
    first = orc.violated_shor_minors(X3, mask, [4, 3], [], 12)
    existing = np.array([t for _, t in first[:6]], dtype=np.int64)
    second = orc.violated_shor_minors(X3, mask, [4, 3], [tuple(int(v) for v in t) for t in existing], 12)
    rec["existing"] = existing
    for nm, lst in (("first", first), ("second", second)):
        rec[nm + "_scores"] = np.array([s for s, _ in lst]); rec[nm + "_minors"] = np.array([t for _, t in lst], dtype=np.int64)
    np.savez_compressed(os.path.join(out_dir, "shor_9x13_k2.npz"), **rec)
    print("shor fixture:", {k_: v.shape for k_, v in rec.items()})


def make_colprox_block_golden():
    """The oracle's certified root of the 130 x 132 instance of tests/test_colprox_block.py (minutes on a CPU: recorded, not recomputed per run)."""
    import json
    n, m, frac, seed = 130, 132, 0.97, 5
    rng = np.random.default_rng(seed)
    mask = rng.random((n, m)) < frac
    mask[0, :] = True; mask[:, 0] = True
    A = (rng.standard_normal((n, 1)) @ rng.standard_normal((1, m)) + 0.01 * rng.standard_normal((n, m))) * mask
    ref = orc.sdp_relaxation(orc.Instance(A, mask, 80.0, 1), [], "linear", params=orc.RelaxParams(rho_scale=4.0))
    rec = dict(n=n, m=m, frac=frac, seed=seed, gamma=80.0, k=1, rho_scale=4.0, sum_A=float(A.sum()), nnz=int(mask.sum()),
               objective=float(ref["objective"]), dual_bound=float(ref["dual_bound"]), termination_status=int(ref["termination_status"]))
    json.dump(rec, open(os.path.join(ROOT, "tests", "golden", "colprox_block_root_130x132.json"), "w"), indent=1)
    print("colprox block fixture:", rec)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "colprox":
        make_colprox_block_golden()
    elif len(sys.argv) > 1 and sys.argv[1] == "shor":
        make_shor_golden()
    elif len(sys.argv) > 1 and sys.argv[1] == "rank_k":      # optionally followed by fixture names; without them condition 2 is checked too
        make_rank_k_golden(sys.argv[2:])
    else:
        main(); make_shor_golden(); make_rank_k_golden()
