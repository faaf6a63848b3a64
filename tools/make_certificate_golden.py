"""Generate tests/golden/certificate_paths.json: the cut paths and the oracle's results that tests/test_gpu_certificate.py reads.

The instances, seeds and paths are those of tests/test_gpu_parity.py::test_relaxation_matches_oracle (make_instance(seed=21),
oracle_path(seed=3), gamma = 80).  The oracle needs a minute for them (the rank-2 nodes run to the iteration cap), which no GPU test should
spend, so they are recorded once: per shape the cuts of the deepest node (node d of the path is its first d cuts) and, per node, the
oracle's status, objective and dual bound."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import omc_oracle as orc
from test_gpu_parity import oracle_path

DIRS = ["left", "middle", "right", "inner_left", "inner_right"]
SHAPES = [(12, 15, 1, "readme", "linear", 8.0, 2), (16, 20, 2, "lowrank", "linear3", 4.0, 2), (24, 30, 1, "lowrank", "linear2", 4.0, 3)]


def main():
    out = {}
    for s, (n, m, k, kind, cut_type, rho_scale, depth) in enumerate(SHAPES):
        A, mask = orc.make_instance(n, m, k, seed=21, kind=kind, n_indices=None if kind == "readme" else int(0.35 * n * m))
        inst = orc.Instance(A, mask, 80.0, k)
        nodes = oracle_path(orc, inst, cut_type, depth, rho_scale, seed=3)
        ref = [orc.sdp_relaxation(inst, c, cut_type, params=orc.RelaxParams(rho_scale=rho_scale), want_certificate=False) for c in nodes]
        cuts = nodes[-1]
        out[f"s{s}_x"] = np.stack([c[0] for c in cuts]); out[f"s{s}_U"] = np.stack([np.asarray(c[1]).reshape(n, k) for c in cuts])
        out[f"s{s}_dir"] = np.array([[DIRS.index(d) for d in c[2]] for c in cuts], dtype=np.int8)
        out[f"s{s}_status"] = np.array([r["termination_status"] for r in ref], dtype=np.int32)
        out[f"s{s}_objective"] = np.array([r["objective"] for r in ref]); out[f"s{s}_dual_bound"] = np.array([r["dual_bound"] for r in ref])
        out[f"s{s}_A_sum"] = np.array([A.sum(), float(mask.sum())])      # the test regenerates the instance and checks it is this one
        print((n, m, k, cut_type), out[f"s{s}_status"], out[f"s{s}_objective"], out[f"s{s}_dual_bound"])
    with open(os.path.join(ROOT, "tests", "golden", "certificate_paths.json"), "w") as f:      # floats round-trip exactly; not *.npz, which tests/test_golden.py takes for its own
        json.dump({key: val.tolist() for key, val in out.items()}, f)


if __name__ == "__main__":
    main()
