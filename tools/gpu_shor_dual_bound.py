"""Device evaluator of Shor-mode certificates (Engine.shor_dual_bound, sanitise on) against the numpy checker (certificate.shor_dual_bound)
on the same multipliers: event time of the kernels alone, wall time of the call, wall time of numpy; one warm-up, then the median of REPS.
Cases: the 12 x 14 root with its 152 class-4 minors (exported certificate of its 1e-6 solve), the 100 x 100 root of BASELINE config 2 with
its class-4 list after ITERS iterations (as tools/gpu_shor_certificates_ab.py sets it up), and config 3's root list (200 x 200, class 4) if
omc_shor_dual_bound_plan fits the device -- there with multipliers of the recipe of test_random_multipliers_smoke, blocks scaled down so that
every mu_j stays positive (no solve: the time of either side does not depend on the values as long as the bound is finite).
With PARENT_LIB=<libomc_hip.so built from the parent commit> the default bench line is run first, parent library | this tree, in
alternating pairs with the dumped outputs compared bit for bit (bench_pairs of gpu_shor_certificates_ab.py).
Output: stdout and OUT (default profiles/r20_shor_dual_bound.txt), from the line MARK on."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import omc_amd  # noqa: E402
from gpu_shor_certificates_ab import bench_pairs  # noqa: E402

REPS = int(os.environ.get("REPS", 5))
ITERS = int(os.environ.get("ITERS", 400))
MARK = "== tools/gpu_shor_dual_bound.py =="


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t)


def measure(emit, name, eng, A, mask, gamma, minors, c):
    cert = omc_amd.pkg.certificate
    n, m = A.shape
    plan = eng.shor_dual_bound_plan(1, len(minors))
    emit(f"-- {name}: {n} x {m}, {len(minors)} minors; omc_shor_dual_bound_plan: {plan['bytes_total']} bytes ({plan['ways']} views, slab {plan['slab_doubles']} doubles)")
    try:
        eng.shor_dual_bound([[]], [(minors, None)], [c])                       # warm-up (allocations, code objects)
    except omc_amd.OmcError as err:
        emit(f"    not run: {err}")
        return
    ev, wall = [], []
    for _ in range(REPS):
        (dev, terms), ms = timed(lambda: eng.shor_dual_bound([[]], [(minors, None)], [c], want_terms=True))
        wall.append(ms); ev.append(eng.last_shor_dual_bound_ms())
    cert.shor_dual_bound(A, mask, gamma, [], "linear", minors, None, c)    # warm-up
    ref_ms = []
    for _ in range(REPS):
        ref, ms = timed(lambda: cert.shor_dual_bound(A, mask, gamma, [], "linear", minors, None, c))
        ref_ms.append(ms)
    med = lambda v: float(np.median(v))
    emit(f"    device {dev[0]!r} numpy {ref!r} difference {abs(dev[0] - ref):.3e}; terms (constant, eig, ||c||, min mu) {tuple(float(t) for t in terms[0])}")
    emit(f"    device kernels (events) {med(ev):.3f} ms ({min(ev):.3f}..{max(ev):.3f}) | device call (wall) {med(wall):.2f} ms ({min(wall):.2f}..{max(wall):.2f}) | "
         f"numpy (wall) {med(ref_ms):.1f} ms ({min(ref_ms):.1f}..{max(ref_ms):.1f}); median of {REPS} after one warm-up")
    emit(f"    numpy / device call {med(ref_ms) / med(wall):.1f}x, numpy / device kernels {med(ref_ms) / med(ev):.0f}x")


def exported(eng, minors, P):
    eng.keep_shor_certificates(True)
    r = eng.matrix_completion_SDP_relaxation([[]], "linear", P, add_Shor_valid_inequalities=True, shor_info=[(minors, None)], want_Y=False)[0]
    c = eng.fetch_shor_certificate([0])[0]
    eng.keep_shor_certificates(False)
    return r, c


def main():
    lines = []

    def emit(t):
        print(t, flush=True); lines.append(t)
    parent = os.environ.get("PARENT_LIB")
    if parent:
        bench_pairs(emit, parent)
    import omc_oracle as orc
    cert = omc_amd.pkg.certificate
    A, mask = orc.make_instance(12, 14, 1, n_indices=70, seed=2, noise=0.1)
    minors = orc.shor_constraints_indexes(mask, [4])
    eng = omc_amd.Engine(A, mask, 80.0, 1)
    r, c = exported(eng, minors, omc_amd.default_params(eps_gap=1e-6, max_iters=6000))
    measure(emit, f"12 x 14 root (status {r['status_code']}, {r['iters']} iterations)", eng, A, mask, 80.0, minors, c)
    eng.close()
    A, mask, gamma, _ = omc_amd.pkg.data.config_instance(2, seed=0)
    eng = omc_amd.Engine(A, mask, gamma, 1)
    minors = eng.generate_rank1_matrix_completion_Shor_constraints_indexes([4])
    r, c = exported(eng, minors, omc_amd.default_params(eps_gap=1e-5, max_iters=ITERS))
    measure(emit, f"config 2 root (status {r['status_code']}, {r['iters']} iterations)", eng, A, mask, gamma, minors, c)
    eng.close()
    A, mask, gamma, _ = omc_amd.pkg.data.config_instance(3, seed=0)
    n, m = A.shape
    eng = omc_amd.Engine(A, mask, gamma, 1)
    minors = eng.generate_rank1_matrix_completion_Shor_constraints_indexes([4])
    rng = np.random.default_rng(3)
    G = rng.standard_normal((len(minors), 5, 5))
    Gam = G @ np.transpose(G, (0, 2, 1))
    Gam *= 1e-5 / gamma / np.abs(Gam).max()
    Q = eng.row_basis([[]])[0]
    R = len(cert.node_rows(n, 1, [], "linear"))
    c = cert.ShorCertificate(scale=1.0, lam=np.abs(rng.standard_normal(R)) * 0.1, Q=Q, Psi3=np.zeros((Q.shape[1] + 1,) * 2), Gam=Gam,
                             zeta=rng.random(m) * 0.1 / gamma, xi=rng.standard_normal((n, m)) * 0.1, Xbar=rng.standard_normal((n, m)) * 0.1)
    measure(emit, "config 3 root list, random multipliers", eng, A, mask, gamma, minors, c)
    eng.close()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r20_shor_dual_bound.txt"))
    kept = open(out).read().split(MARK)[0].rstrip("\n") if os.path.exists(out) else ""
    with open(out, "w") as f:
        f.write((kept + "\n\n" if kept else "") + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
