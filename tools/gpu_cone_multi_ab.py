"""Spectral projection on its own (Engine.psd_project): the single-workgroup kernels (algo = 1) against the multi-workgroup kernels
(algo = 2) at orders 200, 400, 1000 (2000: algo = 2 alone), batch 1 and 8, cold and warm (V0 after a 1e-3 and a 1e-5 relative perturbation
of the matrix).  Four alternating pairs per cell; medians of the device milliseconds of the kernels (Engine.cone_multi_stats) and the
sweeps of the slowest matrix of a call.  Matrix: the spectrum of the big cone of a Shor root.  ORDERS=200,400 restricts the orders;
the table is printed and written to OUT (default profiles/r09_cone_multi.txt) as the section that starts at the line MARK: what the file
holds before that line (sweep counts, errors, solver figures) is kept.  The milliseconds are the kernels of a call alone, between two events
on the stream; what omc_psd_project_batch does on the host around them (staging and transfers of the N x N arrays) is outside."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omc_amd  # noqa: E402

PAIRS = 4
MARK = "== tools/gpu_cone_multi_ab.py =="


def shor_like(N, rng):
    lam = np.concatenate([[67.9, 0.038], -np.geomspace(7e-4, 8.5, N - 2)])
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    return (Q * lam) @ Q.T


def perturbed(M, eps, rng):
    G = rng.standard_normal(M.shape[-2:]); E = (G + G.T) / 2
    return M + eps * np.linalg.norm(M) * E / np.linalg.norm(E)


def call(eng, M, algo, V0):
    eng.psd_project(M, algo=algo, V0=V0)
    st = eng.cone_multi_stats()
    assert st["exhausted"] == 0, st
    return st["device_us"] / 1000.0, st["last_sweeps"]


def main():
    orders = [int(x) for x in os.environ.get("ORDERS", "200,400,1000,2000").split(",")]
    A, mask = omc_amd.pkg.data.generate_matrix_completion_data(1, 8, 10, 40, seed=1)
    eng = omc_amd.Engine(A, mask, 80.0, 1)
    lines = []

    def emit(t):
        print(t, flush=True); lines.append(t)
    emit("order  batch  start        algo 1: ms (min..max) sweeps    algo 2: ms (min..max) sweeps    ratio 1/2   fp64 peak fraction (algo 2)")
    for N in orders:
        for B in (1, 8):
            if N >= 2000 and B > 1:
                continue
            rng = np.random.default_rng(N + B)
            M = np.stack([shor_like(N, rng) for _ in range(B)])
            V = eng.psd_project(M, algo=2, want_V=True)[1]
            for name, eps in (("cold", None), ("warm 1e-3", 1e-3), ("warm 1e-5", 1e-5)):
                M2 = M if eps is None else np.stack([perturbed(M[b], eps, rng) for b in range(B)])
                V0 = None if eps is None else V
                t1, t2, s1, s2 = [], [], 0, 0
                for _ in range(PAIRS):
                    if N <= 1024:
                        ms, s1 = call(eng, M2, 1, V0); t1.append(ms)
                    ms, s2 = call(eng, M2, 2, V0); t2.append(ms)
                m2 = float(np.median(t2))
                # flops of the projection as VERDICT counts them: 4 N^3 per sweep of rotations, 2 N^3 each for G and the rebuild
                frac = B * (4.0 * s2 + 4.0) * N ** 3 / (m2 * 1e-3) / 78.6e12
                if t1:
                    m1 = float(np.median(t1))
                    emit(f"{N:>5d}  {B:>5d}  {name:<10}  {m1:>9.3f} ({min(t1):.3f}..{max(t1):.3f}) {s1:>3d}    {m2:>9.3f} ({min(t2):.3f}..{max(t2):.3f}) {s2:>3d}    {m1 / m2:>8.2f}   {frac:.4f}")
                else:
                    emit(f"{N:>5d}  {B:>5d}  {name:<10}  {'-':>30}    {m2:>9.3f} ({min(t2):.3f}..{max(t2):.3f}) {s2:>3d}    {'-':>8}   {frac:.4f}")
    eng.close()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r09_cone_multi.txt"))
    kept = open(out).read().split(MARK)[0].rstrip("\n") if os.path.exists(out) else ""
    with open(out, "w") as f:
        f.write((kept + "\n\n" if kept else "") + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
