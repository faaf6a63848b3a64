"""Violated-minor selection, materialised keys (OMC_SHOR_SELECT_KB = 0) against the streaming path, on BASELINE configs 3 and 5: five
alternating runs each, medians of the device milliseconds (Engine.shor_last_stats).  Where the default budget would not stream, the
streaming run gets one sixteenth of the materialised key bytes (at least 1 MiB).  Results are compared for equality on the way."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omc_amd  # noqa: E402

DEFAULT_KB = 1 << 20
CARD_BYTES = 200e9          # keys beyond this are not attempted materialised


def run(eng, X3, cl, kb, nm=100):
    eng.tuning_set("OMC_SHOR_SELECT_KB", kb)
    top = eng.generate_violated_Shor_minors(X3, cl, [], nm)
    return top, eng.shor_last_stats(), eng.shor_last_select_stats()


def main():
    rng = np.random.default_rng(0)
    A3, mask3, g3, c3 = omc_amd.pkg.data.config_instance(3, seed=0)
    X3 = (A3 + 0.1 * rng.standard_normal(A3.shape))[None]
    A5, mask5, g5, c5 = omc_amd.pkg.data.config_instance(5, seed=0)
    r5 = np.random.default_rng(1); k5 = c5["k"]
    X5 = r5.standard_normal((k5, A5.shape[0], 1)) * r5.standard_normal((k5, 1, A5.shape[1])) + 0.05 * r5.standard_normal((k5,) + A5.shape)
    e3 = omc_amd.Engine(A3, mask3, g3, c3["k"]); e5 = omc_amd.Engine(A5, mask5, g5, k5)
    print("config  classes        candidates   materialised: ms  key bytes   streaming: budget KiB  ms  tiles  compactions  buffer bytes   ratio")
    for name, eng, X, cl in (("3", e3, X3, [4]), ("3", e3, X3, [4, 3]), ("3", e3, X3, [1, 2, 3, 4]), ("5", e5, X5, [4]), ("5", e5, X5, [1, 2, 3, 4])):
        N = int(sum(eng.shor_count(cl)))
        kb = DEFAULT_KB if 16 * N > DEFAULT_KB * 1024 else max(1024, 16 * N // 16 // 1024)
        both = 16 * N < CARD_BYTES
        run(eng, X, cl, kb)                                         # first call allocates
        ms0, ms1, sel0, sel1 = [], [], None, None
        for _ in range(5):
            if both:
                a, st, sel0 = run(eng, X, cl, 0); ms0.append(st["ms"])
            b, st, sel1 = run(eng, X, cl, kb); ms1.append(st["ms"])
            assert sel1["streamed"] == 1 and (not both or (sel0["streamed"] == 0 and a == b))
        m1 = float(np.median(ms1))
        if both:
            m0 = float(np.median(ms0))
            print(f"{name:>6}  {str(cl):<13} {N:>12d}   {m0:>16.3f}  {sel0['peak_bytes']:>9.3g}   {kb:>21d}  {m1:>8.3f}  {sel1['tiles']:>5d}  {sel1['compactions']:>11d}  {sel1['peak_bytes']:>12d}   {m1 / m0:.2f}")
        else:
            print(f"{name:>6}  {str(cl):<13} {N:>12d}   {'(keys: %.3g B)' % (16.0 * N):>27}   {kb:>21d}  {m1:>8.3f}  {sel1['tiles']:>5d}  {sel1['compactions']:>11d}  {sel1['peak_bytes']:>12d}   -")
    e3.close(); e5.close()


if __name__ == "__main__":
    main()
