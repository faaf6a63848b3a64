"""Index structure of a Shor list on the host and on the device (omc_shor_index_build, OMC_SHOR_INDEX_DEVICE_MIN):
(a) build time of where = 0 / where = 1 for the 2482-minor list of the branching instance (100 x 100) and config 3's class-4 list
    (200 x 200): one warm-up, then the median of five alternating pairs, and whether every array is equal;
(b) one append_shor with a new 2482-minor list to a held solve, knob 0 and knob 1 (what profiles/r12_shor_stream.txt section 2 left open);
(c) kernels launched per list against omc_shor_index_plan.
Prints one JSON line per measurement.  OMC_AMD_LIB points it at another build: a library without omc_shor_index_build (the parent commit)
gives the host figure alone, as the time of a stage_shor call minus that of the same call with an empty list."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import omc_amd          # noqa: E402

data = omc_amd.pkg.data
ARRAYS = ("mi", "kid", "cptr", "cent", "v1ptr", "v1ent", "v2ptr", "v2ent", "slackrow", "eclass", "ctype")
HAVE = hasattr(omc_amd.load(), "omc_shor_index_build")


def med(v):
    return float(np.median(v))


def build_times(name, eng, minors):
    if not HAVE:      # the parent commit: the host build inside stage_shor, against the same call without minors
        P = omc_amd.default_params(max_iters=1, slots=1)
        full, empty = [], []
        for _ in range(6):
            t0 = time.perf_counter(); eng.stage_shor([[]], [(minors, None)], "linear", P); full.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); eng.stage_shor([[]], [(minors[:0], None)], "linear", P); empty.append(time.perf_counter() - t0)
        print(json.dumps(dict(probe="build", list=name, minors=int(len(minors)), stage_ms=round(med(full[1:]) * 1e3, 3),
                              stage_empty_ms=round(med(empty[1:]) * 1e3, 3), host_ms_by_difference=round((med(full[1:]) - med(empty[1:])) * 1e3, 3))), flush=True)
        return
    h = eng.shor_index(minors, None, where="host"); d = eng.shor_index(minors, None, where="device")      # warm-up, and the identity
    equal = all(np.array_equal(h[key], d[key]) for key in ARRAYS) and (h["nv1"], h["nv2"]) == (d["nv1"], d["nv2"])
    th, td = [], []
    for _ in range(5):
        t0 = time.perf_counter(); eng.shor_index(minors, None, where="host"); th.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); eng.shor_index(minors, None, where="device"); td.append(time.perf_counter() - t0)
    plan = eng.shor_index_plan(len(minors))
    print(json.dumps(dict(probe="build", list=name, minors=int(len(minors)), equal=bool(equal), host_ms=round(med(th) * 1e3, 3),
                          device_ms=round(med(td) * 1e3, 3), note="both include the copy of the arrays back to numpy", launches=d["launches"],
                          plan_launches=plan["launches"], passes=[plan[key] for key in ("passes_v1", "passes_v2", "passes_coord", "passes_dup")],
                          scratch_bytes=plan["scratch_bytes"])), flush=True)


def append_time(eng, minors):
    """two-slot batch of the branching instance's root with half the list, held open; one append of a node with the whole list (new to the batch)"""
    P = omc_amd.default_params(rho_scale=1.0, eps_gap=1e-5, max_iters=300, slots=2)
    half = minors[:len(minors) // 2]
    for knob in (("0", "1", "0", "1", "0", "1") if HAVE else ("0", "0", "0")):
        if HAVE:
            eng.tuning_set("OMC_SHOR_INDEX_DEVICE_MIN", knob)
        eng.tuning_set("OMC_NO_GRAPH", "1")
        eng.reserve(1, 0); eng.reserve_shor(len(minors), 1)
        eng.stage_shor([[]], [(half, None)], "linear", P)
        eng.hold(True); eng.submit()
        time.sleep(0.05)
        t0 = time.perf_counter(); eng.append_shor([[]], [(minors, None)], "linear"); t = time.perf_counter() - t0
        eng.hold(False); eng.wait()
        st = eng.shor_index_stats() if HAVE else {}
        print(json.dumps(dict(probe="append", knob=knob, minors=int(len(minors)), append_ms=round(t * 1e3, 3), stats=st)), flush=True)
    if HAVE:
        eng.tuning_set("OMC_SHOR_INDEX_DEVICE_MIN", None)
    eng.tuning_set("OMC_NO_GRAPH", None)


def main():
    A, mask = data.branching_instance(seed=0)
    eng = omc_amd.Engine(A, mask, 80.0, 1)
    mi = eng.generate_rank1_matrix_completion_Shor_constraints_indexes([4])
    build_times("branching 100x100", eng, mi)
    append_time(eng, mi)
    eng.close()
    if os.environ.get("SKIP_CONFIG3"):
        return
    A3, mask3, g3, _ = data.config_instance(3, seed=0)
    e3 = omc_amd.Engine(A3, mask3, g3, 1)
    mi3 = e3.generate_rank1_matrix_completion_Shor_constraints_indexes([4])
    build_times("config 3 200x200", e3, mi3)
    e3.close()


if __name__ == "__main__":
    main()
