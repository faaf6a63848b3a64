"""The event records of the solve loop (EventTape, csrc/omc_events.h): with OMC_EVENT_MERGE=1 a timed iteration shares the events that
mark the same point of a stream and forks and joins on the timing events; with 0 it records every one, in the order before the tape.
Only the records differ, so every result must be bit-identical and every launch and unit count equal -- between the two settings and,
with OMC_PARENT_LIB naming another build of the library (the parent commit's), against that build.  Each arm is a child process with
OMC_GRAPH_MAX=0 and OMC_TIMING_STRIDE=1 in its environment.

Shapes: the 24 x 30 rank-1 instance of smoke(): root, children, grandchildren ... 20 nodes warm-started from their parents' pool entries
through 4 slots (harvests, refills, a drained tail); the same with accel = 1, on one stream, and with every 8th iteration timed (check_every
24, so that every interval is sampled alike); ten nodes appended to a solve that has run dry (tests/test_solve_loop.py); the 70 x 72 root
and its children warm from the root (tests/test_async_harvest.py: intervals that run split and intervals that run quiet); the 10 x 12
Shor program without minors (tests/test_gpu_shor.py).  A node costs milliseconds.

The record counter (Engine.event_counts()) of a solve equals what tests/event_tape_model.py counts for the iterations it ran -- the
model is a restatement of the enqueue order, fed with the solve's own launch counts -- and is below the unmerged count.  No timing
tolerance between the two paths is asserted (profiles/r18_event_tape.txt has the measured per-class ratios on these shapes)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0
HERE = os.path.dirname(os.path.abspath(__file__))
BASE_ENV = {"OMC_GRAPH_MAX": "0", "OMC_TIMING_STRIDE": "1"}
NEW_COUNTS = ("host/body_records", "host/body_waits")
# name -> what the model needs that the counts do not say: streams, stride, check_every, accel, shor, and the stride-1 twin to count iterations by
SCEN = {"base": dict(), "accel": dict(accel=1), "one_stream": dict(multi=False), "ce24": dict(check_every=24),
        "stride8": dict(check_every=24, stride=8, twin="ce24"), "appended": dict(), "quiet70": dict(), "shor": dict(shor=True)}


def _run(eng, nodes, P, env, **kw):
    for k_, v in env.items():
        eng.tuning_set(k_, v)
    try:
        return eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False, **kw)
    finally:
        for k_ in env:
            eng.tuning_set(k_, None)


def _stats(eng):
    ks = eng.kernel_stats()
    c = {"kernel/%s/%s" % (cls, f): v[f] for cls, v in ks.items() for f in ("launches", "units")}
    c.update({"host/%s" % name: v["count"] for name, v in eng.host_phases().items()})
    c.update({"host/body_%s" % name: v for name, v in eng.event_counts().items()})
    return c, {cls: v["ms"] for cls, v in ks.items()}, eng.solver_info()["solve_seconds"]


def _family(omc, eng):
    """Root, children, grandchildren ... in breadth-first order, 20 nodes; node i saves to pool entry i and loads from its parent's."""
    P = omc.default_params(rho_scale=4.0, max_iters=400, slots=4)
    eng.state_pool_create(20)
    nodes, parent = [[]], [-1]
    done = 0
    while done < len(nodes):      # one generation per solve, so that every parent's entry is filled before a child is staged
        gen = list(range(done, len(nodes)))
        res = _run(eng, [nodes[i] for i in gen], P, {}, load_from=[parent[i] for i in gen], save_to=gen)
        for i, o in zip(gen, res):
            if o["feasible"] and len(nodes) < 20:
                for kid in omc.pkg.bnb.make_children(nodes[i], o, "linear", 1):
                    if len(nodes) < 20:
                        nodes.append(kid); parent.append(i)
        done = gen[-1] + 1
    assert len(nodes) == 20
    return nodes, parent


def _appended(eng, nodes, P):
    eng.reserve(len(nodes) - 2, 6)
    eng.stage(nodes[:2], "linear", P)
    eng.hold(True)
    eng.submit()
    t0 = time.monotonic()
    while eng.poll()["nodes_done"] < 2:
        assert time.monotonic() - t0 < 60.0
        time.sleep(0.0005)
    eng.append(nodes[2:], "linear")
    eng.hold(False)
    eng.wait()
    return eng.fetch(want_X=False)


def _scenarios(omc, orc):
    out = {}
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, 24, 30, int(0.35 * 24 * 30), seed=3)
    eng = omc.Engine(A, mask, GAMMA, 1)
    nodes, parent = _family(omc, eng)
    kw = dict(load_from=parent)
    P4 = dict(rho_scale=4.0, max_iters=400, slots=4)
    out["base"] = (_run(eng, nodes, omc.default_params(**P4), {}, **kw), _stats(eng))
    out["accel"] = (_run(eng, nodes, omc.default_params(accel=1, **P4), {}, **kw), _stats(eng))
    out["one_stream"] = (_run(eng, nodes, omc.default_params(**P4), {"OMC_STREAMS": "1"}, **kw), _stats(eng))
    out["ce24"] = (_run(eng, nodes, omc.default_params(check_every=24, **P4), {}, **kw), _stats(eng))
    out["stride8"] = (_run(eng, nodes, omc.default_params(check_every=24, **P4), {"OMC_TIMING_STRIDE": "8"}, **kw), _stats(eng))
    out["appended"] = (_appended(eng, [c[:6] for c in nodes[5:15]], omc.default_params(**P4)), _stats(eng))
    eng.close()
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, 70, 72, 1512, seed=0)
    eng = omc.Engine(A, mask, GAMMA, 1)
    eng.state_pool_create(1)
    root = _run(eng, [[]], omc.default_params(rho_scale=4.0, max_iters=1500), {}, save_to=[0])[0]
    n70 = [[]] + omc.pkg.bnb.make_children([], root, "linear", 1)
    out["quiet70"] = (_run(eng, n70, omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14), {}, load_from=[0] * len(n70)), _stats(eng))
    eng.close()
    A, mask = orc.make_instance(10, 12, 1, n_indices=60, seed=1, noise=0.3)
    eng = omc.Engine(A, mask, GAMMA, 1)
    out["shor"] = (eng.matrix_completion_SDP_relaxation([[]], "linear", omc.default_params(eps_gap=1e-6), add_Shor_valid_inequalities=True,
                                                        shor_info=[([], None)], want_Theta=True), _stats(eng))
    eng.close()
    return out


def _flat(scen):
    flat = {}
    for name, (res, (counts, ms, seconds)) in scen.items():
        flat[name + "/n"] = np.asarray(len(res))
        for i, o in enumerate(res):
            for key, v in o.items():
                if key != "solve_time" and isinstance(v, (bool, int, float, np.ndarray, np.generic)):
                    flat["%s/%d/%s" % (name, i, key)] = np.asarray(v)
        for key, v in counts.items():
            flat["%s/count/%s" % (name, key)] = np.asarray(v)
        for key, v in ms.items():
            flat["%s/ms/%s" % (name, key)] = np.asarray(v)
        flat[name + "/seconds"] = np.asarray(seconds)
    return flat


def _child(out, env):
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=dict(os.environ, **BASE_ENV, **env), timeout=300)
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def arms(omc, tmp_path_factory):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    d = tmp_path_factory.mktemp("event_tape")
    return {m: _child(str(d / ("merge%s.npz" % m)), {"OMC_EVENT_MERGE": m}) for m in ("1", "0")}


def _timing(key):
    return "/ms/" in key or key.endswith("/seconds")


def _equal_but(a, b, skip):
    assert sorted(a) == sorted(b)
    for key, v in a.items():
        if not _timing(key) and not key.endswith(skip):
            assert np.array_equal(v, b[key], equal_nan=True), (key, v, b[key])


def test_merged_and_unmerged_agree(arms):
    """Every scalar and array of every node, the launches and units of every class, the counts of every host phase: only the records differ."""
    _equal_but(arms["1"], arms["0"], ("host/body_records",))
    for name in SCEN:
        assert int(arms["1"][name + "/n"]) >= 1
    for name in ("base", "accel"):      # the path does occur: refills of harvested slots, several checks
        assert int(arms["1"][name + "/count/kernel/setup/units"]) == 4 + 16 and int(arms["1"][name + "/count/kernel/harvest/launches"]) >= 3
    a = arms["1"]
    split = int(a["quiet70/count/kernel/cone/launches"]) - int(a["quiet70/count/kernel/global/launches"])
    print("quiet70: split iterations", split, "quiet intervals", int(a["quiet70/count/host/quiet_intervals"]))
    assert split > 0 and int(a["quiet70/count/host/quiet_intervals"]) >= 1


def test_against_another_build(arms, tmp_path):
    parent = os.environ.get("OMC_PARENT_LIB")
    if not parent:
        pytest.skip("OMC_PARENT_LIB is not set: no other build to compare with")
    z = _child(str(tmp_path / "parent.npz"), {"OMC_AMD_LIB": parent})
    for m in ("1", "0"):
        _equal_but(arms[m], z, NEW_COUNTS)


def test_every_launched_class_is_timed(arms):
    a = arms["1"]
    for name in SCEN:
        for key in a:
            if key.startswith(name + "/count/kernel/") and key.endswith("/launches") and int(a[key]) > 0:
                cls = key.split("/")[3]
                assert float(a["%s/ms/%s" % (name, cls)]) > 0, (name, cls)
    # one stream: the launches follow each other, so their times add up to no more than the solve
    total = sum(float(v) for key, v in a.items() if key.startswith("one_stream/ms/"))
    print("one stream: classes", total, "ms of", 1e3 * float(a["one_stream/seconds"]))
    assert 0 < total <= 1e3 * float(a["one_stream/seconds"])


@pytest.mark.parametrize("name", sorted(SCEN))
def test_record_counter_equals_the_model(arms, name):
    from event_tape_model import solve_counts
    spec = SCEN[name]
    got = {m: (int(arms[m][name + "/count/host/body_records"]), int(arms[m][name + "/count/host/body_waits"])) for m in ("1", "0")}
    twin = spec.get("twin", name)      # a stride-1 solve of the same nodes: every iteration is one counted launch of k_global
    cnt = lambda cls: int(arms["1"]["%s/count/kernel/%s/launches" % (twin, cls)])
    iters, ce = cnt("global"), spec.get("check_every", 25)
    assert iters % ce == 0      # a solve ends at a check
    shor = spec.get("shor", False)
    split_iters = 0 if shor else cnt("cone") - iters
    assert split_iters % ce == 0
    kw = dict(multi=spec.get("multi", True), iters=iters, check_every=ce, stride=spec.get("stride", 1), split_intervals=split_iters // ce,
              split_solve=split_iters > 0, shor=shor, accel=bool(spec.get("accel", 0)), sub=cnt("cone_sub") > 0,
              big_sub=shor and cnt("shor_bigcone") == 2 * iters)
    want = {m: solve_counts(m == "1", **kw) for m in ("1", "0")}
    print(name, kw, "records merged / unmerged", got["1"][0], got["0"][0], "waits", got["1"][1])
    assert got == want
    assert got["1"][0] < got["0"][0] and got["1"][1] == got["0"][1]


def test_per_class_ratio_is_reported(arms):
    """No assertion on times: the per-class ratio merged / unmerged of the base solve, for the profile."""
    for key in sorted(arms["1"]):
        if key.startswith("base/ms/") and float(arms["0"][key]) > 0:
            print(key, "%.3f ms / %.3f ms = %.3f" % (float(arms["1"][key]), float(arms["0"][key]), float(arms["1"][key]) / float(arms["0"][key])))
    print("base/seconds", float(arms["1"]["base/seconds"]), float(arms["0"]["base/seconds"]))


if __name__ == "__main__":      # a child process: every scenario on the library and with the knobs its environment names
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import omc_amd
    import omc_oracle
    np.savez(sys.argv[1], **_flat(_scenarios(omc_amd, omc_oracle)))
