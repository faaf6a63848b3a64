"""The host API against another build of the library, bit for bit, where the comparisons of test_solve_loop.py, test_between_iterations.py,
test_event_tape.py and test_altmin_steps.py do not reach: Shor staging with append and warm pool, the certificates and the two dual-bound
evaluators, the plain operations, and the staging branch of orders above 512.  OMC_PARENT_LIB names the other build (the parent commit's);
without it the module skips.  Both arms run in a child process each (this file as a script, the library chosen by OMC_AMD_LIB), every
returned number and array is compared with np.array_equal.

Shapes: the 12 x 14 / 152 minors instance of test_gpu_shor_certificate.py for three checks 500 iterations apart; the 24 x 30 instances of smoke() at
rank 1 and 2; matrices of order 16 and 160 for psd_project; one 520 x 530 node for two checks' worth of iterations.  A case costs a second or two."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0
SHOR_CHECK_EVERY = 500
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("shor", "shor_dual_bound", "base_certificates", "plain", "order520")
RESULT_KEYS = ("objective", "dual_bound", "status_code", "iters", "U", "lambda_min", "breakpoint_vec", "Y", "X", "W", "Theta")
SHOR_CERT_FIELDS = ("scale", "lam", "Q", "Psi3", "Gam", "zeta", "xi", "Xbar", "bound")
CERT_FIELDS = ("Lam", "lam", "Q", "Psi3", "bound")


def _put(flat, prefix, results, keys=RESULT_KEYS):
    for i, o in enumerate(results):
        for key in keys:
            if key in o:
                flat["%s/%d/%s" % (prefix, i, key)] = np.asarray(o[key])


def _wait_done(eng, count):
    t0 = time.monotonic()
    while eng.poll()["nodes_done"] < count:
        assert time.monotonic() - t0 < 60.0
        time.sleep(0.0005)


def _shor_cases(omc, orc, flat):
    """Shor 12 x 14, rank 1, static list: a held solve of the root, two appended children that load the root's saved state and save their
    own; fetch_done, fetch_done_shor, the pool entries, fetch_shor_certificate; then shor_dual_bound on those certificates, both ways."""
    import omc_oracle_shor as sh
    A, mask = orc.make_instance(12, 14, 1, n_indices=70, seed=2, noise=0.1)
    minors, _ = sh.driver_shor_lists(mask, (4,))
    eng = omc.Engine(A, mask, GAMMA, 1)
    root = eng.matrix_completion_SDP_relaxation([[]], "linear", params=omc.default_params(rho_scale=4.0), want_X=False)[0]
    kids = omc.pkg.bnb.make_children([], root, "linear", 1)[:2]
    # three checks: a Shor node's bound is -inf (no certificate) for its first hundreds of iterations, so the checks are 500 apart
    P = omc.default_params(eps_gap=1e-5, rho_scale=1.0, slots=2, check_every=SHOR_CHECK_EVERY, max_iters=3 * SHOR_CHECK_EVERY)
    eng.keep_shor_certificates(True)
    eng.state_pool_create(3)
    eng.state_pool_reserve_shor(len(minors))
    eng.reserve(2, 1)
    eng.reserve_shor(len(minors), 1)
    eng.stage_shor([[]], [(minors, None)], "linear", P, keep_V=True, save_to=[0])
    eng.hold(True)
    eng.submit()
    _wait_done(eng, 1)      # the loop has run dry and waits: the append below is found by the dry loop, whenever it lands
    done = eng.fetch_done(want_Y=True)
    eng.append_shor(kids, [(minors, None)] * 2, "linear", load_from=[0, 0], save_to=[1, 2])
    eng.hold(False)
    eng.wait()
    done += eng.fetch_done(want_Y=True)
    ids = [d["node"] for d in done]
    assert sorted(ids) == [0, 1, 2]
    _put(flat, "shor/fetch_done", sorted(done, key=lambda d: d["node"]))
    _put(flat, "shor/fetch_done_shor", eng.fetch_done_shor([0, 1, 2], want_W=True, want_Theta=True))
    res = eng.fetch(want_Y=True, want_X=True, want_Theta=True)
    for r, Wb, Vb in zip(res, eng.fetch_shor(), eng.fetch_shor_V()):
        r["W"] = Wb; r["V"] = Vb
    _put(flat, "shor/fetch", res, RESULT_KEYS + ("V",))
    flat["shor/warm_stats"] = np.asarray(sorted(eng.shor_warm_stats().items()), dtype=object).astype(str)
    for e in range(3):
        st = eng.state_pool_fetch_shor(e)
        for key in ("nq", "X", "Theta", "V"):
            flat["shor/pool/%d/%s" % (e, key)] = np.asarray(st[key])
    certs = eng.fetch_shor_certificate([0, 1, 2])
    for i, c in enumerate(certs):
        for f in SHOR_CERT_FIELDS:
            flat["shor/certificate/%d/%s" % (i, f)] = np.asarray(getattr(c, f))
    nodes = [[]] + kids
    info = [(minors, None)] * 3
    for way in (True, False):
        bd, df, tm = eng.shor_dual_bound(nodes, info, certs, "linear", sanitise=way, want_defects=True, want_terms=True)
        pre = "shor_dual_bound/sanitise_%d/" % int(way)
        flat[pre + "bound"] = np.asarray(bd); flat[pre + "terms"] = np.asarray(tm)
        flat[pre + "defects"] = np.asarray([[d[key] for key in sorted(d)] for d in df])
    eng.close()


def _base_certificates(omc, flat):
    """Base 24 x 30, rank 2, linear3, two nodes with two cuts each, certificates kept: fetch_certificate and dual_bound on them."""
    A, mask = omc.pkg.data.generate_matrix_completion_data(2, 24, 30, int(0.35 * 24 * 30), seed=3)
    eng = omc.Engine(A, mask, GAMMA, 2)
    P = omc.default_params(rho_scale=4.0, max_iters=400)
    nodes, _ = omc.pkg.bnb.expand_frontier(eng, 2, "linear3", params=P, max_nodes=2)
    nodes = nodes[:2]
    assert len(nodes) == 2 and all(len(c) == 2 for c in nodes)
    eng.keep_certificates(True)
    res = eng.matrix_completion_SDP_relaxation(nodes, "linear3", params=P, want_X=False)
    _put(flat, "base_certificates/fetch", res)
    certs = eng.fetch_certificate([0, 1])
    for i, c in enumerate(certs):
        for f in CERT_FIELDS:
            flat["base_certificates/certificate/%d/%s" % (i, f)] = np.asarray(getattr(c, f))
    flat["base_certificates/dual_bound"] = np.asarray(eng.dual_bound(nodes, certs, "linear3"))
    eng.close()


def _plain(omc, flat):
    """breakpoint_vectors, round_Y and left_singular at n = 24 on the relaxed root; psd_project at orders 16 and 160; column_prox mode 0."""
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, 24, 30, int(0.35 * 24 * 30), seed=3)
    eng = omc.Engine(A, mask, GAMMA, 1)
    root = eng.matrix_completion_SDP_relaxation([[]], "linear", params=omc.default_params(rho_scale=4.0), want_Theta=True)[0]
    _put(flat, "plain/root", [root])
    x, ev, fe = eng.breakpoint_vectors([root["Y"]] * 2, [root["U"], -root["U"]])
    flat["plain/breakpoint/x"] = x; flat["plain/breakpoint/ev"] = ev; flat["plain/breakpoint/feasible"] = fe
    flat["plain/round_Y"] = np.stack(eng.round_Y([root["Y"], root["Y"].T @ root["Y"]]))
    flat["plain/left_singular"] = np.stack(eng.left_singular([root["X"], A * mask]))
    rng = np.random.default_rng(11)
    for N in (16, 160):
        M = rng.standard_normal((2, N, N))
        P, evals, V = eng.psd_project(M + np.transpose(M, (0, 2, 1)), hi=1.5, want_evals=True, want_V=True)
        flat["plain/psd_project/%d/P" % N] = P; flat["plain/psd_project/%d/evals" % N] = evals; flat["plain/psd_project/%d/V" % N] = V
    cp = eng.column_prox(np.stack([root["Y"], 0.5 * root["Y"]]), rho_f=[1.0, 0.3], mode=0)
    for key in ("alpha", "s", "nfact"):
        flat["plain/column_prox/" + key] = cp[key]
    flat["plain/evaluate_objective"] = np.asarray(eng.evaluate_objective(root["X"]))
    eng.close()


def _order520(omc, flat):
    """Base 520 x 530, rank 1: one node in one slot for two checks' worth of iterations (np16 > 512: the tracked block's Z scratch, cert_enable)."""
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, 520, 530, int(0.2 * 520 * 530), seed=5)
    eng = omc.Engine(A, mask, GAMMA, 1)
    P = omc.default_params(rho_scale=4.0, slots=1)
    P.max_iters = 2 * P.check_every
    res = eng.matrix_completion_SDP_relaxation([[]], "linear", params=P, want_X=True, want_Theta=False)
    _put(flat, "order520/fetch", res)
    eng.close()


def _arm(omc, orc):
    flat = {}
    _shor_cases(omc, orc, flat)
    _base_certificates(omc, flat)
    _plain(omc, flat)
    _order520(omc, flat)
    return flat


@pytest.fixture(scope="module")
def arms(omc, tmp_path_factory):
    parent = os.environ.get("OMC_PARENT_LIB")
    if not parent:
        pytest.skip("OMC_PARENT_LIB is not set: no other build to compare with")
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    out = {}
    for name, lib in (("this", None), ("parent", parent)):
        path = str(tmp_path_factory.mktemp("host_api") / (name + ".npz"))
        env = dict(os.environ)
        env.pop("OMC_AMD_LIB", None)
        if lib:
            env["OMC_AMD_LIB"] = lib
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=300)
        out[name] = np.load(path)
    return out


@pytest.mark.parametrize("case", CASES)
def test_equal_to_the_other_build(arms, case):
    mine, theirs = arms["this"], arms["parent"]
    keys = sorted(key for key in mine.files if key.split("/")[0] == case)
    assert keys and keys == sorted(key for key in theirs.files if key.split("/")[0] == case)
    for key in keys:
        assert np.array_equal(mine[key], theirs[key], equal_nan=mine[key].dtype.kind == "f"), (key, mine[key], theirs[key])
    if case == "shor":      # the case did what it is there for: three nodes within three checks with a certificate each, the children started warm
        print([(int(mine["shor/fetch/%d/iters" % i]), int(mine["shor/fetch/%d/status_code" % i])) for i in range(3)], mine["shor/warm_stats"].tolist())
        assert all(0 < int(mine["shor/fetch/%d/iters" % i]) <= 3 * SHOR_CHECK_EVERY for i in range(3))
        assert dict(mine["shor/warm_stats"].tolist())["loaded_identical"] == "2"
        assert all(np.array_equal(mine["shor/certificate/%d/bound" % i], mine["shor/fetch/%d/dual_bound" % i]) for i in range(3))


if __name__ == "__main__":      # one arm: every case on the library OMC_AMD_LIB names (default: the tree's own)
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import omc_amd
    import omc_oracle
    np.savez(sys.argv[1], **_arm(omc_amd, omc_oracle))
