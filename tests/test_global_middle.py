"""The middle of k_global (rows c = A t - b with the cut vectors read from their staged copy, the row projection on registers, the U
correction from the staged vectors and per-row descriptors in LDS) against the parent commit's build, bit for bit.  OMC_PARENT_LIB names
that build; without it the module skips.  Both arms run in a child process each (this file as a script, the library chosen by
OMC_AMD_LIB); objective, dual bound, iterations, status, Y and U of every node are compared with np.array_equal.

Shapes: the 24 x 30 instance of smoke(), root and children; n = 20 with seven cuts (Rmax = 23: the Gram matrix stays in global memory, seven
cut rows fit one MFMA pass) and with 17 cuts (more cut rows than GL_XS = 16: a second pass, and vectors that are not staged in steps 3, 5
and 6); n = 32, root and children; config 2 at depth 3 and the warm children of those nodes from the state pool; the small Shor root of
test_global_schedule.py.  Every shape runs with the target in LDS and with OMC_GLOBAL_NOLDS=1."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ("smoke24", "n20_7cuts", "n20_17cuts", "n32", "config2_depth3_warm", "shor_root")
ARMS = ("lds", "nolds")
KEYS = ("objective", "dual_bound", "iters", "status_code", "Y", "U")


def _solve(eng, nodes, P, arm, **kw):
    if arm == "nolds":
        eng.tuning_set("OMC_GLOBAL_NOLDS", "1")
    try:
        out = eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False, **kw)
        assert bool(eng.solver_info()["global_lds"]) == (arm == "lds")
        return out
    finally:
        eng.tuning_set("OMC_GLOBAL_NOLDS", None)


def _put(flat, prefix, results):
    assert results and all(o["iters"] > 0 for o in results)
    for i, o in enumerate(results):
        for key in KEYS:
            flat["%s/%d/%s" % (prefix, i, key)] = np.asarray(o[key])


def _root_and_children(omc, flat, name, arm, n, m, frac, seed):
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, n, m, int(frac * n * m), seed=seed)
    eng = omc.Engine(A, mask, GAMMA, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    root = _solve(eng, [[]], P, arm)
    _put(flat, "%s/%s/root" % (name, arm), root)
    _put(flat, "%s/%s/children" % (name, arm), _solve(eng, omc.pkg.bnb.make_children([], root[0], "linear", 1), P, arm))
    eng.close()


def _n20(omc, flat, name, arm, ncuts):
    n, m = 20, 24
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, n, m, int(0.4 * n * m), seed=7)
    eng = omc.Engine(A, mask, GAMMA, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    U = np.array(_solve(eng, [[]], P, arm)[0]["U"])
    rng = np.random.default_rng(13)
    deep = []
    for s in range(2):
        cuts = []
        for t in range(ncuts):
            x = rng.standard_normal(n); x /= np.linalg.norm(x)
            cuts.append((x, U, ["left" if (t + s) % 2 else "right"]))
        deep.append(cuts)
    _put(flat, "%s/%s/deep" % (name, arm), _solve(eng, deep, P, arm))
    eng.close()


def _config2(omc, flat, name, arm):
    A, mask, gamma, _ = omc.pkg.data.config_instance(2, seed=0)
    eng = omc.Engine(A, mask, gamma, 1)
    P = omc.default_params(rho_scale=4.0, max_iters=300, eps_gap=1e-14)
    nodes, _ = omc.pkg.bnb.expand_frontier(eng, 3, "linear", params=omc.default_params(rho_scale=4.0))
    assert nodes and all(len(c) == 3 for c in nodes)
    a = _solve(eng, nodes, P, arm)
    _put(flat, "%s/%s/depth3" % (name, arm), a)
    Pw = omc.default_params(rho_scale=4.0)
    eng.state_pool_create(len(nodes))
    _solve(eng, nodes, Pw, arm, save_to=list(range(len(nodes))))
    kids, lf = [], []
    for i, (cuts, o) in enumerate(zip(nodes, a)):
        for c in omc.pkg.bnb.make_children(cuts, o, "linear", 1):
            kids.append(c); lf.append(i)
    assert kids and all(len(c) == 4 for c in kids)
    _put(flat, "%s/%s/warm_children" % (name, arm), _solve(eng, kids, Pw, arm, load_from=lf))
    eng.close()


def _shor_root(omc, orc, flat, name, arm):
    A, mask = orc.make_instance(10, 12, 1, n_indices=60, seed=1, noise=0.3, kind="lowrank")
    eng = omc.Engine(A, mask, GAMMA, 1)
    out = _solve(eng, [[]], omc.default_params(eps_gap=1e-6), arm, add_Shor_valid_inequalities=True, shor_info=[([], None)])
    _put(flat, "%s/%s/root" % (name, arm), out)
    eng.close()


def _arm(omc, orc):
    flat = {}
    for arm in ARMS:
        _root_and_children(omc, flat, "smoke24", arm, 24, 30, 0.35, 3)
        _n20(omc, flat, "n20_7cuts", arm, 7)
        _n20(omc, flat, "n20_17cuts", arm, 17)
        _root_and_children(omc, flat, "n32", arm, 32, 40, 0.35, 5)
        _config2(omc, flat, "config2_depth3_warm", arm)
        _shor_root(omc, orc, flat, "shor_root", arm)
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
        path = str(tmp_path_factory.mktemp("global_middle") / (name + ".npz"))
        env = dict(os.environ)
        env.pop("OMC_AMD_LIB", None)
        if lib:
            env["OMC_AMD_LIB"] = lib
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=300)
        out[name] = np.load(path)
    return out


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_equal_to_the_parent_build(arms, shape, arm):
    mine, theirs = arms["this"], arms["parent"]
    pre = "%s/%s/" % (shape, arm)
    keys = sorted(key for key in mine.files if key.startswith(pre))
    assert keys and keys == sorted(key for key in theirs.files if key.startswith(pre))
    for key in keys:
        assert np.array_equal(mine[key], theirs[key], equal_nan=mine[key].dtype.kind == "f"), (key, mine[key], theirs[key])


def test_lds_and_global_arm_agree(arms):
    """the two arms of the kernel run the same arithmetic (test_global_schedule.py): so do they here, on this build"""
    mine = arms["this"]
    for key in mine.files:
        shape, arm, rest = key.split("/", 2)
        if arm == "lds":
            assert np.array_equal(mine[key], mine["%s/nolds/%s" % (shape, rest)], equal_nan=mine[key].dtype.kind == "f"), key


if __name__ == "__main__":      # one arm: every shape on the library OMC_AMD_LIB names (default: the tree's own)
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import omc_amd
    import omc_oracle
    np.savez(sys.argv[1], **_arm(omc_amd, omc_oracle))
