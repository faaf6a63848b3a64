"""k_small's projection through small_proj_chain (two row tiles of T1 per wave, Q and dS from their LDS copies, the one-wave pieces of
the eigen part on the wave that ran the sweep, the rebuild entry by entry) against the body it replaces, bit for bit.  Both bodies live in one library:
OMC_SMALL_CHAIN=0 selects the old one.  With OMC_PARENT_LIB naming the parent commit's build the default arm is also compared with that
library, each in a child process (this file as a script, the library chosen by OMC_AMD_LIB); without it that part skips.  objective, dual
bound, iterations, status, Y, U, lambda_min and breakpoint_vec of every node are compared with np.array_equal.  Every solve runs
max_iters=300, eps_gap=1e-14 (nothing stops early) unless stated.

Shapes, the smallest at which each branch of the kernel can go wrong:
  n16          16 x 20, root + children: one row tile, three waves have nothing to do
  smoke24_k1/2 24 x 30 (smoke()'s instance), root + children, k = 1 and k = 2: two tiles, the second with 8 rows; the W3T / Q3T block at k = 2
  n20_Ncuts    n = 20, m = 24 with 7, 14, 15 and 17 cuts; r = k + cuts here (solver_info()["r_max"] is asserted).  7: r = 8, N3 = 9 is odd, so the
               sweep runs on the padded Np = 10; 14: r = 15, N3 = Np = 16, the largest one-wave sweep (added to the issue's three);
               15: r = 16, N3 = 17, Np = 18 > 16 -- the MFMA products with eig_frontend; 17: r = 18 > 16, the scalar path of the old body
               in both arms
  n70          70 x 72 root + children: 5 tiles, one wave has two tiles, three have one
  config2      config 2 (100 x 100) at depth 3 and the warm children from the state pool: 7 tiles, a last tile of 4 rows, warm and cold V3
  n257         257 x 260 root, max_iters=25: n > 256, the scalar T1 / E3 path in both arms
  shor_root    the small Shor root of test_global_schedule.py: k_small on its stream in Shor mode"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 80.0
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ("n16", "smoke24_k1", "smoke24_k2", "n20_7cuts", "n20_14cuts", "n20_15cuts", "n20_17cuts", "n70", "config2", "n257", "shor_root")
KEYS = ("objective", "dual_bound", "iters", "status_code", "Y", "U", "lambda_min", "breakpoint_vec")
# r_max the shape must report (None: not pinned), and whether small_proj_chain serves it in the default arm (r <= 16 and n <= 256)
PATHS = {"n16": (None, True), "smoke24_k1": (None, True), "smoke24_k2": (None, True), "n20_7cuts": (8, True), "n20_14cuts": (15, True),
         "n20_15cuts": (16, True), "n20_17cuts": (18, False), "n70": (None, True), "config2": (None, True), "n257": (None, False),
         "shor_root": (None, True)}


def _solve(eng, nodes, P, arm, **kw):
    if arm == "old":
        eng.tuning_set("OMC_SMALL_CHAIN", "0")
    try:
        out = eng.matrix_completion_SDP_relaxation(nodes, "linear", params=P, want_X=False, **kw)
        assert eng.solver_info()["small_lds"]
        return out
    finally:
        if arm == "old":
            eng.tuning_set("OMC_SMALL_CHAIN", None)


def _put(flat, prefix, results):
    assert results and all(o["iters"] > 0 for o in results)
    for i, o in enumerate(results):
        for key in KEYS:
            flat["%s/%d/%s" % (prefix, i, key)] = np.asarray(o[key])


def _meta(flat, name, arm, eng, n):
    flat["%s/%s/meta" % (name, arm)] = np.array([eng.solver_info()["r_max"], n])


def _root_and_children(omc, flat, name, arm, n, m, frac, seed, k=1, **pkw):
    A, mask = omc.pkg.data.generate_matrix_completion_data(k, n, m, int(frac * n * m), seed=seed)
    eng = omc.Engine(A, mask, GAMMA, k)
    P = omc.default_params(rho_scale=4.0, **{"max_iters": 300, "eps_gap": 1e-14, **pkw})
    root = _solve(eng, [[]], P, arm)
    _put(flat, "%s/%s/root" % (name, arm), root)
    _put(flat, "%s/%s/children" % (name, arm), _solve(eng, omc.pkg.bnb.make_children([], root[0], "linear", k), P, arm))
    _meta(flat, name, arm, eng, n)
    eng.close()


def _root(omc, flat, name, arm, n, m, frac, seed, max_iters):
    A, mask = omc.pkg.data.generate_matrix_completion_data(1, n, m, int(frac * n * m), seed=seed)
    eng = omc.Engine(A, mask, GAMMA, 1)
    _put(flat, "%s/%s/root" % (name, arm), _solve(eng, [[]], omc.default_params(rho_scale=4.0, max_iters=max_iters, eps_gap=1e-14), arm))
    _meta(flat, name, arm, eng, n)
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
    _meta(flat, name, arm, eng, n)
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
    _meta(flat, name, arm, eng, 100)
    if hasattr(eng._lib, "omc_kernel_residency"):
        flat["%s/%s/residency" % (name, arm)] = np.array([eng.kernel_residency()["k_small"]])
    eng.close()


def _shor_root(omc, orc, flat, name, arm):
    A, mask = orc.make_instance(10, 12, 1, n_indices=60, seed=1, noise=0.3, kind="lowrank")
    eng = omc.Engine(A, mask, GAMMA, 1)
    out = _solve(eng, [[]], omc.default_params(eps_gap=1e-6), arm, add_Shor_valid_inequalities=True, shor_info=[([], None)])
    _put(flat, "%s/%s/root" % (name, arm), out)
    _meta(flat, name, arm, eng, 10)
    eng.close()


def _arm(omc, orc, arm, flat):
    _root_and_children(omc, flat, "n16", arm, 16, 20, 0.4, 11)
    _root_and_children(omc, flat, "smoke24_k1", arm, 24, 30, 0.35, 3)
    _root_and_children(omc, flat, "smoke24_k2", arm, 24, 30, 0.35, 3, k=2)
    for ncuts in (7, 14, 15, 17):
        _n20(omc, flat, "n20_%dcuts" % ncuts, arm, ncuts)
    _root_and_children(omc, flat, "n70", arm, 70, 72, 0.3, 5)
    _config2(omc, flat, "config2", arm)
    _root(omc, flat, "n257", arm, 257, 260, 0.1, 9, 25)
    _shor_root(omc, orc, flat, "shor_root", arm)
    return flat


def _equal(mine, theirs, pre_mine, pre_theirs):
    keys = sorted(key[len(pre_mine):] for key in mine if key.startswith(pre_mine) and not key.endswith("/residency"))
    assert keys and keys == sorted(key[len(pre_theirs):] for key in theirs if key.startswith(pre_theirs) and not key.endswith("/residency"))
    for key in keys:
        x, y = mine[pre_mine + key], theirs[pre_theirs + key]
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (key, x, y)


@pytest.fixture(scope="module")
def arms(omc, orc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    flat = {}
    for arm in ("new", "old"):
        _arm(omc, orc, arm, flat)
    return flat


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    parent = os.environ.get("OMC_PARENT_LIB")
    if not parent:
        pytest.skip("OMC_PARENT_LIB is not set: no other build to compare with")
    out = {}
    for name, lib in (("this", None), ("parent", parent)):
        path = str(tmp_path_factory.mktemp("small_chain") / (name + ".npz"))
        env = dict(os.environ)
        env.pop("OMC_AMD_LIB", None)
        env.pop("OMC_SMALL_CHAIN", None)
        if lib:
            env["OMC_AMD_LIB"] = lib
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=300)
        out[name] = dict(np.load(path))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_equals_the_old_body(arms, shape):
    _equal(arms, arms, "%s/new/" % shape, "%s/old/" % shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_intended_path_ran(arms, shape):
    """r_max of the solve decides the kernel's path with n: r <= 16 and n <= 256 is small_proj_chain (Np <= 16: the one-wave sweep)"""
    r_want, chain = PATHS[shape]
    r_max, n = (int(v) for v in arms["%s/new/meta" % shape])
    print(shape, "r_max", r_max, "n", n)
    if r_want is not None:
        assert r_max == r_want
    assert (r_max <= 16 and n <= 256) == chain


def test_residency_is_still_three(arms):
    """the register budget of a fourth workgroup per CU (128 with the AGPRs) was not reached: 134 + 16"""
    assert int(arms["config2/new/residency"][0]) == 3 and int(arms["config2/old/residency"][0]) == 3


@pytest.mark.parametrize("shape", SHAPES)
def test_equal_to_the_parent_build(builds, shape):
    _equal(builds["this"], builds["parent"], "%s/new/" % shape, "%s/new/" % shape)


if __name__ == "__main__":      # the default arm of every shape on the library OMC_AMD_LIB names (default: the tree's own)
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import omc_amd
    import omc_oracle
    np.savez(sys.argv[1], **_arm(omc_amd, omc_oracle, "new", {}))
