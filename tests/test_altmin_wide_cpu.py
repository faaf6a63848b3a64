"""CPU tests of omc_altmin_plan: the launch plan of alternating_minimization (kernel variant by rank, LDS or per-problem global slab,
rows of model_U) is a pure host function of the sizes, taken from the layouts the kernels themselves use (omc_layout.h)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, ARGUMENT = -4, -3


def _plan(omc, n, m, k, max_cuts=0, nolds=0):
    out = np.zeros(4, np.int64)
    rc = omc.load().omc_altmin_plan(n, m, k, max_cuts, nolds, out.ctypes.data_as(C.c_void_p))
    return rc, dict(variant=int(out[0]), lds=int(out[1]), slab=int(out[2]), Rmax=int(out[3]))


def test_error_codes_are_those_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "omc.h")).read()
    assert int(re.search(r"#define OMC_ERR_UNSUPPORTED \((-?\d+)\)", hdr).group(1)) == UNSUPPORTED
    assert int(re.search(r"#define OMC_ERR_ARGUMENT \((-?\d+)\)", hdr).group(1)) == ARGUMENT


def test_altmin_plan_is_declared_exported_and_listed(omc):
    hdr = open(os.path.join(ROOT, "include", "omc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bomc_altmin_plan\s*\(", hdr)
    assert hasattr(omc.load(), "omc_altmin_plan") and "omc_altmin_plan" in omc.EXPORTS


@pytest.mark.parametrize("k,variant", [(1, 1), (2, 2), (4, 2), (5, 3), (8, 3)])
def test_variant_by_rank(omc, k, variant):
    rc, p = _plan(omc, 16, 22, k)
    assert rc == 0 and p["variant"] == variant


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("max_cuts", [0, 1, 2, 7])
def test_rows_of_model_U(omc, k, max_cuts):
    rc, p = _plan(omc, 16, 22, k, max_cuts)
    assert rc == 0 and p["Rmax"] == k * (k + 1) // 2 + 2 * k * max(1, max_cuts)


@pytest.mark.parametrize("k", [1, 2, 5, 8])
def test_nolds_plans_the_slab(omc, k):
    rc, p = _plan(omc, 16, 22, k, 1, nolds=1)
    assert rc == 0 and p["lds"] == 0 and p["slab"] > 0
    rc, q = _plan(omc, 16, 22, k, 1, nolds=0)
    assert rc == 0 and q["lds"] > 0 and q["slab"] == 0          # the same problems fit the LDS
    assert p["slab"] >= q["lds"]                                # one layout serves both: the slab holds at least the LDS block


def test_lds_or_slab_by_size(omc):
    rc, p = _plan(omc, 1000, 1000, 2)                           # BASELINE config 5: 144 KB of state per problem
    assert rc == 0 and p["variant"] == 2 and p["lds"] == 0 and p["slab"] > 128 * 1024
    rc, p = _plan(omc, 16, 22, 5)
    assert rc == 0 and p["variant"] == 3 and 0 < p["lds"] <= 128 * 1024 and p["slab"] == 0
    rc, p = _plan(omc, 100, 100, 8, 1)                          # rank 8 at 100 x 100: H and its inverse alone are 100 KB
    assert rc == 0 and p["variant"] == 3 and p["lds"] == 0 and p["slab"] > 0


def test_the_wide_block_grows_with_the_newton_scratch(omc):
    """k_altmin_w keeps J, P (k^2 x k^2) and the packed Cholesky factor in its block: at least 2 k^4 + k^2 (k^2 + 1) / 2 doubles beyond the row state"""
    for k in (5, 6, 7, 8):
        rc, p = _plan(omc, 16, 22, k, 1, nolds=1)
        mq = k * k
        state = 4 * 16 * k + 2 * 16 * k * k + 22 * k
        assert rc == 0 and p["slab"] >= 8 * (state + 2 * mq * mq + mq * (mq + 1) // 2)


def test_refusals(omc):
    lib = omc.load()
    rc, _ = _plan(omc, 16, 22, 9)
    assert rc == UNSUPPORTED and b"k > 8" in lib.omc_last_error()
    for n, m, k in ((0, 22, 2), (16, 0, 2), (16, 22, 0), (-1, 22, 2)):
        rc, _ = _plan(omc, n, m, k)
        assert rc == ARGUMENT
    assert lib.omc_altmin_plan(16, 22, 2, 0, 0, None) == ARGUMENT
