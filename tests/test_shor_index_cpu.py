"""CPU tests of the device builder of a Shor list's index structure (omc_shor_index_build, omc_shor_index_plan,
omc_last_shor_index_stats): the boundary, the plan, and the numpy restatement the GPU tests compare against
(tests/shor_index_ref.py) checked against the oracle's ShorStructure.  No GPU."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shor_index_ref as ref      # noqa: E402

SYMBOLS = ("omc_shor_index_build", "omc_shor_index_plan", "omc_last_shor_index_stats")


def test_symbols_are_declared_exported_and_bound(omc):
    lib = omc.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omc.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in omc.EXPORTS and (s + "(") in hdr, s


def test_null_handles_are_refused(omc):
    lib = omc.load()
    out = np.zeros(9, np.int64); st = np.zeros(5)
    assert lib.omc_shor_index_build(None, 1, 0, None, 0, None, *([None] * 14)) == -3
    assert lib.omc_last_shor_index_stats(None, omc.pkg._lib.ptr(st)) == -3
    assert lib.omc_shor_index_plan(10, 12, 5, None) == -3
    assert lib.omc_shor_index_plan(0, 12, 5, omc.pkg._lib.ptr(out)) == -3
    assert lib.omc_shor_index_plan(10, 12, -1, omc.pkg._lib.ptr(out)) == -3
    assert lib.omc_shor_index_plan(10, 12, 1 << 28, omc.pkg._lib.ptr(out)) == -4
    assert lib.omc_shor_index_plan(1 << 15, 1 << 15, 1, omc.pkg._lib.ptr(out)) == -4


def test_wrapper_signatures(omc):
    E = omc.Engine
    sig = inspect.signature(E.shor_index)
    assert list(sig.parameters) == ["self", "shor_idx", "soc_idx", "where"]
    assert sig.parameters["soc_idx"].default is None and sig.parameters["where"].default == "device"
    assert list(inspect.signature(E.shor_index_stats).parameters) == ["self"]
    assert list(inspect.signature(omc.pkg.api.shor_index_plan).parameters) == ["n", "m", "nq"]


def _passes(maxkey):
    return max(1, -(-int(maxkey).bit_length() // 8))


@pytest.mark.parametrize("n,m", [(10, 12), (300, 4), (70, 8000)])
def test_plan_pass_counts_follow_the_largest_key(omc, n, m):
    """ceil(bits / 8) of the largest key the shape allows: V1 ((n-1) m + m-2) m + m-1, V2 ((n-2) n + n-1) m + m-1, coordinate n m - 1,
    duplicate (((n-2) n + n-1) m + m-2) m + m-1"""
    p = omc.pkg.api.shor_index_plan(n, m, 100)
    pair = (n - 2) * n + (n - 1)
    assert p["passes_v1"] == _passes(((n - 1) * m + (m - 2)) * m + (m - 1))
    assert p["passes_v2"] == _passes(pair * m + (m - 1))
    assert p["passes_coord"] == _passes(n * m - 1)
    assert p["passes_dup"] == _passes((pair * m + (m - 2)) * m + (m - 1))
    if (n, m) == (70, 8000):
        assert p["passes_v1"] == 5            # the keys pass 2^32
    sorts = p["passes_v1"] + p["passes_v2"] + p["passes_coord"] + p["passes_dup"]
    assert p["launches"] == 5 * sorts + 19 and omc.pkg.api.shor_index_plan(n, m, 0)["launches"] == 4


def test_plan_bytes_are_monotone_and_staging_is_the_capacity_layout(omc):
    n, m = 12, 14
    prev = None
    for nq in (0, 1, 127, 128, 129, 1000, 1024, 1025, 5000, 632732):
        p = omc.pkg.api.shor_index_plan(n, m, nq)
        assert p["stage_ints"] == 20 * nq + n * m + m + 3
        assert p["stage_bytes"] == (n * m + m + 15) // 16 * 16
        assert p["tile"] >= 256
        if prev is not None:
            assert p["scratch_bytes"] >= prev
        prev = p["scratch_bytes"]
    assert omc.pkg.api.shor_index_plan(n, m, 5000)["scratch_bytes"] > omc.pkg.api.shor_index_plan(n, m, 1000)["scratch_bytes"]


def test_knob_is_known(omc):
    """OMC_SHOR_INDEX_DEVICE_MIN is a knob of the table (omc_tuning_set needs a handle, so the name is looked up in the library's strings)"""
    blob = open(omc.LIB_PATH, "rb").read()
    assert b"OMC_SHOR_INDEX_DEVICE_MIN" in blob


@pytest.mark.parametrize("name", ["10x12", "6x7", "12x14", "14x18"])
def test_restatement_matches_the_oracle_structure(orc, name):
    """kid, nv1, nv2 and ctype of omc_oracle_shor.ShorStructure on the class-4 list: forward, reversed, permuted, one minor, empty"""
    import omc_oracle_shor as sh
    A, mask, minors = ref.instance(orc, name)
    n, m = mask.shape
    for vname, lst in ref.variants(minors).items():
        _, soc = sh.driver_shor_lists(mask, (4,), minors=[tuple(t) for t in lst.tolist()])
        st = sh.ShorStructure(n, m, lst, soc, mask)
        got = ref.build(n, m, mask, lst, soc)
        assert (got["nq"], got["nv1"], got["nv2"]) == (st.nq, st.nv1, st.nv2), (name, vname)
        assert np.array_equal(got["kid"], np.stack([st.k12, st.k34, st.k13, st.k24]).astype(np.int32).reshape(4, st.nq)), (name, vname)
        assert np.array_equal(got["ctype"], st.ctype.astype(np.uint8)), (name, vname)
        # internal consistency of the CSR arrays
        assert got["cptr"][-1] == 4 * st.nq and got["v1ptr"][-1] == 2 * st.nq and got["v2ptr"][-1] == 2 * st.nq
        assert len(got["v1ptr"]) == st.nv1 + 1 and len(got["v2ptr"]) == st.nv2 + 1
        assert np.array_equal(np.sort(got["cent"]), np.arange(4 * st.nq))


def test_restatement_refusals():
    mask = np.ones((6, 7), bool)
    ok = np.array([[1, 2, 1, 2], [1, 3, 2, 5]])
    for bad, msg in (([[2, 2, 1, 2]], ref.MSG_RANGE), ([[1, 2, 1, 8]], ref.MSG_RANGE), ([[0, 2, 1, 2]], ref.MSG_RANGE),
                     ([[1, 2, 1, 2]], ref.MSG_DUP), ([[1, 2, 1, 2], [1, 2, 3, 9]], ref.MSG_RANGE)):
        with pytest.raises(ValueError, match=msg[:20]):
            ref.build(6, 7, mask, np.concatenate([ok, np.array(bad)]))
    with pytest.raises(ValueError, match=ref.MSG_SOC):
        ref.build(6, 7, mask, ok, [[7, 1]])
