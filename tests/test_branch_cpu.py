"""Children by reference, without a GPU: the three symbols (header, exports, bindings), omc_branch_plan against bnb.child_directions, the
argument checks that are decided before any device call, the driver's keyword and the documentation."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("omc_branch_plan", "omc_relax_append_children", "omc_relax_fetch_descriptor")
PER_COLUMN = {"linear": 2, "linear2": 3, "linear3": 4}


def test_declared_exported_and_bound(omc):
    with open(os.path.join(ROOT, "include", "omc.h")) as f:
        hdr = f.read()
    lib = omc.load()
    for s in FUNCS:
        assert ("int " + s + "(") in hdr, s
        assert hasattr(lib, s) and s in omc.EXPORTS, s
        assert getattr(lib, s).argtypes is not None, s
    for name in ("branch_plan", "append_children", "fetch_descriptor"):
        assert callable(getattr(omc.Engine, name))


def plan(omc, cut_type, k, capacity):
    d = np.full((max(capacity, 1), k), -1, np.int8)
    cnt = C.c_int(-1)
    rc = omc.load().omc_branch_plan(cut_type, k, capacity, d.ctypes.data_as(C.c_void_p), C.byref(cnt))
    return rc, cnt.value, d


@pytest.mark.parametrize("cut_type", ["linear", "linear2", "linear3"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_plan_is_child_directions(omc, cut_type, k):
    api, bnb = omc.pkg.api, omc.pkg.bnb
    want = [[api.DIR_CODES[x] for x in d] for d in bnb.child_directions(cut_type, k)]
    total = PER_COLUMN[cut_type] ** k
    assert len(want) == total
    rc, cnt, d = plan(omc, api.CUT_TYPES[cut_type], k, total + 3)
    assert rc == 0 and cnt == total
    assert d[:total].tolist() == want
    assert (d[total:] == -1).all()          # nothing written behind the last child
    if k > 1:
        assert d[0, 0] != d[1, 0] and d[0, 1] == d[1, 1]      # the first column varies fastest
    # the Python wrappers give the labels
    assert api.branch_plan(cut_type, k) == [tuple(x) for x in bnb.child_directions(cut_type, k)]


def test_plan_refusals(omc):
    lib = omc.load()
    rc, cnt, d = plan(omc, 0, 3, 7)                    # 2^3 children do not fit 7
    assert rc == -3 and cnt == 8 and (d == -1).all()
    assert "capacity" in lib.omc_last_error().decode()
    assert plan(omc, 0, 3, 8)[0] == 0
    assert plan(omc, 3, 1, 16)[0] == -1                # OMC_ERR_INVALID_ENUM: no such cut type
    assert plan(omc, -1, 1, 16)[0] == -1
    assert plan(omc, 0, 0, 16)[0] == -3 and plan(omc, 0, 9, 1 << 20)[0] == -3
    cnt = C.c_int(0)
    assert lib.omc_branch_plan(0, 1, 2, None, C.byref(cnt)) == -3
    with pytest.raises(ValueError):
        omc.pkg.api.branch_plan("quadratic", 1)


def test_null_handle_is_refused(omc):
    lib = omc.load()
    first = C.c_int(0); p = (C.c_int * 1)(0); d = (C.c_int8 * 1)(0)
    assert lib.omc_relax_append_children(None, 1, p, d, None, None, C.byref(first)) == -3      # OMC_ERR_ARGUMENT, before anything touches a device
    assert lib.omc_relax_fetch_descriptor(None, 0, *([None] * 11)) == -3


def test_driver_accepts_the_keyword_and_defaults_to_off(omc):
    p = inspect.signature(omc.pkg.bnb_stream.branch_and_bound_streaming).parameters["device_branching"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_documents_name_the_functions(omc):
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for s in FUNCS:
        assert s in doc, s
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "omc_relax_append_children" in f.read()
