"""The objective cutoff's surface, without a GPU: header, exports, bindings, argument checks, driver keywords, documentation."""
import ctypes as C
import inspect
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("omc_relax_set_cutoff", "omc_relax_get_cutoff", "omc_last_cutoff_stats")


def test_declared_exported_and_bound(omc):
    with open(os.path.join(ROOT, "include", "omc.h")) as f:
        hdr = f.read()
    lib = omc.load()
    for s in FUNCS:
        assert ("int " + s + "(") in hdr, s
        assert hasattr(lib, s) and s in omc.EXPORTS, s
        assert getattr(lib, s).argtypes is not None, s      # bound with argument types in _lib.py (a double passed untyped would arrive as an int)
    assert lib.omc_relax_set_cutoff.argtypes[1] is C.c_double
    assert "#define OMC_CUTOFF 4" in hdr and "MOI.OBJECTIVE_LIMIT" in hdr
    assert "#define OMC_VERSION 100" in hdr and lib.omc_version() == 100
    for name in ("set_cutoff", "get_cutoff", "cutoff_stats"):
        assert callable(getattr(omc.Engine, name))


def test_null_handle_and_null_output_are_refused(omc):
    lib = omc.load()
    assert lib.omc_relax_set_cutoff(None, 0.0) == -3      # OMC_ERR_ARGUMENT, before anything touches a device
    v = C.c_double(0.0)
    assert lib.omc_relax_get_cutoff(None, C.byref(v)) == -3
    out = (C.c_int64 * 4)()
    assert lib.omc_last_cutoff_stats(None, out) == -3


def test_status_name(omc):
    assert omc.STATUS_NAMES[4] == "OBJECTIVE_LIMIT"
    assert [omc.STATUS_NAMES[q] for q in range(4)] == ["OPTIMAL", "SLOW_PROGRESS", "TIME_LIMIT", "INFEASIBLE"]


def test_drivers_accept_the_keyword_and_default_to_off(omc):
    for fn in (omc.pkg.bnb.branch_and_bound, omc.pkg.bnb_stream.branch_and_bound_streaming):
        p = inspect.signature(fn).parameters["objective_cutoff"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_integration_guide_names_the_functions(omc):
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for s in FUNCS:
        assert s in doc, s
    assert "OBJECTIVE_LIMIT" in doc
