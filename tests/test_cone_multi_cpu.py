"""CPU tests of the boundary of omc_psd_project_batch: declared, exported, listed, and its argument checks come before any device call."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_psd_project_is_declared_exported_and_listed(omc):
    hdr = open(os.path.join(ROOT, "include", "omc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("omc_psd_project_batch", "omc_last_cone_multi_stats", "omc_cone_multi_budget"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(omc.load(), name) and name in omc.EXPORTS, name


def test_psd_project_checks_arguments_before_any_device_call(omc):
    lib = omc.load()
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    rc = lib.omc_psd_project_batch(None, 1, 2, p, 0.0, 1.0, 0, None, p, None, None)
    assert rc == -3 and b"handle" in lib.omc_last_error()


def test_sweep_budget_rule(omc):
    """the budget omc_relax_solve enqueues for the next interval (bound MAX_SWEEPS = 30): what the last interval needed + 2; an interval
    without a call (the tracked block served every slot) must not shrink it to 0 + 2 -- the next call is a fall-back from a stale basis and
    gets the full bound, as a slot's first call does"""
    f = omc.load().omc_cone_multi_budget
    assert f(0) == 30                           # a quiet interval, or nothing known yet
    assert f(1) == 3 and f(5) == 7 and f(16) == 18      # warm calls
    assert f(28) == 30 and f(29) == 30 and f(30) == 30
    assert all(min(30, k + 2) == f(k) for k in range(1, 31))
