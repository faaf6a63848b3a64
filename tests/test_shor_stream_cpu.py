"""CPU part of the streaming violated-minor selection: the entry point that reports how the last call selected is declared,
exported, bound, and checks its arguments before it touches a device."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_stats_symbol_is_declared_exported_and_listed(omc):
    hdr = open(os.path.join(ROOT, "include", "omc.h")).read()
    assert re.search(r"\bint\s+omc_shor_last_select_stats\s*\(\s*omc_instance\s*\*\s*h\s*,\s*int64_t\s+out\[4\]\s*\)\s*;", hdr)
    lib = omc.load()
    assert hasattr(lib, "omc_shor_last_select_stats")
    assert "omc_shor_last_select_stats" in omc.EXPORTS
    assert hasattr(omc.Engine, "shor_last_select_stats")


def test_select_stats_null_arguments_are_refused(omc):
    lib = omc.load()
    out = np.zeros(4, dtype=np.int64)
    assert lib.omc_shor_last_select_stats(None, out.ctypes.data) == -3          # OMC_ERR_ARGUMENT
    assert b"NULL" in lib.omc_last_error()
    assert lib.omc_shor_last_select_stats(None, None) == -3
    assert not out.any()
