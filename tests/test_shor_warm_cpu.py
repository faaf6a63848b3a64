"""CPU tests of the Shor-mode warm start's boundary: the new entry points are declared, exported and listed; NULL handles are refused
before any device call; omc_shor_warm_compat (a pure host function, the one rule the library applies at stage time) on every case of
its contract.  Lists are in the wire format of omc_relax_stage_shor: 1-based Int64 (i1, i2, j1, j2) tuples and (i, j) pairs."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["omc_state_pool_reserve_shor", "omc_shor_warm_compat", "omc_last_shor_warm_stats", "omc_state_pool_fetch_shor"]


def test_new_entry_points_are_declared_exported_and_listed(omc):
    hdr = open(os.path.join(ROOT, "include", "omc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(omc_[A-Za-z0-9_]+)\s*\(", hdr))
    lib = omc.load()
    for s in NEW:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in omc.EXPORTS, s


def test_null_handles_are_refused_before_any_device_call(omc):
    lib = omc.load()
    nq = np.zeros(1, np.int64)
    assert lib.omc_state_pool_reserve_shor(None, 1) == -3
    assert lib.omc_state_pool_fetch_shor(None, 0, omc.pkg._lib.ptr(nq), None, None, None) == -3
    assert lib.omc_last_shor_warm_stats(None, omc.pkg._lib.ptr(np.zeros(4, np.int64))) == -3


def _compat(omc, parent, psoc, child, csoc):
    """psoc / csoc: None = the complement shorthand (n_soc = -1), else a list of pairs."""
    lib = omc.load(); ptr = omc.pkg._lib.ptr
    def lst(a, w):
        a = np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1, w))
        return len(a), (ptr(a) if len(a) else None), a
    npar, pp, _k1 = lst(parent, 4); nch, cp, _k2 = lst(child, 4)
    nps, psp, _k3 = (-1, None, None) if psoc is None else lst(psoc, 2)
    ncs, csp, _k4 = (-1, None, None) if csoc is None else lst(csoc, 2)
    return lib.omc_shor_warm_compat(npar, pp, nps, psp, nch, cp, ncs, csp)


def test_shor_warm_compat_rule(omc):
    L = [(1, 2, 1, 2), (1, 3, 1, 2), (2, 3, 2, 4), (1, 2, 3, 4), (2, 4, 1, 3)]
    soc = [(1, 5), (2, 5), (3, 1)]
    assert _compat(omc, L, None, L, None) == 1                        # identical lists, complement SOC
    assert _compat(omc, L, soc, L, soc) == 1                          # identical lists, identical explicit SOC
    assert _compat(omc, L, soc, L, soc[:2]) == 0                      # same minors, another SOC list
    assert _compat(omc, L, None, L, soc) == 0
    assert _compat(omc, L[:3], None, L, None) == 2                    # strict prefix, complement SOC on both sides
    changed = [L[0], (1, 3, 1, 3), L[2]]
    assert _compat(omc, changed, None, L, None) == 0                  # the prefix with one tuple changed
    assert _compat(omc, L, None, L[:3], None) == 0                    # child shorter than parent
    assert _compat(omc, L[:3], soc, L, None) == 0                     # a prefix with an explicit SOC list on either side
    assert _compat(omc, L[:3], None, L, soc) == 0
    assert _compat(omc, L[:3], soc, L, soc) == 0
    assert _compat(omc, [], None, [], None) == 1                      # two empty lists
    assert _compat(omc, [], None, L, None) == 2                       # empty parent, non-empty child, complement SOC
    assert _compat(omc, [], soc, L, None) == 0
    assert _compat(omc, L[1:4], None, L, None) == 0                   # a sub-list that is not a prefix


def test_pool_byte_formula_matches_the_header(omc):
    """Engine.shor_state_bytes is the formula include/omc.h states (bnb sizes its pool with it)."""
    hdr = open(os.path.join(ROOT, "include", "omc.h")).read()
    assert "8 (3 n m + m^2 + (n + m)^2 + 2 m + 20 nq_max) bytes" in hdr
    n, m, q = 10, 12, 208
    assert omc.Engine.shor_state_bytes(n, m, q) == 8 * (3 * n * m + m * m + (n + m) ** 2 + 2 * m + 20 * q) + 32
