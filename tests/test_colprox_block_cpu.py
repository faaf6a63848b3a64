"""CPU tests of the block column prox (csrc/omc_colprox_block.hip): the two entries exist and refuse bad arguments before any device call,
and the launch plan that host and kernel take from one layout definition (CpBlockLayout, csrc/omc_layout.h) keeps its promises.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DYN_LDS = 144 * 1024
TILE = 256      # doubles of a 16 x 16 tile


def test_entries_declared_exported_and_listed(omc):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "omc.h")).read(), flags=re.S)
    lib = omc.load()
    for name in ("omc_column_prox_batch", "omc_colprox_plan"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in omc.EXPORTS


def test_argument_checks_come_before_any_device_call(omc):
    lib = omc.load()
    nul = [None] * 9
    assert lib.omc_column_prox_batch(None, 1, 0, 0, *nul) == -3 and b"handle" in lib.omc_last_error()
    assert lib.omc_column_prox_batch(None, 1, 2, 0, *nul) == -3 and b"mode" in lib.omc_last_error()
    assert lib.omc_column_prox_batch(None, 1, -1, 0, *nul) == -3 and b"mode" in lib.omc_last_error()
    assert lib.omc_column_prox_batch(None, 1, 0, 3, *nul) == -3 and b"algo" in lib.omc_last_error()
    assert lib.omc_column_prox_batch(None, 1, 1, -1, *nul) == -3 and b"algo" in lib.omc_last_error()
    out = np.zeros(5, np.int64)
    assert lib.omc_colprox_plan(100, 50, 65, None) == -3
    assert lib.omc_colprox_plan(100, 101, 65, out.ctypes.data_as(C.c_void_p)) == -3      # a column cannot be longer than n
    assert lib.omc_colprox_plan(0, 0, 65, out.ctypes.data_as(C.c_void_p)) == -3


def test_plan_properties(omc):
    plan = omc.pkg.api.colprox_plan
    n = 1000
    lds_cmax = plan(n, 300)["lds_cmax"]
    assert lds_cmax % 16 == 0 and lds_cmax == 176      # 66 tiles of 2 KiB and the vectors under 144 KiB; 78 tiles alone are above
    slab_cmax = max(c for c in range(1, n + 1) if plan(n, c, 1)["block"])
    assert slab_cmax % 16 == 0 and slab_cmax > 340       # config 5 (c ~ 300) is inside
    for c in list(range(1, 260)) + [300, 340, slab_cmax]:
        p = plan(n, c, 1)
        nb = (c + 15) // 16
        assert p["block"] and 0 < p["lds_bytes"] <= MAX_DYN_LDS and p["workgroups_per_cu"] >= 1
        if c <= lds_cmax:
            assert p["slab_doubles"] == 0 and p["lds_bytes"] >= 8 * (TILE * nb * (nb + 1) // 2 + 5 * c)      # the tiles and five vectors fit the launch
        else:
            assert p["slab_doubles"] >= TILE * nb * (nb + 1) // 2 and p["lds_bytes"] >= 8 * (TILE * (nb - 1) + 5 * c)      # L in the slab, a panel and the vectors in LDS
    assert plan(n, lds_cmax)["slab_doubles"] == 0 and plan(n, lds_cmax + 1)["slab_doubles"] > 0
    assert not plan(n, slab_cmax + 1, 1)["block"]       # beyond the kernel: the column stays with k_colprox
    for c in (1, 64, 65, 300):
        for bm in (c + 1, 100000):
            p = plan(n, c, bm)
            assert not p["block"] and p["lds_bytes"] == 0 and p["slab_doubles"] == 0      # block_min above cmax: no block columns
    assert not plan(n, 64)["block"] and plan(n, 65)["block"]      # the default knob
