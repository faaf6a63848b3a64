"""Host side of the plain operations on the multi-workgroup eigen-kernels (omc_launch_cone_plain_mw): the plan omc_plain_multi_plan against
the layout arithmetic of csrc/omc_layout.h, the threshold the library reports, the declarations, and the golden error units that
tests/test_plain_multi.py reads (tests/golden/plain_multi_error_units.json, tools/record_plain_multi_error_units.py).  No GPU."""
import ctypes as C
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest

import omc_plain_ref as R
import plain_multi_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "optimalmatrixcompletion.jl_amd", "csrc")
SWEEPS = 30
UNITS_REL = 1e-3
# mw_layout, as csrc/omc_layout.h states it: the lines mirrored by _layout below must stand verbatim in the source
LAYOUT_LINES = [
    "#define MW_B 16 ",
    "#define MW_MIN_ORDER 145 ",
    "#define MW_MAX_ORDER 4096",
    "#define MW_PLAIN_SWEEPS 30 ",
    "const int NP = (N + 15) & ~15, Ncp = (N + 2 * MW_B - 1) & ~(2 * MW_B - 1), ld = NP + 4;",
    "const size_t ev = (size_t)Ncp * ld, sel = ev + 3 * (size_t)Ncp, smax = sel + Ncp / 2, head = smax + MW_MAXSW;",
    "OMC_HD int mw_plain_launches(const MwLayout& L, int sweeps) { return sweeps * (L.nb - 1) + 4; }",
]


def _layout(N):
    NP = (N + 15) & ~15; Ncp = (N + 31) & ~31; ld = NP + 4
    head = Ncp * ld + 3 * Ncp + Ncp // 2 + 32
    return dict(NP=NP, Ncp=Ncp, nb=Ncp // 16, slab_bytes=(head + 4) * 8, launches=SWEEPS * (Ncp // 16 - 1) + 4)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(HERE, "golden", "plain_multi_error_units.json")) as f:
        return json.load(f)["cases"]


def test_entries_declared_exported_and_listed(omc):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "omc.h")).read(), flags=re.S)
    lib = omc.load()
    for name in ("omc_plain_multi_plan", "omc_plain_multi_tau", "omc_last_plain_multi_stats"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in omc.EXPORTS
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read(), name
    out = np.zeros(4, np.int64)
    assert lib.omc_plain_multi_plan(145, 145, None) == -3
    assert lib.omc_plain_multi_plan(0, 145, out.ctypes.data_as(C.c_void_p)) == -3
    assert lib.omc_last_plain_multi_stats(None, out.ctypes.data_as(C.c_void_p)) == -3
    host = open(os.path.join(CSRC, "omc_host.h")).read()
    assert "int plain_multi_min = 1025;" in host and '{"OMC_PLAIN_MULTI_MIN", nullptr, &Tuning::plain_multi_min}' in host
    assert "OMC_PLAIN_MULTI_MIN" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_tau_is_the_cold_kernels_or_a_stated_power_of_ten_up_to_1e_12(omc):
    tau = omc.pkg.api.plain_multi_tau()
    assert tau in (1e-14, 1e-13, 1e-12), tau
    assert ("#define MW_TAU_PLAIN %g " % tau) in open(os.path.join(CSRC, "omc_layout.h")).read()


def test_plan_thresholds(omc):
    plan = omc.pkg.api.plain_multi_plan
    for knob in (1, 100, 144, 145, 1025, 4096):
        assert not plan(144, knob)["multi"], knob          # LDS-resident for k_cone_ws: never
        assert not plan(2, knob)["multi"] and not plan(4097, knob)["multi"], knob
    for knob in (-5, 0, 1, 144, 145):
        assert plan(145, knob)["multi"], knob
    assert not plan(145, 146)["multi"]
    assert not plan(1024)["multi"] and plan(1025)["multi"]                      # the default knob
    assert plan(1040)["multi"] and plan(4096)["multi"] and not plan(4097)["multi"]
    assert plan(4096, 4096)["multi"] and not plan(4095, 4096)["multi"]
    assert not plan(4096, 4097)["multi"]


def test_plan_follows_mw_layout(omc):
    src = open(os.path.join(CSRC, "omc_layout.h")).read()
    assert [ln for ln in LAYOUT_LINES if ln not in src] == []
    for N in [144, 145, 159, 160, 161, 176, 177, 192, 257, 514, 1000, 1024, 1025, 1040, 2000, 4096]:
        got = omc.pkg.api.plain_multi_plan(N, 145)
        want = _layout(N)
        assert {q: got[q] for q in want} == want, (N, got, want)
    # the shapes the GPU test relies on
    assert (_layout(145)["NP"], _layout(145)["Ncp"]) == (160, 160)
    assert (_layout(160)["NP"], _layout(160)["Ncp"], _layout(160)["nb"]) == (160, 160, 10)
    assert (_layout(161)["NP"], _layout(161)["Ncp"]) == (176, 192)
    assert (_layout(176)["NP"], _layout(176)["Ncp"]) == (176, 192)
    assert _layout(1040)["nb"] == 66 and _layout(1040)["launches"] == 30 * 65 + 4


def test_golden_file_holds_every_case_of_the_gpu_test(gold):
    """Every input with a reference has an entry that belongs to it: same seed, same ||M||_F."""
    ins = PC.all_inputs()
    assert sorted(key for key, _, _, _ in ins) == sorted(gold)
    assert {N for _, _, N, _ in ins} == set(PC.SMALL_ORDERS + [PC.BIG_ORDER])
    for key, seed, N, build in ins:
        rec = gold[key]
        assert rec["seed"] == seed, key
        f = R.fro(build()[0])
        assert abs(f - rec["fro"]) <= 1e-9 * max(f, rec["fro"]), key
        assert rec["units"] > 0.0 and 1 <= rec["sweeps"] < R.MAX_SWEEPS, (key, rec)
    big = [key for key, _, N, _ in ins if N == PC.BIG_ORDER]
    assert sorted(big) == sorted(["sep/1040/%s" % f for f in PC.BIG_SEP_FAMILIES] + ["round/1040/k2/%s" % f for f in PC.BIG_ROUND_FAMILIES])


def test_tool_reproduces_the_entries_of_order_145(gold):
    """The restatement is plain numpy arithmetic, so ||M||_F and its sweeps repeat exactly.  At every one of these inputs e_ref is the
    restatement's error (LAPACK's on the shifted matrix is at most 0.47 of it), so the units repeat too, up to what another BLAS changes in
    LAPACK's eigenvectors, which enter only through the long-double Rayleigh quotients: those are good to 1e-19 ||M|| against an e_ref of
    500 u ||M|| and more, 1e-5 of a unit.  Seen with 1 and with 8 BLAS threads: no difference at all.  UNITS_REL leaves a hundred times that."""
    spec = importlib.util.spec_from_file_location("record_plain_multi_error_units", os.path.join(ROOT, "tools", "record_plain_multi_error_units.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    keys = [key for key, _, _, _ in PC.all_inputs([145])]
    assert len(keys) == 9 + 3 + 4 + 3 + 2 and keys == [key for key, _, N, _ in PC.all_inputs() if N == 145]
    for i, key in enumerate(keys):
        k2, rec = tool._measure(([145], i))
        ref = gold[key]
        assert k2 == key and rec["seed"] == ref["seed"]
        assert abs(rec["fro"] - ref["fro"]) <= 1e-12 * ref["fro"], key
        assert rec["sweeps"] == ref["sweeps"], (key, rec, ref)
        assert abs(rec["units"] / ref["units"] - 1.0) <= UNITS_REL, (key, rec, ref)
    assert math.isfinite(sum(gold[k]["units"] for k in gold))
