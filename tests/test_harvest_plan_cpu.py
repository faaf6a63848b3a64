"""CPU tests of omc_harvest_plan, the host rule by which omc_relax_solve treats the finished slots at a certificate check: leave them
parked, harvest and refill before the next iteration (synchronous), or enqueue the harvest kernels beside the next interval and book
and refill at the next check (asynchronous).  No device call, no handle."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, SYNC, ASYNC = 0, 1, 2

# (nlive, nfin, pending, check_index, async_min_live) -> plan
CASES = [
    # nothing has finished: nothing to do, whatever else holds
    ((1000, 0, 1, 3, 256), NONE), ((0, 0, 1, 3, 256), NONE), ((1000, 0, 0, 12, 256), NONE),
    # nothing is left running: at once and waited for, at any check, with or without pending nodes, whatever the threshold
    ((0, 5, 1, 1, 256), SYNC), ((0, 5, 0, 7, 256), SYNC), ((0, 1024, 1, 2, 1), SYNC),
    # pending nodes, the chip full: every third check only
    ((1000, 24, 1, 1, 256), NONE), ((1000, 24, 1, 2, 256), NONE), ((1000, 24, 1, 3, 256), ASYNC), ((1000, 24, 1, 4, 256), NONE),
    ((1000, 24, 1, 6, 256), ASYNC), ((1000, 24, 1, 300, 256), ASYNC),
    # the threshold itself: 256 live slots are asynchronous, 255 are not -- and 255 no longer fill the chip, so they do not wait for a third check
    ((256, 24, 1, 3, 256), ASYNC), ((256, 24, 1, 4, 256), NONE), ((255, 24, 1, 3, 256), SYNC), ((255, 24, 1, 4, 256), SYNC),
    ((1, 3, 1, 5, 256), SYNC),
    # a lower threshold moves the asynchronous path down, not the cadence: below 256 live slots every check harvests
    ((3, 1, 1, 1, 1), ASYNC), ((3, 1, 1, 2, 1), ASYNC), ((100, 4, 1, 4, 64), ASYNC), ((63, 4, 1, 4, 64), SYNC),
    # a higher one keeps a full chip synchronous
    ((600, 24, 1, 3, 1024), SYNC), ((1024, 24, 1, 3, 1024), ASYNC),
    # no pending nodes: every twelfth check
    ((1000, 24, 0, 3, 256), NONE), ((1000, 24, 0, 11, 256), NONE), ((1000, 24, 0, 12, 256), ASYNC), ((1000, 24, 0, 24, 256), ASYNC),
    ((100, 24, 0, 6, 256), NONE), ((100, 24, 0, 12, 256), SYNC),
    # the asynchronous path switched off (the caller passes 0 for OMC_HARVEST_ASYNC=0): the cadence alone
    ((1000, 24, 1, 3, 0), SYNC), ((1000, 24, 1, 4, 0), NONE), ((1000, 24, 0, 12, 0), SYNC), ((1000, 24, 1, 3, -5), SYNC),
]


def test_harvest_plan_is_declared_exported_and_listed(omc):
    hdr = open(os.path.join(ROOT, "include", "omc.h")).read()
    hdr_code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bomc_harvest_plan\s*\(", hdr_code)
    assert hasattr(omc.load(), "omc_harvest_plan") and "omc_harvest_plan" in omc.EXPORTS
    for name, val in (("OMC_HARVEST_NONE", NONE), ("OMC_HARVEST_SYNC", SYNC), ("OMC_HARVEST_ASYNC", ASYNC)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name


@pytest.mark.parametrize("args,want", CASES)
def test_harvest_plan_table(omc, args, want):
    assert omc.load().omc_harvest_plan(*args) == want, args


def test_harvest_plan_against_the_rule_it_replaces(omc):
    """With the asynchronous path off the function is the rule the solve loop applied before it existed: harvest when something has
    finished and (nothing runs, or with pending nodes at every third check or below 256 live slots, or without at every twelfth)."""
    f = omc.load().omc_harvest_plan
    for nlive in (0, 1, 255, 256, 257, 1024):
        for nfin in (0, 1, 24):
            for pending in (0, 1):
                for ci in range(1, 26):
                    now = nfin > 0 and (nlive == 0 or ((ci % 3 == 0 or nlive < 256) if pending else ci % 12 == 0))
                    assert f(nlive, nfin, pending, ci, 0) == (SYNC if now else NONE)
                    got = f(nlive, nfin, pending, ci, 256)
                    assert (got != NONE) == now and (got == ASYNC) == (now and nlive >= 256)


def test_host_phase_names_cover_the_new_counters(omc):
    hdr = open(os.path.join(ROOT, "include", "omc.h")).read()
    nphase = int(re.search(r"#define\s+OMC_HOST_NPHASE\s+(\d+)", hdr).group(1))
    names = omc.pkg.api.HOST_PHASES
    assert len(names) == nphase
    assert names[int(re.search(r"#define\s+OMC_HOST_ASYNC_HARVESTS\s+(\d+)", hdr).group(1))] == "async_harvests"
    assert names[int(re.search(r"#define\s+OMC_HOST_QUIET_INTERVALS\s+(\d+)", hdr).group(1))] == "quiet_intervals"
