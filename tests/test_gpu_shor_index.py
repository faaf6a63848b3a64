"""GPU tests of the device builder of a Shor list's index structure (omc_shor_index.hip, OMC_SHOR_INDEX_DEVICE_MIN, omc_shor_index_build;
DESIGN.md 3.7a).  Run on the MI355X box: `pytest -m gpu`.

Everything is integer work, so every comparison is bit identity (np.array_equal / ==) over every array and count: the device builder
(where = 1) against the host builder (where = 0) and against the numpy restatement of tests/shor_index_ref.py; the refusals and their
messages; and whole solves and bounds with the knob at 1 against the knob at 0.

The sort works on tiles of T = 1024 items (omc_shor_index_plan reports it).  A list of nq minors sorts 2 nq and 4 nq items, an even number
and a multiple of four, so the lengths "T - 1, T + 1, 2 T + 1" of the issue are met by their nearest neighbours: nq = 511, 512, 513, 1025
(2 nq = T - 2, T, T + 2, 2 T + 2) and nq = 255, 256, 257, 513 (4 nq = T - 4, T, T + 4, 2 T + 4).
The library takes n <= m only, so the 299 minors (1, i2, 1, 2) of the issue's 300 x 4 case live in a 300 x 300 instance: one V1 key with 299
members, two coordinates with 299 members each, as there."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shor_index_ref as ref      # noqa: E402

pytestmark = pytest.mark.gpu
GAMMA = 80.0
KNOB = "OMC_SHOR_INDEX_DEVICE_MIN"
SEVEN = [(1, 1), (10, 12), (3, 4), (5, 6), (2, 11), (9, 1), (3, 4)]


@pytest.fixture(scope="module")
def have_gpu(omc):
    if omc.load().omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


class Env:
    pass


def _engine(have_gpu, omc, orc, name):
    e = Env()
    e.A, e.mask, e.minors = ref.instance(orc, name)
    e.n, e.m = e.mask.shape
    e.eng = omc.Engine(e.A, e.mask, GAMMA, 1)
    return e


@pytest.fixture(scope="module")
def e10(have_gpu, omc, orc):
    e = _engine(have_gpu, omc, orc, "10x12")
    yield e
    e.eng.close()


@pytest.fixture(scope="module")
def e12(have_gpu, omc, orc):
    e = _engine(have_gpu, omc, orc, "12x14")
    yield e
    e.eng.close()


def three_way(eng, mask, lst, soc, tag):
    """device == host == numpy over every array and count; r4 and hash of the two builders too"""
    n, m = mask.shape
    d = eng.shor_index(lst, soc, where="device")
    h = eng.shor_index(lst, soc, where="host")
    r = ref.build(n, m, mask, lst, soc)
    assert ref.same(d, h) == [], (tag, "device / host", ref.same(d, h))
    assert ref.same(d, r) == [], (tag, "device / numpy", ref.same(d, r))
    assert d["r4"] == h["r4"] and d["hash"] == h["hash"], tag
    assert d["launches"] == eng.shor_index_plan(len(lst))["launches"] and h["launches"] == 0, (tag, d["launches"])
    return d


# ---- structure ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soc", [None, [], SEVEN], ids=["soc=-1", "soc=0", "soc=7"])
def test_10x12_list_in_every_order(e10, soc):
    for vname, lst in ref.variants(e10.minors).items():
        three_way(e10.eng, e10.mask, lst, soc, ("10x12", vname))


def test_6x7_column_types(have_gpu, omc, orc):
    A, mask, minors = ref.instance(orc, "6x7")
    eng = omc.Engine(A, mask, GAMMA, 1)
    try:
        d = three_way(eng, mask, minors, None, "6x7 full")
        assert (d["ctype"] == 2).all() and (d["slackrow"] == -1).all()
        d = three_way(eng, mask, minors[:1], None, "6x7 one")
        assert (d["ctype"] == 1).all()
        three_way(eng, mask, minors[::-1].copy(), [], "6x7 reversed")
    finally:
        eng.close()
    mask2 = mask.copy(); mask2[4, 2] = False          # one entry of column 3 unobserved
    eng = omc.Engine(A, mask2, GAMMA, 1)
    try:
        d = three_way(eng, mask2, minors[:1], None, "6x7 one, hole")
        assert d["ctype"][2] == 0 and d["slackrow"][2] == 4 and (np.delete(d["ctype"], 2) == 1).all()
    finally:
        eng.close()


def test_prefix_lengths_around_the_tile_sizes(e12):
    T = e12.eng.shor_index_plan(1)["tile"]
    lengths = {127, 128, 129, 255, 256, 257, T // 2 - 1, T // 2, T // 2 + 1, T + 1, T // 4 - 1, T // 4, T // 4 + 1, T // 2 + 1}
    assert max(lengths) <= len(e12.minors)
    rng = np.random.default_rng(1)
    perm = e12.minors[rng.permutation(len(e12.minors))]
    for nq in sorted(lengths):
        three_way(e12.eng, e12.mask, e12.minors[:nq], None, ("12x14 prefix", nq))
        three_way(e12.eng, e12.mask, perm[:nq], [], ("12x14 permuted prefix", nq))
    three_way(e12.eng, e12.mask, perm, None, "12x14 whole list, permuted")


def test_one_key_with_299_members(have_gpu, omc):
    n = m = 300
    rng = np.random.default_rng(11)
    A = rng.standard_normal((n, 1)) @ rng.standard_normal((1, m))
    mask = rng.random((n, m)) < 0.5
    mask[np.arange(n), np.arange(n)] = True
    lst = np.array([(1, i2, 1, 2) for i2 in range(2, n + 1)], np.int64)
    eng = omc.Engine(A, mask, GAMMA, 1)
    try:
        for tag, l in (("forward", lst), ("reversed", lst[::-1].copy())):
            d = three_way(eng, mask, l, None, ("300", tag))
            assert np.diff(d["v1ptr"]).max() == 299 and sorted(np.diff(d["cptr"]))[-2:] == [299, 299]
    finally:
        eng.close()


def test_keys_beyond_32_bits(have_gpu, omc):
    """70 x 8000: V1 keys pass 2^32 (five passes), so the upper digits are sorted.  One instance for all assertions."""
    n, m = 70, 8000
    rng = np.random.default_rng(5)
    A = rng.standard_normal((n, 1)) @ rng.standard_normal((1, m))
    mask = rng.random((n, m)) < 0.3
    mask[rng.integers(0, n, m), np.arange(m)] = True
    mask[np.arange(n), np.arange(n)] = True
    rows, cols = [1, 2, 69, 70], [1, 2, 7999, 8000]
    lst = np.array([(rows[a], rows[b], cols[c], cols[d]) for a in range(4) for b in range(a + 1, 4) for c in range(4) for d in range(c + 1, 4)], np.int64)
    assert len(lst) == 36
    t0 = time.time()
    eng = omc.Engine(A, mask, GAMMA, 1)
    print(f"  70 x 8000 instance created in {time.time() - t0:.2f} s")
    try:
        assert eng.shor_index_plan(36)["passes_v1"] == 5
        rng2 = np.random.default_rng(6)
        for tag, l in (("forward", lst), ("reversed", lst[::-1].copy()), ("permuted", lst[rng2.permutation(36)])):
            d = three_way(eng, mask, l, None, ("70x8000", tag))
            assert ((d["mi"][1].astype(np.int64) * m + d["mi"][2]) * m + d["mi"][3]).max() >= 2 ** 32
        three_way(eng, mask, lst, [(70, 8000), (1, 1), (35, 4000)], "70x8000 soc")
    finally:
        eng.close()


def test_same_list_three_times(e12):
    runs = [e12.eng.shor_index(e12.minors, None, where="device") for _ in range(3)]
    assert ref.same(runs[0], runs[1]) == [] and ref.same(runs[0], runs[2]) == []


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _bad_lists(e):
    ok = e.minors[:20]
    add = lambda *t: np.concatenate([ok, np.array(t, np.int64).reshape(-1, 4)])      # noqa: E731
    return [("i1 = i2", add((2, 2, 1, 2)), None, ref.MSG_RANGE), ("j2 = m + 1", add((1, 2, 1, e.m + 1)), None, ref.MSG_RANGE),
            ("an index 0", add((0, 2, 1, 2)), None, ref.MSG_RANGE), ("a duplicate", add(tuple(ok[3])), None, ref.MSG_DUP),
            ("out of range and a duplicate", add(tuple(ok[3]), (1, 2, 1, e.m + 1)), None, ref.MSG_RANGE),
            ("SOC row n + 1", ok, [(1, 1), (e.n + 1, 1)], ref.MSG_SOC)]


def _refusal(omc, call):
    with pytest.raises(omc.OmcError) as err:
        call()
    return err.value.code, str(err.value)


def test_refusals_are_the_host_builders(e10, omc):
    e = e10; eng = e.eng
    P = omc.default_params(max_iters=100, slots=2)
    for tag, lst, soc, msg in _bad_lists(e):
        host = _refusal(omc, lambda: eng.shor_index(lst, soc, where="host"))
        dev = _refusal(omc, lambda: eng.shor_index(lst, soc, where="device"))
        eng.tuning_set(KNOB, "1")
        try:
            staged = _refusal(omc, lambda: eng.stage_shor([[], []], [(e.minors, None), (lst, soc)], "linear", P))
            assert eng.shor_index_stats()["device_lists"] == 1 and eng.shor_index_stats()["host_lists"] == 0      # the good list before it
        finally:
            eng.tuning_set(KNOB, None)
        assert host[0] == -3 and msg in host[1], (tag, host)
        assert dev == host and staged == host, (tag, host, dev, staged)
        with pytest.raises(ValueError, match=msg[:20]):
            ref.build(e.n, e.m, e.mask, lst, soc)


# ---- end to end: knob 1 against knob 0 ---------------------------------------------------------------------------------------------------------
ORDER = ["root/208", "left/208", "right/208", "root/104", "left/104", "right/104"]


def _key(o):
    return (o["objective"], o["dual_bound"], o["iters"], o["status_code"])


def _collect(eng, lists):
    out = eng.fetch(want_Y=False, want_X=True, want_Theta=True)
    for r, W in zip(out, eng.fetch_shor()):
        r["W"] = W
    for r, V, l in zip(out, eng.fetch_shor_V(), lists):
        r["V"] = V[:len(l)]
    return out


@pytest.fixture(scope="module")
def six(e10, omc, orc):
    """The six (cut, list) nodes of tests/test_gpu_shor_append.py: the cut is the oracle's root breakpoint vector (computed once)"""
    import omc_oracle_shor as sh
    e = e10
    inst = orc.Instance(e.A, e.mask, GAMMA, 1)
    full, soc = sh.driver_shor_lists(e.mask, (4,))
    t0 = time.time()
    o_root = sh.sdp_relaxation_shor(inst, full, soc, params=sh.ShorParams(eps_gap=1e-5, max_iters=6000))
    print(f"  oracle root: {time.time() - t0:.1f} s")
    x = orc.breakpoint_vector(o_root["Y"], o_root["U"])[0]
    left = [(x, o_root["U"], ["left"])]; right = [(x, o_root["U"], ["right"])]
    e.nodes = [[], left, right, [], left, right]
    e.lists = [full] * 3 + [full[:104]] * 3
    e.info = [(l, None) for l in e.lists]
    e.P2 = omc.default_params(eps_gap=1e-5, max_iters=100, rho_scale=1.0, slots=2)
    e.omc_params = omc.default_params
    return e


def _arm(e, arm):
    eng = e.eng
    if arm == "staged":
        eng.stage_shor(e.nodes, e.info, "linear", e.P2, keep_V=True)
        stats = eng.shor_index_stats()
        eng.solve()
        return _collect(eng, e.lists), stats
    running = arm == "running"
    if running:
        eng.tuning_set("OMC_NO_GRAPH", "1")
    try:
        eng.reserve(4, 1); eng.reserve_shor(208, 1)
        eng.stage_shor(e.nodes[:2], e.info[:2], "linear", e.P2, keep_V=True)
        if running:
            eng.hold(True); eng.submit()
        eng.append_shor(e.nodes[2:4], e.info[2:4], "linear")
        eng.append_shor(e.nodes[4:], e.info[4:], "linear")
        stats = eng.shor_index_stats()
        if running:
            eng.hold(False); eng.wait()
        else:
            eng.solve()
    finally:
        if running:
            eng.tuning_set("OMC_NO_GRAPH", None)
    return _collect(eng, e.lists), stats


@pytest.mark.parametrize("arm", ["staged", "appended", "running"])
def test_solves_are_bit_identical_with_the_knob_on_and_off(six, arm):
    """max_iters = 100: the status at the cap is whatever it is, on both sides"""
    e = six
    got = {}
    for knob in ("1", None):
        e.eng.tuning_set(KNOB, knob)
        try:
            got[knob] = _arm(e, arm)
        finally:
            e.eng.tuning_set(KNOB, None)
    (on, s_on), (off, s_off) = got["1"], got[None]
    assert (s_on["device_lists"], s_on["host_lists"]) == (2, 0), s_on          # the knob did take the device path
    assert (s_off["device_lists"], s_off["host_lists"]) == (0, 2), s_off
    assert len(on) == len(off) == 6
    for nm, a, b in zip(ORDER, on, off):
        assert _key(a) == _key(b), (arm, nm, _key(a), _key(b))
        for q in ("X", "W", "Theta", "V"):
            assert np.array_equal(a[q], b[q]), (arm, nm, q)


def test_dual_bounds_are_equal_with_the_knob_on_and_off(six):
    """Engine.shor_dual_bound on the certificates of the six staged nodes: equal doubles under both knob values, and with the knob at 1 its two
    lists were built on the device.  At max_iters = 100 no node has reached a rigorous check, so there is no certificate to fetch there
    (omc_relax_fetch_shor_certificate refuses); the certificates come from one solve of the same six nodes at the cap of
    tests/test_gpu_shor_append.py (eps_gap 1e-5, at most 6000 iterations, where all six certify)."""
    e = six; eng = e.eng
    P = e.omc_params(eps_gap=1e-5, max_iters=6000, rho_scale=1.0, slots=2)
    eng.keep_shor_certificates(True)
    try:
        t0 = time.time()
        eng.stage_shor(e.nodes, e.info, "linear", P)
        eng.solve()
        certs = eng.fetch_shor_certificate(list(range(6)))
        print(f"  six nodes to certificates: {time.time() - t0:.1f} s")
    finally:
        eng.keep_shor_certificates(False)
    before = eng.shor_index_stats()
    eng.tuning_set(KNOB, "1")
    try:
        on, d_on = eng.shor_dual_bound(e.nodes, e.info, certs, want_defects=True)
    finally:
        eng.tuning_set(KNOB, None)
    mid = eng.shor_index_stats()
    off, d_off = eng.shor_dual_bound(e.nodes, e.info, certs, want_defects=True)
    after = eng.shor_index_stats()
    assert (mid["device_lists"] - before["device_lists"], mid["host_lists"] - before["host_lists"]) == (2, 0)
    assert (after["device_lists"] - mid["device_lists"], after["host_lists"] - mid["host_lists"]) == (0, 2)
    assert np.isfinite(on).all() and np.array_equal(np.asarray(on), np.asarray(off)), (on, off)
    assert d_on == d_off          # min_zeta reads ctype on the host: copied back from the device-built list


def test_a_refused_append_leaves_the_batch_as_it_was(six, omc):
    """Knob at 1: two nodes staged, every bad list refused as an append (host messages), then the four valid nodes appended: the results equal
    the batch staged as a whole with the knob at 0."""
    e = six; eng = e.eng
    eng.stage_shor(e.nodes, e.info, "linear", e.P2, keep_V=True)
    eng.solve()
    want = _collect(eng, e.lists)
    eng.tuning_set(KNOB, "1")
    try:
        eng.reserve(4, 1); eng.reserve_shor(208, 1)
        eng.stage_shor(e.nodes[:2], e.info[:2], "linear", e.P2, keep_V=True)
        for tag, lst, soc, msg in _bad_lists(e):
            code, text = _refusal(omc, lambda: eng.append_shor([[]], [(lst, soc)], "linear"))
            assert code == -3 and msg in text, (tag, code, text)
        eng.append_shor(e.nodes[2:], e.info[2:], "linear")
        assert eng.shor_index_stats()["device_lists"] == 2
        eng.solve()
        got = _collect(eng, e.lists)
    finally:
        eng.tuning_set(KNOB, None)
    for nm, a, b in zip(ORDER, got, want):
        assert _key(a) == _key(b), (nm, _key(a), _key(b))
        for q in ("X", "W", "Theta", "V"):
            assert np.array_equal(a[q], b[q]), (nm, q)
