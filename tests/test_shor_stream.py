"""Streaming selection of the violated Shor minors (knob OMC_SHOR_SELECT_KB): the same minors and the same doubles as the
materialised selection and as the oracle, with device memory bounded by the budget instead of by the number of candidates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GAMMA = 80.0
SEL_CAP = 8192                 # slack of the radix select (SHOR_SEL_CAP in omc_api_minors.cpp): it stops refining once at most this many extra keys remain


@pytest.fixture(scope="module")
def have_gpu(omc):
    lib = omc.load()
    if lib.omc_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (the HIP path has no CPU fallback)")
    return True


def _shor_instance(omc, n, m, k, frac, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, m)) < frac
    mask[rng.integers(0, n, m), np.arange(m)] = True
    mask[np.arange(n), rng.integers(0, m, n)] = True
    A = rng.standard_normal((n, m))
    return A, mask, omc.Engine(A, mask, GAMMA, k)


def _pair_lists(mask):
    """|both|, |xor|, |none| of every row pair i1 < i2"""
    Mi = mask.astype(np.int64)
    both = Mi @ Mi.T; obs = Mi.sum(1); m = mask.shape[1]
    xor = obs[:, None] + obs[None, :] - 2 * both; none = m - obs[:, None] - obs[None, :] + both
    iu = np.triu_indices(mask.shape[0], 1)
    return both[iu], xor[iu], none[iu]


def _class_counts(mask):
    b, x, z = _pair_lists(mask)
    return {4: int((b * (b - 1) // 2).sum()), 3: int((b * x).sum()), 2: int((b * z).sum() + (x * (x - 1) // 2).sum()), 1: int((x * z).sum()),
            0: int((z * (z - 1) // 2).sum())}


def _largest_pair_count(mask):
    """largest number of candidates that one row pair contributes to one pass of the enumeration"""
    b, x, z = _pair_lists(mask)
    return int(max((b * (b - 1) // 2).max(), (b * x).max(), (b * z).max(), (x * (x - 1) // 2).max(), (x * z).max(), (z * (z - 1) // 2).max()))


@pytest.mark.parametrize("k", [1, 2])
def test_stream_bit_exact_against_oracle_tiles_forced(have_gpu, omc, orc, k):
    """The instances and cases of test_violated_shor_minors_bit_exact with a 1 KiB budget: every call streams, in more than one tile."""
    n, m = 10, 14
    A, mask, eng = _shor_instance(omc, n, m, k, 0.45, 10 + k)
    eng.tuning_set("OMC_SHOR_SELECT_KB", 1)
    rng = np.random.default_rng(5)
    cases = {"gauss": rng.standard_normal((k, n, m)), "ties": rng.integers(-2, 3, (k, n, m)).astype(float), "zero": np.zeros((k, n, m))}
    for name, X3 in cases.items():
        for cl in ([4], [4, 3], [3, 2, 1, 0, 4]):
            first = orc.violated_shor_minors(X3, mask, cl, [], 7)
            existing = [t for _, t in first[:5]] + [(1, 2, 1, 2), (n, n, m, m)]
            for ex, nm in (([], 7), (existing, 100), (existing, 10 ** 6), ([], 0)):
                want = orc.violated_shor_minors(X3, mask, cl, ex, nm)
                got = eng.generate_violated_Shor_minors(X3, cl, ex, nm)
                st = eng.shor_last_select_stats()
                print(name, cl, nm, len(got), st)
                assert len(got) == len(want), (name, cl, nm)
                assert [t for _, t in got] == [t for _, t in want], (name, cl, nm)
                assert [s for s, _ in got] == [s for s, _ in want], (name, cl, nm)      # identical doubles
                assert st["streamed"] == 1, (name, cl, nm, st)
                if nm > 0:                                   # n_minors = 0 returns before anything is enumerated
                    assert st["tiles"] > 1, (name, cl, nm, st)
    eng.close()


def _stream_vs_materialised(eng, X3, cl, ex, nm, budget_kb):
    eng.tuning_set("OMC_SHOR_SELECT_KB", 0)
    want = eng.generate_violated_Shor_minors(X3, cl, ex, nm)
    st0 = eng.shor_last_select_stats()
    eng.tuning_set("OMC_SHOR_SELECT_KB", budget_kb)
    got = eng.generate_violated_Shor_minors(X3, cl, ex, nm)
    st = eng.shor_last_select_stats()
    assert st0["streamed"] == 0 and st["streamed"] == 1, (st0, st)
    return want, got, st


def test_stream_bit_exact_against_materialised(have_gpu, omc):
    """60 x 80, 40 % observed, every class (5.6e6 candidates), k = 2, 64 KiB budget against budget 0.  The all-zero X is the worst case of
    the filter: every score ties, later row pairs of a pass carry larger tuples, so the threshold never keeps anything out for long."""
    n, m, k = 60, 80, 2
    A, mask, eng = _shor_instance(omc, n, m, k, 0.4, 21)
    cl = [4, 3, 2, 1, 0]
    rng = np.random.default_rng(6)
    cases = {"gauss": rng.standard_normal((k, n, m)), "ties": rng.integers(-2, 3, (k, n, m)).astype(float), "zero": np.zeros((k, n, m))}
    largest = _largest_pair_count(mask)
    for name, X3 in cases.items():
        eng.tuning_set("OMC_SHOR_SELECT_KB", 0)
        first = eng.generate_violated_Shor_minors(X3, cl, [], 50)
        assert len(first) == 50
        existing = [t for _, t in first] + [(0, 1, 1, 2), (n, n + 1, m, m)]
        for nm in (1, 100, 5000):
            want, got, st = _stream_vs_materialised(eng, X3, cl, existing, nm, 64)
            print(name, nm, len(got), st, "ms", eng.shor_last_stats()["ms"])
            assert len(got) == nm and got == want, (name, nm)
            assert not set(t for _, t in got) & set(existing)
            assert st["peak_bytes"] <= max(64 * 1024, 16 * (len(got) + SEL_CAP + largest)), (name, nm, st, largest)
            if name == "zero":
                assert st["compactions"] > st["tiles"] / 2, (nm, st)
    eng.close()


def test_stream_overflow_path(have_gpu, omc):
    """Scores that grow along the enumeration (X[t, i, j] = (t + 1) (i m + j): score ~ (i2 - i1)(j2 - j1), and a second X whose score grows
    with the first row index): tiles sized by the survival rate of their predecessor overflow the buffer, which is at its floor."""
    n, m, k = 60, 80, 2
    A, mask, eng = _shor_instance(omc, n, m, k, 0.4, 21)
    cl = [4, 3, 2, 1, 0]
    i = np.arange(n)[:, None]; j = np.arange(m)[None, :]
    ramp = np.stack([(t + 1.0) * (i * m + j) for t in range(k)])
    rows = np.stack([(t + 1.0) * np.exp2(i / 4.0) * (1.0 + ((i + j) % 2)) for t in range(k)])      # |x11 x22 - x12 x21| is 0 or ~ 2^((i1 + i2) / 4)
    for name, X3 in (("ramp", ramp), ("rows", rows)):
        for nm in (1, 100, 5000):
            want, got, st = _stream_vs_materialised(eng, X3, cl, [], nm, 1)
            print(name, nm, st, "ms", eng.shor_last_stats()["ms"])
            assert len(got) == nm and got == want, (name, nm)
            assert st["peak_bytes"] == 16 * (nm + SEL_CAP + _largest_pair_count(mask)), st      # the floor
    eng.close()


def test_stream_config5_size_default_classes(have_gpu, omc):
    """BASELINE config 5 shape (1000 x 1000, k = 2, 30 % observed) with the reference's default class list (1, 2, 3, 4): ~1.9e11 candidates,
    whose keys (~3 TB) no device holds.  The default budget streams them through 1 GiB.  Checked by properties, as
    test_violated_shor_minors_config5_size does for class 4 alone."""
    A, mask, gamma, c = omc.pkg.data.config_instance(5, seed=0)
    n, m = mask.shape; k = c["k"]
    eng = omc.Engine(A, mask, gamma, k)
    rng = np.random.default_rng(1)
    L = rng.standard_normal((k, n, 1)); R = rng.standard_normal((k, 1, m))
    X3 = L * R + 0.05 * rng.standard_normal((k, n, m))
    cl = [1, 2, 3, 4]
    top = eng.generate_violated_Shor_minors(X3, cl, [], 100)
    st = eng.shor_last_stats(); sel = eng.shor_last_select_stats()
    print("config 5, classes", cl, st, sel)
    assert len(top) == 100
    def score(i1, i2, j1, j2):
        s = 0.0
        for t in range(k):
            s += abs(X3[t, i1, j1] * X3[t, i2, j2] - X3[t, i1, j2] * X3[t, i2, j1])
        return s
    sc = [s for s, _ in top]
    keys = [(s, t) for s, t in top]
    assert keys == sorted(keys, reverse=True) and len(set(keys)) == 100                  # strictly decreasing (score, tuple)
    for s, (i1, i2, j1, j2) in top:
        assert 1 <= i1 < i2 <= n and 1 <= j1 < j2 <= m
        assert int(mask[i1 - 1, j1 - 1]) + int(mask[i1 - 1, j2 - 1]) + int(mask[i2 - 1, j1 - 1]) + int(mask[i2 - 1, j2 - 1]) in cl
        assert s == score(i1 - 1, i2 - 1, j1 - 1, j2 - 1)                                  # identical doubles
    # random candidates of the requested classes: none beats the 100th score
    i1 = rng.integers(0, n, 4_000_000); i2 = rng.integers(0, n, 4_000_000); j1 = rng.integers(0, m, 4_000_000); j2 = rng.integers(0, m, 4_000_000)
    ok = (i1 < i2) & (j1 < j2)
    i1, i2, j1, j2 = i1[ok], i2[ok], j1[ok], j2[ok]
    pc = mask[i1, j1].astype(int) + mask[i1, j2] + mask[i2, j1] + mask[i2, j2]
    ok = np.isin(pc, cl)
    i1, i2, j1, j2 = i1[ok], i2[ok], j1[ok], j2[ok]
    s = np.zeros(len(i1))
    for t in range(k):
        s += np.abs(X3[t, i1, j1] * X3[t, i2, j2] - X3[t, i1, j2] * X3[t, i2, j1])
    assert len(s) > 100_000
    assert s.max() <= sc[-1] or s.max() in sc
    want = _class_counts(mask)
    assert st["candidates"] == sum(want[p] for p in cl)
    assert sel["streamed"] == 1 and sel["tiles"] > 1
    assert sel["peak_bytes"] <= 1 << 30
    eng.close()
