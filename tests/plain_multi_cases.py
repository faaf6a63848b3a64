"""The inputs of tests/test_plain_multi.py, shared with tools/record_plain_multi_error_units.py and tests/test_plain_multi_cpu.py: the
builders, families, keys and seeds are those of oracle/omc_plain_ref.py, at the orders at which the multi-workgroup form of the plain
operations (omc_launch_cone_plain_mw) can go wrong.  No test in this file."""
import omc_plain_ref as R

# 145: the smallest order of the path, NP = Ncp = 160 (15 zero rows and columns inside a real block); 160: no padding, nb = 10;
# 161: NP = 176, Ncp = 192 (31 padding columns); 176: a whole block of zero columns paired with real ones; 257: more than 256 rows
SMALL_ORDERS = [145, 160, 161, 176, 257]
BIG_ORDER = 1040      # what the default OMC_PLAIN_MULTI_MIN serves, nb = 66
BIG_SEP_FAMILIES = ["a", "d", "b_out", "b_in", "c_two"]
BIG_ROUND_FAMILIES = ["top", "projector"]
BIG_ROUND_K = 2
ROUND_K8_ORDERS = [145, 176]
SVD_SHAPES = [(145, 147), (161, 200), (176, 176), (257, 260)]
SVD_K = 2


def sep_cases(N):
    return [c for c in R.sep_cases(N) if N != BIG_ORDER or c[1] in BIG_SEP_FAMILIES]


def round_ranks(N):
    if N == BIG_ORDER:
        return [BIG_ROUND_K]
    return [1, 2] + ([8] if N in ROUND_K8_ORDERS else [])


def round_cases(N, k):
    return [c for c in R.round_cases(N, k) if N != BIG_ORDER or c[1] in BIG_ROUND_FAMILIES]


def svd_cases(n, m):
    return R.svd_cases(n, m, SVD_K)


def all_inputs(orders=None):
    """[(key, seed, order, M builder, long-double M builder)] of every input with a reference (the zero matrices have none)."""
    out = []
    for N in (SMALL_ORDERS + [BIG_ORDER]) if orders is None else orders:
        for key, fam, seed in sep_cases(N):
            if fam != "e":
                out.append((key, seed, N, lambda fam=fam, N=N, seed=seed: _sep(fam, N, seed)))
        for k in round_ranks(N):
            for key, fam, seed in round_cases(N, k):
                if fam != "zero":
                    out.append((key, seed, N, lambda fam=fam, N=N, k=k, seed=seed: _round(fam, N, k, seed)))
    for n, m in SVD_SHAPES:
        if orders is not None and n not in orders:
            continue
        for key, fam, seed in svd_cases(n, m):
            if fam != "zero":
                out.append((key, seed, n, lambda fam=fam, n=n, m=m, seed=seed: _svd(fam, n, m, seed)))
    return out


def _sep(fam, N, seed):
    Y, U = R.sep_input(fam, N, R.SEP_K, seed)
    return R.sep_matrix(Y, U), R.sep_matrix_ld(Y, U)


def _round(fam, N, k, seed):
    Y = R.round_input(fam, N, k, seed)
    return R.sym(Y), R.sym_ld(Y)


def _svd(fam, n, m, seed):
    X = R.svd_input(fam, n, m, SVD_K, seed)
    return X @ X.T, R.gram_ld(X)
