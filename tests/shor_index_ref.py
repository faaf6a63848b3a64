"""An independent numpy restatement of the index structure of one Shor list (the arrays of ShorGroupDev), for
tests/test_shor_index_cpu.py and tests/test_gpu_shor_index.py.  It shares no code with the host builder (build_shor_group, omc_api_shor.cpp) or
the device builder (omc_shor_index.hip): np.lexsort on (member, key) for the three sorted structures, bincount / cumsum for the
coordinate CSR, a plain column walk for ctype / slackrow.  Also the lists the two test files share."""
import numpy as np

ARRAYS = ("mi", "kid", "cptr", "cent", "v1ptr", "v1ent", "v2ptr", "v2ent", "slackrow", "eclass", "ctype")
COUNTS = ("nq", "nv1", "nv2")
MSG_RANGE = "Shor minors must satisfy 1 <= i1 < i2 <= n, 1 <= j1 < j2 <= m (OMC.jl:2556-2603)"
MSG_DUP = "duplicate Shor minor in a node's list"
MSG_SOC = "SOC coordinate out of range"


def _grouped(key, nq):
    """key: (2, nq) keys of the members 2 q + which.  -> ids (2, nq), ptr, ent, number of keys"""
    member = np.arange(2 * nq, dtype=np.int64)
    flat = key.T.reshape(-1)                                   # member order: (q, which)
    order = np.lexsort((member, flat))
    sk = flat[order]
    head = np.ones(2 * nq, bool)
    head[1:] = sk[1:] != sk[:-1]
    ids_sorted = np.cumsum(head) - 1
    ids = np.empty(2 * nq, np.int64)
    ids[order] = ids_sorted
    ptr = np.concatenate([np.flatnonzero(head), [2 * nq]])
    return ids.reshape(nq, 2).T, ptr.astype(np.int32), member[order].astype(np.int32), int(head.sum())


def build(n, m, mask, shor_idx, soc_idx=None):
    """mask: (n, m) bool; shor_idx: (nq, 4) 1-based; soc_idx: None (every entry) or (n_soc, 2) 1-based.  Raises ValueError with the library's
    message, in the library's precedence (range, duplicate, SOC range)."""
    q = np.asarray(shor_idx, np.int64).reshape(-1, 4) - 1
    nq = len(q)
    i1, i2, j1, j2 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    if not ((0 <= i1) & (i1 < i2) & (i2 < n) & (0 <= j1) & (j1 < j2) & (j2 < m)).all():
        raise ValueError(MSG_RANGE)
    if len(set(map(tuple, q.tolist()))) != nq:
        raise ValueError(MSG_DUP)
    o = dict(nq=nq)
    o["mi"] = q.T.astype(np.int32).reshape(4, nq)
    k1, o["v1ptr"], o["v1ent"], o["nv1"] = _grouped(np.stack([(i1 * m + j1) * m + j2, (i2 * m + j1) * m + j2]), nq)
    k2, o["v2ptr"], o["v2ent"], o["nv2"] = _grouped(np.stack([(i1 * n + i2) * m + j1, (i1 * n + i2) * m + j2]), nq)
    o["kid"] = np.concatenate([k1, k2]).astype(np.int32).reshape(4, nq)
    # coordinates in block order (i1,j1), (i1,j2), (i2,j1), (i2,j2); member 4 q + p
    ci = np.stack([i1, i1, i2, i2], 1).reshape(-1); cj = np.stack([j1, j2, j1, j2], 1).reshape(-1)
    cid = cj * n + ci
    member = np.arange(4 * nq, dtype=np.int64)
    o["cent"] = member[np.lexsort((member, cid))].astype(np.int32)
    cnt = np.bincount(cid, minlength=n * m)
    o["cptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    ec = np.zeros(n * m, np.uint8)
    if soc_idx is None:
        ec[:] = 1
    else:
        s = np.asarray(soc_idx, np.int64).reshape(-1, 2) - 1
        if len(s) and not ((0 <= s[:, 0]) & (s[:, 0] < n) & (0 <= s[:, 1]) & (s[:, 1] < m)).all():
            raise ValueError(MSG_SOC)
        ec[s[:, 1] * n + s[:, 0]] = 1
    ec[cnt > 0] = 2
    o["eclass"] = ec
    ctype = np.full(m, 2, np.uint8); slack = np.full(m, -1, np.int32)
    obs = np.asarray(mask, bool)
    for j in range(m):
        rows = [i for i in range(n) if ec[j * n + i] != 2]
        unobs = [i for i in rows if not obs[i, j]]
        if unobs:
            ctype[j], slack[j] = 0, unobs[0]
        elif rows:
            ctype[j], slack[j] = 1, rows[0]
    o["ctype"] = ctype; o["slackrow"] = slack
    return o


def same(a, b):
    """every array and count of two structures, by name: the names that differ"""
    bad = [key for key in COUNTS if a[key] != b[key]]
    for key in ARRAYS:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y):
            bad.append(key)
    return bad


# ---- the lists of the tests ----------------------------------------------------------------------------------------------------------------
INSTANCES = {"10x12": (10, 12, 60, 2, 208), "12x14": (12, 14, 120, 3, 1615), "14x18": (14, 18, 150, 5, 1765)}


def instance(orc, name):
    """(A, mask, class-4 minor list as an (nq, 4) int64 array) of a named instance; "6x7" is fully observed"""
    import omc_oracle_shor as sh
    if name == "6x7":
        rng = np.random.default_rng(7)
        u, v = rng.standard_normal((6, 1)), rng.standard_normal((1, 7))
        A, mask, count = u @ v, np.ones((6, 7), bool), 315
    else:
        n, m, nobs, seed, count = INSTANCES[name]
        A, mask = orc.make_instance(n, m, 1, n_indices=nobs, seed=seed, noise=0.1)
    minors, _ = sh.driver_shor_lists(mask, (4,))
    minors = np.asarray(minors, np.int64).reshape(-1, 4)
    assert len(minors) == count, (name, len(minors))
    return A, mask, minors


def variants(minors, seed=0):
    """forward, reversed, permuted, first minor only, empty"""
    rng = np.random.default_rng(seed)
    return {"forward": minors, "reversed": minors[::-1].copy(), "permuted": minors[rng.permutation(len(minors))], "one": minors[:1].copy(),
            "empty": minors[:0].copy()}
