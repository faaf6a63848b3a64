"""Host-side mirror of the reference's per-node interface (same names, argument meaning and error behaviour),
backed by the HIP library.  Reference = /root/reference/src/OptimalMatrixCompletion.jl (OMC.jl).

    Engine(A, indices, gamma, k)                  uploads (A, indices, gamma) once       (OMC.jl:470-471)
    .matrix_completion_SDP_relaxation(nodes, ...) OMC.jl:1431-1943, a batch of nodes; with `shor_info` = one (constraints_indexes,
                                                  SOC_constraints_indexes) pair per node (BBNodeShorInfo, OMC.jl:37-40) the Shor-mode program
                                                  (add_Shor_valid_inequalities = true, rank 1)
    .reserve / .append / .fetch_done / .hold      nodes pushed into a staged or running batch as their parents finish (the queue of OMC.jl:700-719);
    .reserve_shor / .append_shor / .fetch_done_shor   the same for a Shor-mode batch (rank 1)
    .branch_plan / .append_children / .fetch_descriptor   the children of finished nodes by reference: their descriptors are built on the device
    .keep_certificates / .fetch_certificate       the multipliers behind a node's dual_bound, for certificate.py (numpy) or .dual_bound (device) to re-evaluate
    .keep_shor_certificates / .fetch_shor_certificate   the same for Shor-mode nodes (rank 1), for certificate.shor_dual_bound (numpy)
    .matrix_completion_master_feasible(Y, U)      OMC.jl:1261-1277
    .breakpoint_vectors(Y, U, breakpoints)        OMC.jl:2466-2477
    .evaluate_objective(X)                        OMC.jl:2330-2359
    .alternating_minimization(U_initial, ...)     OMC.jl:1979-2279
A node is the reference's BBNode reduced to what the relaxation reads: a list of cuts
(breakpoint_vec, U_hat, directions) exactly as BBNodeDisjunctiveCuts.cuts holds them (OMC.jl:33-35).
"""
from __future__ import annotations

import atexit
import weakref
import ctypes as C

import numpy as np

from . import _lib, certificate
from ._lib import RelaxParams, OmcError

CUT_TYPES = {"linear": 0, "linear2": 1, "linear3": 2}
DIR_CODES = {"left": 0, "middle": 1, "right": 2, "inner_left": 3, "inner_right": 4}
DIR_NAMES = {v: k_ for k_, v in DIR_CODES.items()}
BREAKPOINTS = {"smallest_1_eigvec": 1, "smallest_2_eigvec": 2}
STATUS_NAMES = {0: "OPTIMAL", 1: "SLOW_PROGRESS", 2: "TIME_LIMIT", 3: "INFEASIBLE", 4: "OBJECTIVE_LIMIT"}      # 4: dual_bound > the cutoff of set_cutoff
KERNEL_CLASSES = ["colprox", "cone", "global", "check", "setup", "small", "accel", "cone_sub", "check_col", "check_build", "harvest",
                  "shor_bigcone", "shor_minors", "shor_cols"]
# omc_last_host_phases, in the order of OMC_HOST_* (include/omc.h)
HOST_PHASES = ["check_wait", "check_scan", "list", "event_drain", "harvest_flags", "harvest_enqueue", "harvest_wait", "harvest_book",
               "setup_enqueue", "check_total", "harvest_total", "async_harvests", "quiet_intervals", "body_records", "body_waits"]      # the last four are counts only
HOST_BODY_COUNTS = ("body_records", "body_waits")      # counts of the iterations themselves: Engine.event_counts(), not host_phases()
# order of omc_kernel_residency's output (OMC_RES_* in include/omc.h)
RESIDENCY_KERNELS = ["k_cone_sub<0>", "k_cone_sub<1>", "k_cone_sub<2>", "k_global", "k_small", "k_colprox_pair", "k_colprox_wide", "k_colprox",
                     "k_cone_ws", "k_cone"]


def default_params(**kw) -> RelaxParams:
    p = RelaxParams()
    _lib.load().omc_relax_params_default(C.byref(p))
    for k_, v in kw.items():
        if not hasattr(p, k_):
            raise TypeError(f"unknown relaxation parameter {k_!r}")
        setattr(p, k_, v)
    return p


def _pack_cuts(nodes, n, k, cut_type):
    if cut_type not in CUT_TYPES:
        raise ValueError("Invalid input for disjunctive cuts type.\nDisjunctive cuts type must be either "
                         f"\"linear\" or \"linear2\" or \"linear3\";\n{cut_type} supplied instead.")   # OMC.jl:1456-1462
    L = np.array([len(c) for c in nodes], dtype=np.int32)
    tot = int(L.sum())
    cx = np.zeros((max(tot, 1), n)); cU = np.zeros((max(tot, 1), n * k)); cd = np.zeros((max(tot, 1), k), dtype=np.int8)
    t = 0
    for cuts in nodes:
        for (x, Uh, dirs) in cuts:
            x = np.asarray(x, float); Uh = np.asarray(Uh, float).reshape(n, k)
            if x.shape != (n,) or len(dirs) != k:
                raise ValueError("Dimension mismatch in cut (OMC.jl:34)")
            cx[t] = x; cU[t] = Uh.ravel(order="F")
            for j, d in enumerate(dirs):
                cd[t, j] = DIR_CODES[d] if isinstance(d, str) else int(d)
            t += 1
    return L, cx, cU, cd


def _pack_shor(shor_info):
    """Wire format of omc_relax_stage_shor / omc_relax_append_shor: (n_shor, shor_idx, n_soc, soc_idx) of one (constraints_indexes,
    SOC_constraints_indexes) pair per node; SOC_constraints_indexes = None is sent as n_soc = -1."""
    B = len(shor_info)
    nsh = np.zeros(B, np.int64); nso = np.zeros(B, np.int64); sh_parts = []; so_parts = []
    for b, (minors, soc) in enumerate(shor_info):
        mq = np.asarray(minors, np.int64).reshape(-1, 4)
        nsh[b] = len(mq); sh_parts.append(mq)
        if soc is None:
            nso[b] = -1
        else:
            sq = np.asarray(soc, np.int64).reshape(-1, 2)
            nso[b] = len(sq); so_parts.append(sq)
    shi = np.ascontiguousarray(np.concatenate(sh_parts)) if sh_parts and sum(len(a) for a in sh_parts) else np.zeros((1, 4), np.int64)
    soi = np.ascontiguousarray(np.concatenate(so_parts)) if so_parts and sum(len(a) for a in so_parts) else np.zeros((1, 2), np.int64)
    return nsh, nso, shi, soi


def shor_rank_k_extension(k, X, W, minors):
    """The lifted variables of the reference's rank k > 1 Shor form (Xt, Wt, H, V1, V2, V3: OMC.jl:1526-1551, results at 1909-1917) as an explicit
    extension of the relaxation's (X, W).  Reference quirk Q5: in that form the slack s that H cancels in W = sum Wt + 2 sum H makes every
    per-layer order-5 block satisfiable, so the minors do not constrain (X, W) and the engine solves the program without them; this is the closed form
        Xt_1 = X, Xt_t = 0;  Wt_1 = X^2 + (W - X^2) + s, Wt_t = s/(k-1);  H_(1,t) = -s/(k-1), H_(t,t') = 0;  V^1 = products of X (V3: their mean), V^t = 0,
        s_c = max over the minors that contain c of |X_{i1j2} X_{i2j1} - X_{i1j1} X_{i2j2}| / 2.
    Returns Xt (k, n, m), Wt (k, n, m), H (k, k, n, m) and V (k, nq, 5) with the five products of each minor in the order of omc_relax_fetch_shor_V."""
    X = np.asarray(X, float); W = np.asarray(W, float); n, m = X.shape
    mi = np.asarray(minors, np.int64).reshape(-1, 4) - 1
    nq = len(mi)
    Xt = np.zeros((k, n, m)); Xt[0] = X
    Wt = np.zeros((k, n, m)); H = np.zeros((k, k, n, m)); V = np.zeros((k, nq, 5))
    if nq == 0:
        return dict(Xt=Xt, Wt=Wt, H=H, V=V)
    ci = np.stack([mi[:, 0], mi[:, 0], mi[:, 1], mi[:, 1]], 1); cj = np.stack([mi[:, 2], mi[:, 3], mi[:, 2], mi[:, 3]], 1)
    xs = X[ci, cj]
    e = 0.5 * np.abs(xs[:, 1] * xs[:, 2] - xs[:, 0] * xs[:, 3])
    s = np.zeros((n, m)); inC = np.zeros((n, m), bool)
    for p_ in range(4):
        np.maximum.at(s, (ci[:, p_], cj[:, p_]), e); inC[ci[:, p_], cj[:, p_]] = True
    s = np.where(inC, s * (1.0 + 1e-12) + 1e-300, 0.0)
    b = s / (k - 1)
    Wt[0] = np.where(inC, X * X + np.maximum(W - X * X, 0.0) + s, 0.0)
    for t in range(1, k):
        Wt[t] = np.where(inC, b, 0.0); H[0, t] = np.where(inC, -b, 0.0)
    V[0, :, 0] = xs[:, 0] * xs[:, 1]; V[0, :, 1] = xs[:, 2] * xs[:, 3]; V[0, :, 2] = xs[:, 0] * xs[:, 2]; V[0, :, 3] = xs[:, 1] * xs[:, 3]
    V[0, :, 4] = 0.5 * (xs[:, 0] * xs[:, 3] + xs[:, 1] * xs[:, 2])
    return dict(Xt=Xt, Wt=Wt, H=H, V=V)


_LIVE = weakref.WeakSet()      # engines still holding a device instance: closed before the interpreter (and then the HIP runtime) goes down


def _close_all():
    for e in list(_LIVE):
        try:
            e.close()
        except Exception:
            pass


atexit.register(_close_all)


def branch_plan(cut_type, k):
    """omc_branch_plan (host only, no GPU): the direction tuples of one node's children in the order of bnb.child_directions."""
    if cut_type not in CUT_TYPES:
        raise ValueError(f"Invalid input for disjunctive cuts type: {cut_type}")
    lib = _lib.load()
    if not hasattr(lib, "omc_branch_plan"):
        raise OmcError(-100, "this build of the library has no omc_branch_plan")
    cap = 4 ** int(k)
    d = np.zeros((cap, int(k)), np.int8); cnt = np.zeros(1, np.int32)
    _lib.check(lib.omc_branch_plan(CUT_TYPES[cut_type], int(k), cap, _lib.ptr(d), _lib.ptr(cnt)))
    return [tuple(DIR_NAMES[int(c)] for c in row) for row in d[:int(cnt[0])]]


def colprox_plan(n, cmax, block_min=65):
    """omc_colprox_plan (host only, no GPU): where k_colprox_block keeps a column of cmax observed rows."""
    out = np.zeros(5, np.int64)
    _lib.check(_lib.load().omc_colprox_plan(int(n), int(cmax), int(block_min), _lib.ptr(out)))
    return dict(lds_cmax=int(out[0]), lds_bytes=int(out[1]), slab_doubles=int(out[2]), workgroups_per_cu=int(out[3]), block=bool(out[4]))


def plain_multi_plan(n, plain_multi_min=1025):
    """omc_plain_multi_plan (host only, no GPU): whether separation, rounding and the left singular vectors at order n take the
    multi-workgroup eigen-kernels under OMC_PLAIN_MULTI_MIN = plain_multi_min, and their layout there."""
    out = np.zeros(6, np.int64)
    _lib.check(_lib.load().omc_plain_multi_plan(int(n), int(plain_multi_min), _lib.ptr(out)))
    return dict(multi=bool(out[0]), NP=int(out[1]), Ncp=int(out[2]), nb=int(out[3]), slab_bytes=int(out[4]), launches=int(out[5]))


def plain_multi_tau():
    """omc_plain_multi_tau: rotation threshold and stop rule of that path."""
    return float(_lib.load().omc_plain_multi_tau())


def certificate_plan(n, k, nnz, max_cuts=0, nonstandard_box_rows=0):
    """omc_certificate_plan (host only, no GPU): strides of a certificate in doubles, bytes the arena holds per node, rmax."""
    out = np.zeros(6, np.int64)
    _lib.check(_lib.load().omc_certificate_plan(int(n), int(k), int(nnz), int(max_cuts), int(nonstandard_box_rows), _lib.ptr(out)))
    return dict(Lam=int(out[0]), lam=int(out[1]), Q=int(out[2]), Psi3=int(out[3]), bytes_per_node=int(out[4]), rmax=int(out[5]))


def shor_certificate_plan(n, m, k, nq_stride, max_cuts=0, nonstandard_box_rows=0):
    """omc_shor_certificate_plan (host only, no GPU): strides of a Shor-mode certificate in doubles, bytes per node of the arena and per slot, rmax."""
    out = np.zeros(10, np.int64)
    _lib.check(_lib.load().omc_shor_certificate_plan(int(n), int(m), int(k), int(nq_stride), int(max_cuts), int(nonstandard_box_rows), _lib.ptr(out)))
    keys = ("lam", "Q", "Psi3", "Gam", "zeta", "xi", "Xbar", "bytes_per_node", "bytes_per_slot", "rmax")
    return {key: int(v) for key, v in zip(keys, out)}


def shor_dual_bound_plan(n, m, k, B, nq_stride, max_cuts=0, nonstandard_box_rows=0, sanitise=True):
    """omc_shor_dual_bound_plan (host only, no GPU): device bytes Engine.shor_dual_bound needs -- per node, in total, the node and view parts,
    views per node, doubles of the eigen-kernel's slab, Rmax, rmax."""
    out = np.zeros(8, np.int64)
    _lib.check(_lib.load().omc_shor_dual_bound_plan(int(n), int(m), int(k), int(B), int(nq_stride), int(max_cuts), int(nonstandard_box_rows),
                                                    1 if sanitise else 0, _lib.ptr(out)))
    keys = ("bytes_per_node", "bytes_total", "node_bytes", "view_bytes", "ways", "slab_doubles", "Rmax", "rmax")
    return {key: int(v) for key, v in zip(keys, out)}


def shor_index_plan(n, m, nq):
    """omc_shor_index_plan (host only, no GPU): what the shape fixes for the device builder of a Shor list's index structure -- radix passes of
    its four sorts, bytes of sort scratch, ints and bytes of one built list in the staging room, kernels per list, items per workgroup and pass."""
    out = np.zeros(9, np.int64)
    _lib.check(_lib.load().omc_shor_index_plan(int(n), int(m), int(nq), _lib.ptr(out)))
    keys = ("passes_v1", "passes_v2", "passes_coord", "passes_dup", "scratch_bytes", "stage_ints", "stage_bytes", "launches", "tile")
    return {key: int(v) for key, v in zip(keys, out)}


class Engine:
    """Device-resident instance + the four call sites of the reference driver."""

    def __init__(self, A, indices, gamma, k, device=0):
        A = np.asarray(A, dtype=np.float64); indices = np.asarray(indices)
        if A.ndim != 2 or A.shape != indices.shape:
            raise ValueError("Dimension mismatch.\nInput matrix A must have size (n, m);\nInput matrix indices must have size (n, m).")
        self.n, self.m = A.shape
        self.k = int(k); self.gamma = float(gamma); self.device = int(device)
        self.A = np.asfortranarray(A); self.indices = indices.astype(bool)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        mask = np.asfortranarray(self.indices.astype(np.uint8))
        _lib.check(self._lib.omc_instance_create(self.n, self.m, self.k, _lib.ptr(self.A), _lib.ptr(mask), self.gamma,
                                                 int(device), C.byref(self._h)))
        _LIVE.add(self)

    def close(self):
        _LIVE.discard(self)
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.omc_instance_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tuning knobs ----------------------------------------------------------------------------------
    def tuning_set(self, name, value=None):
        """Set (or, with None, remove) one tuning knob of this instance (omc_tuning_set); the library reads the environment only at creation."""
        _lib.check(self._lib.omc_tuning_set(self._h, name.encode(), None if value is None else str(value).encode()))

    def tuning_reload_env(self):
        """Read the OMC_* knobs from the environment again (omc_tuning_reload_env)."""
        _lib.check(self._lib.omc_tuning_reload_env(self._h))

    # ---- relaxation ------------------------------------------------------------------------------------
    def state_pool_create(self, capacity):
        """Reserve `capacity` final states on the device for warm starts (omc_state_pool_create)."""
        _lib.check(self._lib.omc_state_pool_create(self._h, int(capacity)))
        self.pool_capacity = int(capacity)

    def state_pool_reserve_shor(self, nq_max):
        """Extend every pool entry by the Shor state of a node with at most nq_max minors (omc_state_pool_reserve_shor; after
        state_pool_create).  From then on stage_shor honours load_from / save_to."""
        _lib.check(self._lib.omc_state_pool_reserve_shor(self._h, int(nq_max)))
        self.pool_shor_nq_max = int(nq_max)

    @staticmethod
    def shor_state_bytes(n, m, nq_max):
        """Bytes the Shor extension adds to one pool entry (the formula of include/omc.h)."""
        return 8 * (3 * n * m + m * m + (n + m) ** 2 + 2 * m + 20 * int(nq_max)) + 32

    def shor_warm_stats(self):
        """Warm-start accounting of the last staged Shor batch (omc_last_shor_warm_stats)."""
        o = np.zeros(4, np.int64)
        _lib.check(self._lib.omc_last_shor_warm_stats(self._h, _lib.ptr(o)))
        return dict(loaded_identical=int(o[0]), loaded_prefix=int(o[1]), refused=int(o[2]), saved=int(o[3]))

    def state_pool_fetch_shor(self, entry):
        """The point a Shor-mode pool entry holds, unscaled (omc_state_pool_fetch_shor): dict(nq, X (n, m), Theta (m, m), V (nq, 5))."""
        n, m = self.n, self.m
        nq = np.zeros(1, np.int64)
        _lib.check(self._lib.omc_state_pool_fetch_shor(self._h, int(entry), _lib.ptr(nq), None, None, None))
        X = np.zeros(n * m); Th = np.zeros(m * m); V = np.zeros((max(int(nq[0]), 1), 5))
        _lib.check(self._lib.omc_state_pool_fetch_shor(self._h, int(entry), _lib.ptr(nq), _lib.ptr(X), _lib.ptr(Th), _lib.ptr(V)))
        return dict(nq=int(nq[0]), X=X.reshape((n, m), order="F"), Theta=Th.reshape((m, m), order="F"), V=V[:int(nq[0])])

    def _set_warm(self, B, load_from, save_to):
        if load_from is None and save_to is None:
            return
        lf = None if load_from is None else np.ascontiguousarray(np.asarray(load_from, dtype=np.int32))
        sv = None if save_to is None else np.ascontiguousarray(np.asarray(save_to, dtype=np.int32))
        if (lf is not None and lf.shape != (B,)) or (sv is not None and sv.shape != (B,)):
            raise ValueError("load_from / save_to must hold one pool index per node")
        _lib.check(self._lib.omc_relax_set_warm(self._h, B, _lib.ptr(lf), _lib.ptr(sv)))

    def stage(self, nodes, disjunctive_cuts_type="linear", params=None, U_lower=None, U_upper=None, rho_scales=None, load_from=None, save_to=None):
        n, k = self.n, self.k
        self._set_warm(len(nodes), load_from, save_to)
        if rho_scales is not None:
            rs = np.ascontiguousarray(np.asarray(rho_scales, dtype=np.float64))
            if rs.shape != (len(nodes),):
                raise ValueError("rho_scales must hold one value per node")
            _lib.check(self._lib.omc_set_node_rho_scales(self._h, len(nodes), _lib.ptr(rs)))
        L, cx, cU, cd = _pack_cuts(nodes, n, k, disjunctive_cuts_type)
        p = params or default_params()
        B = len(nodes)
        lo = hi = None
        if U_lower is not None:
            lo = np.ascontiguousarray(np.stack([np.asfortranarray(u).ravel(order="F") for u in U_lower]))
        if U_upper is not None:
            hi = np.ascontiguousarray(np.stack([np.asfortranarray(u).ravel(order="F") for u in U_upper]))
        self._keep = (L, cx, cU, cd, lo, hi, p)
        _lib.check(self._lib.omc_relax_stage(self._h, B, C.byref(p), CUT_TYPES[disjunctive_cuts_type], _lib.ptr(L), _lib.ptr(cx),
                                             _lib.ptr(cU), _lib.ptr(cd), _lib.ptr(lo), _lib.ptr(hi)))
        self._B = B
        # what fetch_descriptor and append_children need of this batch: its cut type and the cut stride (include/omc.h: Lmax); reserve() is consumed
        extra_nodes, max_cuts = getattr(self, "_reserved", (0, 0)); self._reserved = (0, 0)
        self._cut_type = disjunctive_cuts_type
        self._Lmax = max(1, int(L.max()) if len(L) else 0, max_cuts if extra_nodes > 0 else 0)

    def stage_shor(self, nodes, shor_info, disjunctive_cuts_type="linear", params=None, U_lower=None, U_upper=None, penalties=None, keep_V=False,
                   load_from=None, save_to=None):
        """Stage a batch with add_Shor_valid_inequalities = true (OMC.jl:747-754 with node.Shor_info).  shor_info[b] =
        (constraints_indexes, SOC_constraints_indexes): 1-based (i1, i2, j1, j2) tuples and 1-based (i, j) pairs as the reference
        holds them (OMC.jl:37-40); SOC_constraints_indexes = None means "every coordinate outside the minors" (what the reference's
        driver always builds, OMC.jl:656-673, 2508-2517).  load_from / save_to: pool entries as in stage(); honoured once
        state_pool_reserve_shor has been called (rank 1), ignored otherwise; shor_warm_stats() tells what the library did with them."""
        n, k = self.n, self.k
        if len(shor_info) != len(nodes):
            raise ValueError("one Shor_info per node")
        self._set_warm(len(nodes), load_from, save_to)
        _lib.check(self._lib.omc_set_shor_keep_V(self._h, 1 if keep_V else 0))
        self._nqmax = max([len(np.asarray(mi).reshape(-1, 4)) for (mi, _) in shor_info] + [1, getattr(self, "_reserved_nq", 0)])      # reserve_shor: consumed below
        self._reserved_nq = 0
        if penalties is not None:
            _lib.check(self._lib.omc_set_shor_penalties(self._h, float(penalties[0]), float(penalties[1]), float(penalties[2])))
        L, cx, cU, cd = _pack_cuts(nodes, n, k, disjunctive_cuts_type)
        p = params or default_params()
        B = len(nodes)
        lo = hi = None
        if U_lower is not None:
            lo = np.ascontiguousarray(np.stack([np.asfortranarray(u).ravel(order="F") for u in U_lower]))
        if U_upper is not None:
            hi = np.ascontiguousarray(np.stack([np.asfortranarray(u).ravel(order="F") for u in U_upper]))
        nsh, nso, shi, soi = _pack_shor(shor_info)
        self._keep = (L, cx, cU, cd, lo, hi, p, nsh, nso, shi, soi)
        self._reserved = (0, 0); self._cut_type = disjunctive_cuts_type      # the reservation is consumed by this stage call
        _lib.check(self._lib.omc_relax_stage_shor(self._h, B, C.byref(p), CUT_TYPES[disjunctive_cuts_type], _lib.ptr(L), _lib.ptr(cx),
                                                  _lib.ptr(cU), _lib.ptr(cd), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(nsh), _lib.ptr(shi),
                                                  _lib.ptr(nso), _lib.ptr(soi)))
        self._B = B

    def fetch_shor(self):
        """W of the last Shor-mode batch (results["W"], OMC.jl:1908), one (n, m) matrix per node."""
        W = np.zeros((self._B, self.n * self.m))
        _lib.check(self._lib.omc_relax_fetch_shor(self._h, _lib.ptr(W)))
        return [W[b].reshape((self.n, self.m), order="F") for b in range(self._B)]

    def fetch_shor_V(self):
        """(nq_max, 5) per node: V1[i1,(j1,j2)], V1[i2,(j1,j2)], V2[(i1,i2),j1], V2[(i1,i2),j2], V3 of every minor (needs keep_V at staging)."""
        V = np.zeros((self._B, self._nqmax * 5))
        _lib.check(self._lib.omc_relax_fetch_shor_V(self._h, _lib.ptr(V)))
        return [V[b].reshape(self._nqmax, 5) for b in range(self._B)]

    def reserve(self, extra_nodes, max_cuts):
        """Room for nodes appended to the NEXT staged batch (omc_relax_reserve): extra_nodes more nodes with at most max_cuts cuts each."""
        _lib.check(self._lib.omc_relax_reserve(self._h, int(extra_nodes), int(max_cuts)))
        self._reserved = (int(extra_nodes), int(max_cuts))

    def append(self, nodes, disjunctive_cuts_type="linear", load_from=None, save_to=None):
        """Add nodes to the staged batch -- also while a submitted solve is running (omc_relax_append): the reference's queue keeps receiving
        the children of relaxed nodes (OMC.jl:700-719, 2520-2542).  Raises OmcError once that solve has ended.  fetch() returns the appended
        nodes behind the staged ones."""
        n, k = self.n, self.k
        L, cx, cU, cd = _pack_cuts(nodes, n, k, disjunctive_cuts_type)
        lf = None if load_from is None else np.ascontiguousarray(np.asarray(load_from, dtype=np.int32))
        sv = None if save_to is None else np.ascontiguousarray(np.asarray(save_to, dtype=np.int32))
        if (lf is not None and lf.shape != (len(nodes),)) or (sv is not None and sv.shape != (len(nodes),)):
            raise ValueError("load_from / save_to must hold one pool index per node")
        _lib.check(self._lib.omc_relax_append(self._h, len(nodes), _lib.ptr(L), _lib.ptr(cx), _lib.ptr(cU), _lib.ptr(cd), _lib.ptr(lf), _lib.ptr(sv)))
        self._B += len(nodes)

    def branch_plan(self, cut_type):
        """The direction tuples of one node's children, in the order of bnb.child_directions (omc_branch_plan; host only)."""
        return branch_plan(cut_type, self.k)

    def append_children(self, parent_ids, dirs=None, load_from=None, save_to=None):
        """Add children of finished nodes to the staged batch by reference (omc_relax_append_children): child c is node parent_ids[c] plus
        one cut (x = that node's breakpoint_vec, Uhat = its U, directions dirs[c]), its descriptor is built on the device.  With dirs = None
        every child of every parent, in branch_plan order.  The parents must have been returned by fetch_done().  Returns the children's
        node ids (consecutive, in the order given); load_from / save_to as in append().  Raises OmcError when the library refuses: the
        batch is then as it was."""
        if not hasattr(self._lib, "omc_relax_append_children"):
            raise OmcError(-100, "this build of the library has no omc_relax_append_children")
        k = self.k
        parents = [int(p) for p in parent_ids]
        if dirs is None:
            plan = self.branch_plan(self._cut_type)
            dirs = [d for _ in parents for d in plan]
            parents = [p for p in parents for _ in plan]
        if len(dirs) != len(parents) or any(len(d) != k for d in dirs):
            raise ValueError("dirs must hold one tuple of k directions per child")
        Cn = len(parents)
        pv = np.ascontiguousarray(np.asarray(parents, dtype=np.int32))
        dv = np.zeros((max(Cn, 1), k), np.int8)
        for c, d in enumerate(dirs):
            for j, x in enumerate(d):
                dv[c, j] = DIR_CODES[x] if isinstance(x, str) else int(x)
        lf = None if load_from is None else np.ascontiguousarray(np.asarray(load_from, dtype=np.int32))
        sv = None if save_to is None else np.ascontiguousarray(np.asarray(save_to, dtype=np.int32))
        if (lf is not None and lf.shape != (Cn,)) or (sv is not None and sv.shape != (Cn,)):
            raise ValueError("load_from / save_to must hold one pool index per child")
        first = np.zeros(1, np.int32)
        _lib.check(self._lib.omc_relax_append_children(self._h, Cn, _lib.ptr(pv), _lib.ptr(dv), _lib.ptr(lf), _lib.ptr(sv), _lib.ptr(first)))
        self._B += Cn
        return list(range(int(first[0]), int(first[0]) + Cn))

    def fetch_descriptor(self, node_id):
        """One node's staged descriptor as the kernels read it, whole strides with their padding (omc_relax_fetch_descriptor): dict(R, rkind,
        rcut, rbi, rbj (Rmax each), rcoef (Rmax, k), rrhs (Rmax), L, cutx (Lmax, n), r, Q (n, rmax) with the basis in its first r columns)."""
        if not hasattr(self._lib, "omc_relax_fetch_descriptor"):
            raise OmcError(-100, "this build of the library has no omc_relax_fetch_descriptor")
        n, k = self.n, self.k
        info = self.solver_info()
        Rmax, rmax, Lmax = max(info["R_max"], 1), max(info["r_max"], 1), self._Lmax
        R = np.zeros(1, np.int32); L = np.zeros(1, np.int32); r = np.zeros(1, np.int32)
        rkind = np.zeros(Rmax, np.int32); rcut = np.zeros(Rmax, np.int32); rbi = np.zeros(Rmax, np.int32); rbj = np.zeros(Rmax, np.int32)
        rcoef = np.zeros(Rmax * k); rrhs = np.zeros(Rmax); cutx = np.zeros(Lmax * n); Q = np.zeros(n * rmax)
        _lib.check(self._lib.omc_relax_fetch_descriptor(self._h, int(node_id), _lib.ptr(R), _lib.ptr(rkind), _lib.ptr(rcut), _lib.ptr(rbi), _lib.ptr(rbj),
                                                        _lib.ptr(rcoef), _lib.ptr(rrhs), _lib.ptr(L), _lib.ptr(cutx), _lib.ptr(r), _lib.ptr(Q)))
        return dict(R=int(R[0]), rkind=rkind, rcut=rcut, rbi=rbi, rbj=rbj, rcoef=rcoef.reshape(Rmax, k), rrhs=rrhs, L=int(L[0]),
                    cutx=cutx.reshape(Lmax, n), r=int(r[0]), Q=Q.reshape((n, rmax), order="F"))

    def reserve_shor(self, nq_max, extra_lists):
        """With reserve(): room in the NEXT stage_shor batch for appended nodes whose lists hold at most nq_max minors, extra_lists of them
        lists the batch does not know yet (omc_relax_reserve_shor).  A node that carries a list the batch knows needs no list room."""
        _lib.check(self._lib.omc_relax_reserve_shor(self._h, int(nq_max), int(extra_lists)))
        self._reserved_nq = int(nq_max)

    def append_shor(self, nodes, shor_info, disjunctive_cuts_type="linear", load_from=None, save_to=None):
        """Add Shor nodes to the staged Shor batch -- also while a submitted solve is running (omc_relax_append_shor).  shor_info as in
        stage_shor; load_from / save_to as in append().  Raises OmcError when the library refuses (solve ended, a capacity of reserve() /
        reserve_shor() used up, ...): the batch is then as it was."""
        n, k = self.n, self.k
        if len(shor_info) != len(nodes):
            raise ValueError("one Shor_info per node")
        L, cx, cU, cd = _pack_cuts(nodes, n, k, disjunctive_cuts_type)
        lf = None if load_from is None else np.ascontiguousarray(np.asarray(load_from, dtype=np.int32))
        sv = None if save_to is None else np.ascontiguousarray(np.asarray(save_to, dtype=np.int32))
        if (lf is not None and lf.shape != (len(nodes),)) or (sv is not None and sv.shape != (len(nodes),)):
            raise ValueError("load_from / save_to must hold one pool index per node")
        nsh, nso, shi, soi = _pack_shor(shor_info)
        _lib.check(self._lib.omc_relax_append_shor(self._h, len(nodes), _lib.ptr(L), _lib.ptr(cx), _lib.ptr(cU), _lib.ptr(cd), _lib.ptr(nsh),
                                                   _lib.ptr(shi), _lib.ptr(nso), _lib.ptr(soi), _lib.ptr(lf), _lib.ptr(sv)))
        self._B += len(nodes)

    def fetch_done_shor(self, ids, want_W=False, want_Theta=False):
        """X (and W, Theta on request) of nodes that fetch_done() has already returned, while the solve runs (omc_relax_fetch_done_shor):
        one dict per id, the matrices that fetch() / fetch_shor() give for the node after the solve."""
        n, m = self.n, self.m
        idv = np.ascontiguousarray(np.asarray(list(ids), dtype=np.int32))
        c = len(idv)
        X = np.zeros((max(c, 1), n * m)); W = np.zeros((max(c, 1), n * m)) if want_W else None; Th = np.zeros((max(c, 1), m * m)) if want_Theta else None
        _lib.check(self._lib.omc_relax_fetch_done_shor(self._h, c, _lib.ptr(idv), _lib.ptr(X), _lib.ptr(W), _lib.ptr(Th)))
        out = []
        for i in range(c):
            d = dict(node=int(idv[i]), X=X[i].reshape((n, m), order="F"))
            if want_W:
                d["W"] = W[i].reshape((n, m), order="F")
            if want_Theta:
                d["Theta"] = Th[i].reshape((m, m), order="F")
            out.append(d)
        return out

    def hold(self, on=True):
        """Keep the submitted solve open when it runs dry (omc_relax_hold): it waits for append() until hold(False)."""
        _lib.check(self._lib.omc_relax_hold(self._h, 1 if on else 0))

    # ---- objective cutoff ------------------------------------------------------------------------------
    def set_cutoff(self, value):
        """Objective cutoff of this engine (omc_relax_set_cutoff): a node whose rigorous dual_bound exceeds it at a certificate check ends there
        with status 4, "OBJECTIVE_LIMIT".  Holds for every batch until set again; inf (the default) is off.  May be called while a submitted
        solve runs: it takes effect at the first check that starts after the call returns."""
        if not hasattr(self._lib, "omc_relax_set_cutoff"):
            raise OmcError(-100, "this build of the library has no omc_relax_set_cutoff")
        _lib.check(self._lib.omc_relax_set_cutoff(self._h, float(value)))

    def get_cutoff(self):
        if not hasattr(self._lib, "omc_relax_get_cutoff"):
            raise OmcError(-100, "this build of the library has no omc_relax_get_cutoff")
        v = np.zeros(1)
        _lib.check(self._lib.omc_relax_get_cutoff(self._h, _lib.ptr(v)))
        return float(v[0])

    def cutoff_stats(self):
        """(nodes of the last or running solve that ended OBJECTIVE_LIMIT, the sum of their iterations, set_cutoff calls taken while it ran, 0)
        (omc_last_cutoff_stats)."""
        if not hasattr(self._lib, "omc_last_cutoff_stats"):
            raise OmcError(-100, "this build of the library has no omc_last_cutoff_stats")
        o = np.zeros(4, np.int64)
        _lib.check(self._lib.omc_last_cutoff_stats(self._h, _lib.ptr(o)))
        return tuple(int(x) for x in o)

    def fetch_done(self, max_nodes=4096, want_Y=False):
        """Results of the nodes finished since the last call (omc_relax_fetch_done), also while the submitted solve is running: a list of dicts
        with the keys of fetch() that a driver needs to branch (node = index among the staged + appended nodes; Y on request)."""
        n, k = self.n, self.k
        key = (int(max_nodes), bool(want_Y))
        if getattr(self, "_fd_key", None) != key:          # the receive buffers are kept between calls (a polling loop calls this every millisecond)
            self._fd_key = key
            self._fd = (np.zeros(max_nodes, np.int32), np.zeros(max_nodes), np.zeros(max_nodes), np.zeros(max_nodes, np.int32), np.zeros(max_nodes, np.int32),
                        np.zeros((max_nodes, n * k)), np.zeros((max_nodes, 2)), np.zeros((max_nodes, n)), np.zeros(1, np.int32),
                        np.zeros((max_nodes, n * n)) if want_Y else None)
        ids, obj, lb, st, it, U, ev, bx, cnt, Y = self._fd
        _lib.check(self._lib.omc_relax_fetch_done(self._h, int(max_nodes), _lib.ptr(ids), _lib.ptr(obj), _lib.ptr(lb), _lib.ptr(st), _lib.ptr(it),
                                                  _lib.ptr(U), _lib.ptr(ev), _lib.ptr(bx), _lib.ptr(Y), _lib.ptr(cnt)))
        out = []
        for i in range(int(cnt[0])):
            d = dict(node=int(ids[i]), objective=float(obj[i]), dual_bound=float(lb[i]), status_code=int(st[i]), termination_status=STATUS_NAMES[int(st[i])],
                     feasible=int(st[i]) != 3, iters=int(it[i]), U=U[i].reshape((n, k), order="F").copy(), lambda_min=ev[i].copy(), breakpoint_vec=bx[i].copy())
            if want_Y:
                d["Y"] = Y[i].reshape((n, n), order="F").copy()
            out.append(d)
        return out

    def solve(self):
        _lib.check(self._lib.omc_relax_solve(self._h))

    def submit(self):
        """Asynchronous solve of the staged batch: returns at once; poll() / wait() follow (omc_relax_submit)."""
        _lib.check(self._lib.omc_relax_submit(self._h))

    def poll(self):
        r = np.zeros(3, np.int32)
        _lib.check(self._lib.omc_relax_poll(self._h, _lib.ptr(r[0:1]), _lib.ptr(r[1:2]), _lib.ptr(r[2:3])))
        return dict(running=bool(r[0]), nodes_done=int(r[1]), nodes_total=int(r[2]))

    def wait(self):
        _lib.check(self._lib.omc_relax_wait(self._h))

    def fetch(self, want_Y=True, want_X=True, want_Theta=False):
        B, n, m, k = self._B, self.n, self.m, self.k
        obj = np.zeros(B); lb = np.zeros(B); st = np.zeros(B, np.int32); it = np.zeros(B, np.int32)
        Y = np.zeros((B, n * n)) if want_Y else None
        U = np.zeros((B, n * k))
        X = np.zeros((B, n * m)) if want_X else None
        Th = np.zeros((B, m * m)) if want_Theta else None
        lmin = np.zeros((B, 2)); bx = np.zeros((B, n)); tm = np.zeros(B)
        _lib.check(self._lib.omc_relax_fetch(self._h, _lib.ptr(obj), _lib.ptr(lb), _lib.ptr(st), _lib.ptr(it), _lib.ptr(Y),
                                             _lib.ptr(U), _lib.ptr(X), _lib.ptr(Th), _lib.ptr(lmin), _lib.ptr(bx), _lib.ptr(tm)))
        out = []
        for b in range(B):
            r = {
                "objective": float(obj[b]), "dual_bound": float(lb[b]), "termination_status": STATUS_NAMES[int(st[b])],
                "status_code": int(st[b]), "feasible": int(st[b]) != 3, "iters": int(it[b]), "solve_time": float(tm[b]),
                "U": U[b].reshape((n, k), order="F"), "lambda_min": lmin[b].copy(), "breakpoint_vec": bx[b].copy(),
            }
            if want_Y: r["Y"] = Y[b].reshape((n, n), order="F")
            if want_X: r["X"] = X[b].reshape((n, m), order="F")
            if want_Theta: r["Theta"] = Th[b].reshape((m, m), order="F")
            out.append(r)
        return out

    def matrix_completion_SDP_relaxation(self, nodes, disjunctive_cuts_type="linear", params=None, U_lower=None, U_upper=None,
                                         want_Y=True, want_X=True, want_Theta=False, rho_scales=None, add_Shor_valid_inequalities=False,
                                         shor_info=None, shor_penalties=None, want_V=False, load_from=None, save_to=None):
        """Batch form of OMC.jl:1431-1943 (use_disjunctive_cuts = true).  `nodes` = list of cut lists; with
        add_Shor_valid_inequalities = True, `shor_info` = one (constraints_indexes, SOC_constraints_indexes) pair per node and
        every result also carries "W" (OMC.jl:1907-1908)."""
        if add_Shor_valid_inequalities:
            if shor_info is None:
                raise ValueError("add_Shor_valid_inequalities = true needs node.Shor_info (OMC.jl:1508)")
            self.stage_shor(nodes, shor_info, disjunctive_cuts_type, params, U_lower, U_upper, shor_penalties, keep_V=(want_V and self.k == 1),
                            load_from=load_from, save_to=save_to)
            self.solve()
            out = self.fetch(want_Y, want_X, want_Theta)
            for r, Wb in zip(out, self.fetch_shor()):
                r["W"] = Wb
            if want_V and self.k == 1:
                for r, Vb, (mi, _) in zip(out, self.fetch_shor_V(), shor_info):
                    r["V"] = Vb[:len(np.asarray(mi).reshape(-1, 4))]
            elif want_V:                                   # rank k > 1: the lifted variables are an explicit extension of (X, W) (quirk Q5)
                for r, (mi, _) in zip(out, shor_info):
                    r.update(shor_rank_k_extension(self.k, r["X"], r["W"], mi))
            return out
        self.stage(nodes, disjunctive_cuts_type, params, U_lower, U_upper, rho_scales, load_from, save_to)
        self.solve()
        return self.fetch(want_Y, want_X, want_Theta)

    def kernel_stats(self):
        """Launches, units and HIP-event milliseconds per kernel class of the last solve.  The ms of "setup" covers k_setup and k_setup_gram
        (the Gram matrix k_setup used to form itself); its launches and units count k_setup only."""
        nc = len(KERNEL_CLASSES); la = np.zeros(nc, np.int64); ms = np.zeros(nc); un = np.zeros(nc, np.int64)
        _lib.check(self._lib.omc_last_kernel_stats(self._h, _lib.ptr(la), _lib.ptr(ms), _lib.ptr(un)))
        return {KERNEL_CLASSES[i]: dict(launches=int(la[i]), ms=float(ms[i]), units=int(un[i])) for i in range(nc)}

    def host_phases(self):
        """Host time of the last solve between its iterations, by piece (omc_last_host_phases): {piece: dict(ms, count)}; "async_harvests" and
        "quiet_intervals" are counts (harvests run beside the next interval; intervals with one launch of the full eigen-kernel per iteration).
        Everything here is what happens between the iterations, which does not depend on how the iterations record their events; the two
        counts of the iterations themselves that the same call returns are event_counts()."""
        if not hasattr(self._lib, "omc_last_host_phases"):
            raise OmcError(-100, "this build of the library has no omc_last_host_phases")
        ms = np.zeros(len(HOST_PHASES)); cnt = np.zeros(len(HOST_PHASES), np.int64)
        _lib.check(self._lib.omc_last_host_phases(self._h, _lib.ptr(ms), _lib.ptr(cnt)))
        return {HOST_PHASES[i]: dict(ms=float(ms[i]), count=int(cnt[i])) for i in range(len(HOST_PHASES)) if HOST_PHASES[i] not in HOST_BODY_COUNTS}

    def event_counts(self):
        """Event records and stream waits the iterations of the last solve enqueued on their streams (timing, fork, joins, the wait for the main
        stream, the check's wait): dict(records, waits), the last two entries of omc_last_host_phases; zeros from a build without them."""
        if not hasattr(self._lib, "omc_last_host_phases"):
            raise OmcError(-100, "this build of the library has no omc_last_host_phases")
        ms = np.zeros(len(HOST_PHASES)); cnt = np.zeros(len(HOST_PHASES), np.int64)
        _lib.check(self._lib.omc_last_host_phases(self._h, _lib.ptr(ms), _lib.ptr(cnt)))
        return {name[len("body_"):]: int(cnt[HOST_PHASES.index(name)]) for name in HOST_BODY_COUNTS}

    def subspace_stats(self):
        """k_cone_sub accounting of the last solve: calls, power steps, fall-backs to the full eigendecomposition, seedings."""
        out = np.zeros(8, np.int64)
        _lib.check(self._lib.omc_last_subspace_stats(self._h, _lib.ptr(out)))
        return dict(calls=int(out[0]), power_steps=int(out[1]), fallbacks=int(out[2]), seeds=int(out[3]), fail_positive=int(out[4]),
                    fail_steps=int(out[5]), fail_cholesky=int(out[6]), ritz_passes=int(out[7]))

    def shor_subspace_stats(self):
        """The same counters for the order-(n+m) cone of the last Shor-mode solve."""
        out = np.zeros(8, np.int64)
        _lib.check(self._lib.omc_last_shor_subspace_stats(self._h, _lib.ptr(out)))
        return dict(calls=int(out[0]), power_steps=int(out[1]), fallbacks=int(out[2]), seeds=int(out[3]), fail_positive=int(out[4]),
                    fail_steps=int(out[5]), fail_cholesky=int(out[6]), ritz_passes=int(out[7]))

    def kernel_residency(self):
        """Workgroups per CU that the HIP runtime reports for the iteration kernels at the geometry last staged (block size and dynamic
        LDS as launched); -1 for a kernel that geometry does not launch.  Read-only: solver_info() keeps its shape."""
        out = np.zeros(len(RESIDENCY_KERNELS), np.int32)
        _lib.check(self._lib.omc_kernel_residency(self._h, _lib.ptr(out)))
        return {nm: int(v) for nm, v in zip(RESIDENCY_KERNELS, out)}

    def solver_info(self):
        info = np.zeros(8)
        _lib.check(self._lib.omc_last_solver_info(self._h, _lib.ptr(info)))
        return dict(solve_seconds=info[0], jacobi_sweeps=int(info[1]), rho=info[2], r_max=int(info[3]), cone_lds=bool(info[4]),
                    global_lds=bool(info[5]), small_lds=bool(info[6]), R_max=int(info[7]))

    # ---- certificates (include/omc.h "certificates"; the checker is certificate.py) -------------------------------
    def keep_certificates(self, on=True):
        """The stage() calls that follow keep, per node, the multipliers of the check that gave its dual_bound (omc_relax_keep_certificates).
        Refused while a submitted solve runs; stage_shor raises OMC_ERR_UNSUPPORTED while it is on (Shor mode has keep_shor_certificates)."""
        _lib.check(self._lib.omc_relax_keep_certificates(self._h, 1 if on else 0))

    def certificate_plan(self, max_cuts=0, nonstandard_box_rows=0):
        """Strides and bytes per node of the certificates of this instance (omc_certificate_plan, host only)."""
        return certificate_plan(self.n, self.k, int(self.indices.sum()), max_cuts, nonstandard_box_rows)

    def _support(self):
        cols, rows = np.nonzero(self.indices.T)      # the library's nnz order: columns in order, rows ascending
        return rows, cols

    def fetch_certificate(self, ids):
        """certificate.Certificate of every node id (omc_relax_fetch_certificate): ids that fetch_done() has returned while the solve runs, or
        any node of fetch() after it.  Raises OmcError for a batch staged without keep_certificates(), an unfinished id, and a node that
        never reached a rigorous check."""
        n, m, k = self.n, self.m, self.k
        idv = np.ascontiguousarray(np.asarray(list(ids), dtype=np.int32))
        c = len(idv)
        info = self.solver_info()
        Rmax, rmax = max(info["R_max"], 1), max(info["r_max"], 1)
        rows, cols = self._support()
        nnz = rows.size
        ps = (rmax + k) ** 2
        Lam = np.zeros((max(c, 1), max(nnz, 1))); lam = np.zeros((max(c, 1), Rmax)); R = np.zeros(max(c, 1), np.int32)
        Q = np.zeros((max(c, 1), n * rmax)); r = np.zeros(max(c, 1), np.int32); Psi = np.zeros((max(c, 1), ps)); bd = np.zeros(max(c, 1))
        if nnz:
            Lam = np.zeros((max(c, 1), nnz))
        _lib.check(self._lib.omc_relax_fetch_certificate(self._h, c, _lib.ptr(idv), _lib.ptr(Lam), _lib.ptr(lam), _lib.ptr(R), _lib.ptr(Q),
                                                         _lib.ptr(r), _lib.ptr(Psi), _lib.ptr(bd)))
        out = []
        for i in range(c):
            ri = int(r[i]); N3 = ri + k
            dense = np.zeros((n, m)); dense[rows, cols] = Lam[i, :nnz]
            out.append(certificate.Certificate(Lam=dense, lam=lam[i, :int(R[i])].copy(), Q=Q[i, :n * ri].reshape((n, ri), order="F").copy(),
                                               Psi3=Psi[i, :N3 * N3].reshape((N3, N3), order="F").copy(), bound=float(bd[i])))
        return out

    def keep_shor_certificates(self, on=True):
        """The stage_shor() calls that follow keep, per node, the multipliers of the check that gave its dual_bound
        (omc_relax_keep_shor_certificates): a switch of its own, independent of keep_certificates().  Rank 1; refused while a submitted solve runs."""
        _lib.check(self._lib.omc_relax_keep_shor_certificates(self._h, 1 if on else 0))

    def shor_certificate_plan(self, nq_stride, max_cuts=0, nonstandard_box_rows=0):
        """Strides and bytes per node / per slot of the Shor-mode certificates of this instance (omc_shor_certificate_plan, host only)."""
        return shor_certificate_plan(self.n, self.m, self.k, nq_stride, max_cuts, nonstandard_box_rows)

    def fetch_shor_certificate(self, ids):
        """certificate.ShorCertificate of every node id (omc_relax_fetch_shor_certificate): ids that fetch_done() has returned while the solve
        runs, or any node of fetch() after it, staged or appended.  Raises OmcError for a batch staged without keep_shor_certificates(), an
        unfinished id, and a node that never reached a rigorous check.  The lists are the caller's: certificate.shor_dual_bound takes them."""
        n, m, k = self.n, self.m, self.k
        idv = np.ascontiguousarray(np.asarray(list(ids), dtype=np.int32))
        c = len(idv); c1 = max(c, 1)
        stride = np.zeros(1, np.int64)
        _lib.check(self._lib.omc_relax_fetch_shor_certificate(self._h, 0, None, *([None] * 12), _lib.ptr(stride)))
        ns = int(stride[0])
        info = self.solver_info()
        Rmax, rmax = max(info["R_max"], 1), max(info["r_max"], 1)
        ps = (rmax + k) ** 2
        sc = np.zeros(c1); bd = np.zeros(c1); lam = np.zeros((c1, Rmax)); R = np.zeros(c1, np.int32); Q = np.zeros((c1, n * rmax)); r = np.zeros(c1, np.int32)
        Psi = np.zeros((c1, ps)); Gam = np.zeros((c1, 15 * max(ns, 1))); zeta = np.zeros((c1, m)); xi = np.zeros((c1, n * m)); Xb = np.zeros((c1, n * m))
        nq = np.zeros(c1, np.int32)
        _lib.check(self._lib.omc_relax_fetch_shor_certificate(self._h, c, _lib.ptr(idv), _lib.ptr(sc), _lib.ptr(bd), _lib.ptr(lam), _lib.ptr(R), _lib.ptr(Q),
                                                              _lib.ptr(r), _lib.ptr(Psi), _lib.ptr(Gam) if ns else None, _lib.ptr(zeta), _lib.ptr(xi), _lib.ptr(Xb),
                                                              _lib.ptr(nq), None))
        out = []
        for i in range(c):
            ri = int(r[i]); N3 = ri + k
            G = certificate.unpack_gam(Gam[i, :15 * ns].reshape(15, ns), int(nq[i])) if ns else np.zeros((0, 5, 5))
            out.append(certificate.ShorCertificate(scale=float(sc[i]), lam=lam[i, :int(R[i])].copy(), Q=Q[i, :n * ri].reshape((n, ri), order="F").copy(),
                                                   Psi3=Psi[i, :N3 * N3].reshape((N3, N3), order="F").copy(), Gam=G, zeta=zeta[i].copy(),
                                                   xi=xi[i].reshape((n, m), order="F").copy(), Xbar=Xb[i].reshape((n, m), order="F").copy(),
                                                   bound=float(bd[i])))
        return out

    def _bounds_flat(self, B, U_lower, U_upper):
        lo = hi = None
        if U_lower is not None:
            lo = np.ascontiguousarray(np.stack([np.asfortranarray(np.asarray(u, float)).ravel(order="F") for u in U_lower]))
        if U_upper is not None:
            hi = np.ascontiguousarray(np.stack([np.asfortranarray(np.asarray(u, float)).ravel(order="F") for u in U_upper]))
        for a in (lo, hi):
            if a is not None and a.shape != (B, self.n * self.k):
                raise ValueError("U_lower / U_upper: one (n, k) matrix per node")
        return lo, hi

    def row_basis(self, nodes, disjunctive_cuts_type="linear", U_lower=None, U_upper=None, reference_quirk_q1=True):
        """The row basis Q (n x r) the library builds for every node (omc_dual_bound_batch without multipliers: host only, no device call)."""
        n, k, B = self.n, self.k, len(nodes)
        L, cx, cU, cd = _pack_cuts(nodes, n, k, disjunctive_cuts_type)
        lo, hi = self._bounds_flat(B, U_lower, U_upper)
        args = (self._h, B, CUT_TYPES[disjunctive_cuts_type], int(bool(reference_quirk_q1)), _lib.ptr(L), _lib.ptr(cx), _lib.ptr(cU), _lib.ptr(cd),
                _lib.ptr(lo), _lib.ptr(hi), None, None, None)
        r = np.zeros(B, np.int32)
        _lib.check(self._lib.omc_dual_bound_batch(*args, None, _lib.ptr(r), None))
        rmax = max(1, int(r.max()))
        Q = np.zeros((B, n * rmax))
        _lib.check(self._lib.omc_dual_bound_batch(*args, _lib.ptr(Q), _lib.ptr(r), None))
        return [Q[b, :n * int(r[b])].reshape((n, int(r[b])), order="F").copy() for b in range(B)]

    def dual_bound(self, nodes, certs, disjunctive_cuts_type="linear", U_lower=None, U_upper=None, reference_quirk_q1=True):
        """The Lagrangian bound of certs[b] (certificate.Certificate: Lam n x m, lam, Q, Psi3) for nodes[b], evaluated on the device as the
        multipliers are (omc_dual_bound_batch): no sanitising -- certificate.dual_bound is the checker.  Psi3 must be expressed in the basis
        row_basis() returns (the Q of a fetched certificate is that basis).  Returns the B bounds."""
        n, m, k, B = self.n, self.m, self.k, len(nodes)
        if len(certs) != B:
            raise ValueError("one certificate per node")
        L, cx, cU, cd = _pack_cuts(nodes, n, k, disjunctive_cuts_type)
        lo, hi = self._bounds_flat(B, U_lower, U_upper)
        dlo, dhi = certificate.default_U_bounds(n, k)
        Rb = []
        for b in range(B):
            lb_ = dlo if lo is None else lo[b]; hb_ = dhi if hi is None else hi[b]
            Rb.append(1 + int((np.asarray(lb_) > -1.0).sum()) + int((np.asarray(hb_) < 1.0).sum()) + int(L[b]) * (2 * k + 1))
        rb = [int(np.asarray(c.Q).shape[1]) for c in certs]
        Rmax, rmax = max(Rb), max(1, max(rb))
        rows, cols = self._support()
        nnz = rows.size
        ps = (rmax + k) ** 2
        Lam = np.zeros((B, max(nnz, 1))); lam = np.zeros((B, Rmax)); Psi = np.zeros((B, ps))
        for b, c in enumerate(certs):
            if np.asarray(c.Lam).shape != (n, m) or len(c.lam) != Rb[b] or np.asarray(c.Psi3).shape != (rb[b] + k, rb[b] + k):
                raise ValueError(f"certificate {b}: Lam must be n x m, lam hold {Rb[b]} multipliers and Psi3 be of order r + k")
            Lam[b, :nnz] = np.asarray(c.Lam, float)[rows, cols]; lam[b, :Rb[b]] = c.lam
            Psi[b, :(rb[b] + k) ** 2] = np.asarray(c.Psi3, float).ravel(order="F")
        r = np.zeros(B, np.int32); bd = np.zeros(B)
        _lib.check(self._lib.omc_dual_bound_batch(self._h, B, CUT_TYPES[disjunctive_cuts_type], int(bool(reference_quirk_q1)), _lib.ptr(L), _lib.ptr(cx),
                                                  _lib.ptr(cU), _lib.ptr(cd), _lib.ptr(lo), _lib.ptr(hi), None, None, None, None, _lib.ptr(r), None))
        if [int(v) for v in r] != rb:
            raise ValueError(f"Q of the certificates has {rb} columns, the library's row basis {[int(v) for v in r]}: build Psi3 in the basis of row_basis()")
        _lib.check(self._lib.omc_dual_bound_batch(self._h, B, CUT_TYPES[disjunctive_cuts_type], int(bool(reference_quirk_q1)), _lib.ptr(L), _lib.ptr(cx),
                                                  _lib.ptr(cU), _lib.ptr(cd), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(Lam), _lib.ptr(lam), _lib.ptr(Psi),
                                                  None, None, _lib.ptr(bd)))
        return bd

    def shor_dual_bound(self, nodes, shor_info, certs, disjunctive_cuts_type="linear", U_lower=None, U_upper=None, reference_quirk_q1=True,
                        sanitise=True, want_defects=False, want_terms=False, nq_stride=None):
        """The Shor-mode bound of certs[b] (certificate.ShorCertificate) for nodes[b] with the lists shor_info[b] = (minors, SOC list or None),
        evaluated on the device (omc_shor_dual_bound_batch).  sanitise=True is certificate.shor_dual_bound (the multipliers are made admissible,
        the blocks in two ways, the larger value is returned), sanitise=False is certificate.evaluate_shor (as they are).  Psi3 must be expressed
        in the basis row_basis() returns (the Q of a fetched certificate is that basis).  -inf where the formula gives it.  Returns the B bounds;
        with want_defects also a list of dicts (gam_min_eig, v_residual, min_zeta, min_lam, psi_min_eig of the input as given), with want_terms
        also a (B, 4) array (constant, min(eig_0(M), 0), ||c||, min_j mu_j of the evaluation returned, in the scaled variables).  nq_stride:
        stride of the per-minor planes on the wire (default: the longest list); the result does not depend on it."""
        if not hasattr(self._lib, "omc_shor_dual_bound_batch"):
            raise _lib.OmcError(-100, "this libomc_hip.so has no omc_shor_dual_bound_batch")
        n, m, k, B = self.n, self.m, self.k, len(nodes)
        if len(certs) != B or len(shor_info) != B:
            raise ValueError("one certificate and one (minors, SOC list) pair per node")
        L, cx, cU, cd = _pack_cuts(nodes, n, k, disjunctive_cuts_type)
        lo, hi = self._bounds_flat(B, U_lower, U_upper)
        nsh, nso, shi, soi = _pack_shor(shor_info)
        dlo, dhi = certificate.default_U_bounds(n, k)
        Rb = []
        for b in range(B):
            lb_ = dlo if lo is None else lo[b]; hb_ = dhi if hi is None else hi[b]
            Rb.append(1 + int((np.asarray(lb_) > -1.0).sum()) + int((np.asarray(hb_) < 1.0).sum()) + int(L[b]) * (2 * k + 1))
        rb = [int(np.asarray(c.Q).shape[1]) for c in certs]
        Rmax, rmax = max(Rb), max(1, max(rb))
        ns = int(nsh.max()) if nq_stride is None else int(nq_stride)
        ps = (rmax + k) ** 2
        sc = np.zeros(B); lam = np.zeros((B, Rmax)); Psi = np.zeros((B, ps)); Gam = np.zeros((B, 15, max(ns, 1)))
        zeta = np.zeros((B, m)); xi = np.zeros((B, n * m)); Xb = np.zeros((B, n * m))
        for b, c in enumerate(certs):
            G = np.asarray(c.Gam, float).reshape(-1, 5, 5)
            if len(c.lam) != Rb[b] or np.asarray(c.Psi3).shape != (rb[b] + k, rb[b] + k) or len(G) != int(nsh[b]):
                raise ValueError(f"certificate {b}: lam must hold {Rb[b]} multipliers, Psi3 be of order r + k and Gam hold {int(nsh[b])} blocks")
            sc[b] = float(c.scale); lam[b, :Rb[b]] = c.lam
            Psi[b, :(rb[b] + k) ** 2] = np.asarray(c.Psi3, float).ravel(order="F")
            if len(G) and ns >= len(G):
                Gam[b] = certificate.pack_gam(0.5 * (G + np.transpose(G, (0, 2, 1))), ns)
            zeta[b] = np.asarray(c.zeta, float)
            xi[b] = np.asarray(c.xi, float).ravel(order="F"); Xb[b] = np.asarray(c.Xbar, float).ravel(order="F")
        ct = CUT_TYPES[disjunctive_cuts_type]; q1 = int(bool(reference_quirk_q1))
        if k == 1:      # the basis check needs no device; for k > 1 the evaluator itself refuses
            r = np.zeros(B, np.int32)
            _lib.check(self._lib.omc_dual_bound_batch(self._h, B, ct, q1, _lib.ptr(L), _lib.ptr(cx), _lib.ptr(cU), _lib.ptr(cd), _lib.ptr(lo), _lib.ptr(hi),
                                                      None, None, None, None, _lib.ptr(r), None))
            if [int(v) for v in r] != rb:
                raise ValueError(f"Q of the certificates has {rb} columns, the library's row basis {[int(v) for v in r]}: build Psi3 in the basis of row_basis()")
        bd = np.zeros(B); df = np.zeros((B, 5)); tm = np.zeros((B, 4))
        _lib.check(self._lib.omc_shor_dual_bound_batch(self._h, B, ct, q1, _lib.ptr(L), _lib.ptr(cx), _lib.ptr(cU), _lib.ptr(cd), _lib.ptr(lo), _lib.ptr(hi),
                                                       _lib.ptr(nsh), _lib.ptr(shi), _lib.ptr(nso), _lib.ptr(soi), 1 if sanitise else 0, ns, _lib.ptr(sc),
                                                       _lib.ptr(lam), _lib.ptr(Psi), _lib.ptr(Gam) if int(nsh.max()) else None, _lib.ptr(zeta), _lib.ptr(xi),
                                                       _lib.ptr(Xb), _lib.ptr(bd), _lib.ptr(df) if want_defects else None, _lib.ptr(tm) if want_terms else None))
        out = [bd]
        if want_defects:
            keys = ("gam_min_eig", "v_residual", "min_zeta", "min_lam", "psi_min_eig")
            out.append([{key: float(v) for key, v in zip(keys, df[b])} for b in range(B)])
        if want_terms:
            out.append(tm)
        return out[0] if len(out) == 1 else tuple(out)

    def shor_dual_bound_plan(self, B, nq_stride, max_cuts=0, nonstandard_box_rows=0, sanitise=True):
        """Device bytes shor_dual_bound() needs for B nodes of this instance (omc_shor_dual_bound_plan, host only)."""
        return shor_dual_bound_plan(self.n, self.m, self.k, B, nq_stride, max_cuts, nonstandard_box_rows, sanitise)

    def last_shor_dual_bound_ms(self):
        """Event time (ms) of the kernels of the last shor_dual_bound() call, copies excluded."""
        ms = np.zeros(1)
        _lib.check(self._lib.omc_last_shor_dual_bound_ms(self._h, _lib.ptr(ms)))
        return float(ms[0])

    # ---- the index structure of one Shor list (omc_shor_index_build) -----------------------------------------------
    def shor_index(self, shor_idx, soc_idx=None, where="device"):
        """The index structure of one list of minors ((nq, 4) 1-based tuples; soc_idx: None = every entry on the SOC list, else (n_soc, 2)
        1-based pairs), built by the host builder (where="host") or the device builder (where="device") whatever OMC_SHOR_INDEX_DEVICE_MIN
        says.  Returns a dict of numpy arrays at their true lengths (mi and kid as (4, nq)), the counts nq / nv1 / nv2, r4, hash and the
        kernels launched.  Nothing is staged."""
        if where not in ("host", "device"):
            raise ValueError("where is 'host' or 'device'")
        mq = np.ascontiguousarray(np.asarray(shor_idx, np.int64).reshape(-1, 4)); nq = len(mq)
        if soc_idx is None:
            nsoc, sq = -1, np.zeros((1, 2), np.int64)
        else:
            sq = np.ascontiguousarray(np.asarray(soc_idx, np.int64).reshape(-1, 2)); nsoc = len(sq)
            if nsoc == 0:
                sq = np.zeros((1, 2), np.int64)
        if nq == 0:
            mq = np.zeros((1, 4), np.int64)
        n, m = self.n, self.m
        counts = np.zeros(4, np.int64); r4 = np.zeros(1); hv = np.zeros(1, np.uint64)
        i32 = lambda c: np.full(c, -7, np.int32)      # noqa: E731
        o = dict(mi=i32(4 * nq), kid=i32(4 * nq), cptr=i32(n * m + 1), cent=i32(4 * nq), v1ptr=i32(2 * nq + 1), v1ent=i32(2 * nq),
                 v2ptr=i32(2 * nq + 1), v2ent=i32(2 * nq), slackrow=i32(m), eclass=np.full(n * m, 255, np.uint8), ctype=np.full(m, 255, np.uint8))
        _lib.check(self._lib.omc_shor_index_build(self._h, 1 if where == "device" else 0, nq, _lib.ptr(mq), nsoc, _lib.ptr(sq), _lib.ptr(counts),
                                                  _lib.ptr(r4), _lib.ptr(hv), *[_lib.ptr(o[key]) for key in ("mi", "kid", "cptr", "cent", "v1ptr",
                                                  "v1ent", "v2ptr", "v2ent", "slackrow", "eclass", "ctype")]))
        q, nv1, nv2 = int(counts[0]), int(counts[1]), int(counts[2])      # q = 0 for rank k > 1 (quirk Q5)
        o["mi"] = o["mi"][:4 * q].reshape(4, q); o["kid"] = o["kid"][:4 * q].reshape(4, q); o["cent"] = o["cent"][:4 * q]
        o["v1ptr"] = o["v1ptr"][:nv1 + 1]; o["v2ptr"] = o["v2ptr"][:nv2 + 1]; o["v1ent"] = o["v1ent"][:2 * q]; o["v2ent"] = o["v2ent"][:2 * q]
        o.update(nq=q, nv1=nv1, nv2=nv2, launches=int(counts[3]), r4=float(r4[0]), hash=int(hv[0]))
        return o

    def shor_index_plan(self, nq):
        """shor_index_plan for this instance's shape."""
        return shor_index_plan(self.n, self.m, nq)

    def shor_index_stats(self):
        """Lists whose index structure was built on the host / on the device since the last stage_shor() call began, the milliseconds spent
        in each as the caller saw them, and the kernels of the last device build (omc_last_shor_index_stats)."""
        o = np.zeros(5)
        _lib.check(self._lib.omc_last_shor_index_stats(self._h, _lib.ptr(o)))
        return dict(host_lists=int(o[0]), device_lists=int(o[1]), host_ms=float(o[2]), device_ms=float(o[3]), last_launches=int(o[4]))

    # ---- multi-GPU exchange behind the C ABI (RCCL) ------------------------------------------------
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL id, created by rank 0 and handed to every rank by the host (torch.distributed, MPI, a file ...)."""
        buf = np.zeros(128, np.uint8)
        _lib.check(_lib.load().omc_comm_unique_id(_lib.ptr(buf)))
        return buf

    def comm_init(self, rank, world_size, unique_id):
        uid = np.ascontiguousarray(np.asarray(unique_id, np.uint8))
        _lib.check(self._lib.omc_comm_init(self._h, int(rank), int(world_size), _lib.ptr(uid)))
        self.rank, self.world_size = int(rank), int(world_size)

    def allreduce_bounds(self, upper_bound, lower_bound):
        """MIN over ranks of {incumbent UB, smallest open LB}; returns (ub, lb, owner rank of the UB)."""
        ub = np.array([upper_bound], np.float64); lb = np.array([lower_bound], np.float64); ow = np.zeros(1, np.int32)
        _lib.check(self._lib.omc_allreduce_bounds(self._h, _lib.ptr(ub), _lib.ptr(lb), _lib.ptr(ow)))
        return float(ub[0]), float(lb[0]), int(ow[0])

    def allgather_records(self, rows, width, capacity_rows):
        """Rows (cnt, width) of every rank, in rank order, through the library's communicator (omc_allgather_records)."""
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, width))
        out = np.zeros((int(capacity_rows), width)); counts = np.zeros(self.world_size, np.int32)
        _lib.check(self._lib.omc_allgather_records(self._h, _lib.ptr(rows) if len(rows) else None, len(rows), int(width), _lib.ptr(out), int(capacity_rows), _lib.ptr(counts)))
        return out[: int(counts.sum())]

    def bcast_incumbent(self, root, X):
        Xf = np.asfortranarray(np.asarray(X, np.float64).reshape(self.n, self.m))
        _lib.check(self._lib.omc_bcast_incumbent(self._h, int(root), _lib.ptr(Xf)))
        return Xf

    # ---- separation / feasibility ----------------------------------------------------------------------
    def breakpoint_vectors(self, Ys, Us, disjunctive_cuts_breakpoints="smallest_1_eigvec"):
        if disjunctive_cuts_breakpoints not in BREAKPOINTS:
            raise ValueError("Invalid input for disjunctive cuts breakpoints.")                     # OMC.jl:2440-2446
        B, n, k = len(Ys), self.n, self.k
        Yb = np.ascontiguousarray(np.stack([np.asfortranarray(y, dtype=np.float64).ravel(order="F") for y in Ys]))
        Ub = np.ascontiguousarray(np.stack([np.asfortranarray(np.asarray(u, float).reshape(n, k)).ravel(order="F") for u in Us]))
        ev = np.zeros((B, 2)); x = np.zeros((B, n)); fe = np.zeros(B, np.int32)
        _lib.check(self._lib.omc_separation_batch(self._h, B, BREAKPOINTS[disjunctive_cuts_breakpoints], _lib.ptr(Yb), _lib.ptr(Ub),
                                                  _lib.ptr(ev), _lib.ptr(x), _lib.ptr(fe)))
        return x, ev, fe.astype(bool)

    def matrix_completion_master_feasible(self, Y, U):
        """OMC.jl:1261-1277 (disjunctive branch): lambda_min(U U' - Y) >= -1e-6."""
        _, ev, fe = self.breakpoint_vectors([Y], [U])
        return bool(fe[0])

    # ---- rounding glue + alternating minimisation ---------------------------------------------------------
    def round_Y(self, Ys):
        """svd(Y).U[:, 1:k] of the relaxed Y (OMC.jl:873), batched; sign: largest-magnitude entry positive."""
        B, n, k = len(Ys), self.n, self.k
        Yb = np.ascontiguousarray(np.stack([np.asfortranarray(y, dtype=np.float64).ravel(order="F") for y in Ys]))
        U = np.zeros((B, n * k))
        _lib.check(self._lib.omc_round_Y_batch(self._h, B, _lib.ptr(Yb), _lib.ptr(U)))
        return [U[b].reshape((n, k), order="F") for b in range(B)]

    def left_singular(self, Xs):
        """svd(X).U[:, 1:k] of n x m matrices (OMC.jl:524, 564, 921), batched on the device (omc_left_singular_batch); sign: largest-magnitude entry positive."""
        B, n, m, k = len(Xs), self.n, self.m, self.k
        Xb = np.ascontiguousarray(np.stack([np.asfortranarray(x, dtype=np.float64).ravel(order="F") for x in Xs]))
        if Xb.shape != (B, n * m):
            raise ValueError("left_singular: every matrix must be n x m")
        U = np.zeros((B, n * k))
        _lib.check(self._lib.omc_left_singular_batch(self._h, B, _lib.ptr(Xb), _lib.ptr(U)))
        return [U[b].reshape((n, k), order="F") for b in range(B)]

    def psd_project(self, M, lo=0.0, hi=np.inf, algo=0, V0=None, want_evals=False, want_V=False):
        """Spectral clip P = V diag(min(max(lambda, lo), hi)) V' of one symmetric matrix (N x N) or a batch (B x N x N) by the eigen-kernels of
        the relaxation (omc_psd_project_batch; the cones of OMC.jl:1554-1556).  algo: 0 = what a relaxation at this order uses, 1 = single-
        workgroup kernels, 2 = multi-workgroup.  V0: orthonormal starting basis (the V of an earlier call on a nearby matrix).  Returns P, or
        (P, evals, V) with the parts asked for (evals ascending, V's columns in their order), shaped like M."""
        Ma = np.asarray(M, dtype=np.float64)
        single = Ma.ndim == 2
        Mb = Ma[None] if single else Ma
        if Mb.ndim != 3 or Mb.shape[1] != Mb.shape[2]:
            raise ValueError("psd_project: M must be N x N or B x N x N")
        B, N = Mb.shape[0], Mb.shape[1]
        flat = lambda X: np.ascontiguousarray(np.stack([np.asfortranarray(x).ravel(order="F") for x in X]))
        Mf = flat(Mb)
        V0f = None
        if V0 is not None:
            V0b = np.asarray(V0, dtype=np.float64)
            V0b = V0b[None] if V0b.ndim == 2 else V0b
            if V0b.shape != Mb.shape:
                raise ValueError("psd_project: V0 must have the shape of M")
            V0f = flat(V0b)
        P = np.zeros((B, N * N))
        ev = np.zeros((B, N)) if want_evals else None
        V = np.zeros((B, N * N)) if want_V else None
        _lib.check(self._lib.omc_psd_project_batch(self._h, B, N, _lib.ptr(Mf), float(lo), float(hi), int(algo), _lib.ptr(V0f), _lib.ptr(P),
                                                   _lib.ptr(ev), _lib.ptr(V)))
        unflat = lambda X: np.stack([X[b].reshape((N, N), order="F") for b in range(B)])
        out = [unflat(P)] + ([ev] if want_evals else []) + ([unflat(V)] if want_V else [])
        if single:
            out = [o[0] for o in out]
        return out[0] if len(out) == 1 else tuple(out)

    def column_prox(self, Y, alpha_old=None, rho_f=1.0, s0=None, mode=0, algo=0):
        """The column prox of the ADMM iteration on its own (omc_column_prox_batch).  Y: (n, n) or (B, n, n); alpha_old: dense (B, n, m) with
        zeros off the support (None = zeros); rho_f: scalar or (B,); s0: (B, m) starting values (None = cold).  mode 0: the prox, mode 1: the
        exact multipliers of the certificate.  algo: 0 = the solver's dispatch, 1 = without the block kernel, 2 = the block kernel for every
        non-empty column.  Returns a dict: alpha (B, n, m) dense, s (B, m; mode 0), objcol, c0col (B, m; mode 1), nfact (B, m)."""
        n, m = self.n, self.m
        Yb = np.asarray(Y, dtype=np.float64)
        Yb = Yb[None] if Yb.ndim == 2 else Yb
        if Yb.ndim != 3 or Yb.shape[1:] != (n, n):
            raise ValueError("column_prox: Y must be n x n or B x n x n")
        B = Yb.shape[0]
        cols, rows = np.nonzero(self.indices.T)      # the library's nnz order: columns in order, rows ascending
        nnz = rows.size
        Yf = np.ascontiguousarray(np.stack([np.asfortranarray(y).ravel(order="F") for y in Yb]))
        ao = None
        if alpha_old is not None:
            ad = np.asarray(alpha_old, dtype=np.float64)
            ad = ad[None] if ad.ndim == 2 else ad
            if ad.shape != (B, n, m):
                raise ValueError("column_prox: alpha_old must be B x n x m")
            ao = np.ascontiguousarray(ad[:, rows, cols])
        rf = np.ascontiguousarray(np.broadcast_to(np.asarray(rho_f, dtype=np.float64), (B,)))
        s0f = None
        if s0 is not None:
            s0f = np.ascontiguousarray(np.asarray(s0, dtype=np.float64).reshape(B, m))
        al = np.zeros((B, max(nnz, 1))); sv = np.zeros((B, m)); oc = np.zeros((B, m)); cc = np.zeros((B, m)); nf = np.zeros((B, m), np.int32)
        _lib.check(self._lib.omc_column_prox_batch(self._h, B, int(mode), int(algo), _lib.ptr(Yf), _lib.ptr(ao), _lib.ptr(rf), _lib.ptr(s0f),
                                                   _lib.ptr(al), _lib.ptr(sv), _lib.ptr(oc), _lib.ptr(cc), _lib.ptr(nf)))
        dense = np.zeros((B, n, m))
        dense[:, rows, cols] = al[:, :nnz]
        return dict(alpha=dense, s=sv, objcol=oc, c0col=cc, nfact=nf)

    def row_project(self, G, c, lam0=None, which=1):
        """The exact projection on the linear rows (step 4 of k_global) on its own (omc_row_project_batch): lam = argmin 1/2 l'G l - c'l,
        l >= 0.  G: (R, R) or (B, R, R) symmetric; c, lam0: (R,) or (B, R) (lam0 None = zeros, the warm start otherwise).  which: 0 = the
        routines of the alternating-minimisation kernels, 1 = the ones k_global runs.  Returns (lam (B, R), overflow (B,) int32), or the
        pair for the one problem."""
        if not hasattr(self._lib, "omc_row_project_batch"):
            raise _lib.OmcError(-4, "this build of the library has no omc_row_project_batch")
        Ga = np.asarray(G, dtype=np.float64)
        single = Ga.ndim == 2
        Gb = np.ascontiguousarray(Ga[None] if single else Ga)
        if Gb.ndim != 3 or Gb.shape[1] != Gb.shape[2]:
            raise ValueError("row_project: G must be R x R or B x R x R")
        B, R = Gb.shape[0], Gb.shape[1]
        cb = np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(B, R))
        l0 = None if lam0 is None else np.ascontiguousarray(np.asarray(lam0, dtype=np.float64).reshape(B, R))
        lam = np.zeros((B, R)); ov = np.zeros(B, np.int32)
        _lib.check(self._lib.omc_row_project_batch(self._h, B, R, R, int(which), _lib.ptr(Gb), _lib.ptr(cb), _lib.ptr(l0), _lib.ptr(lam),
                                                   _lib.ptr(ov)))
        return (lam[0], int(ov[0])) if single else (lam, ov)

    def colprox_plan(self, block_min=65, cmax=None):
        """Launch plan of k_colprox_block for this instance's longest column (or cmax) under OMC_COLPROX_BLOCK_MIN = block_min
        (omc_colprox_plan, host only)."""
        return colprox_plan(self.n, int(self.indices.sum(axis=0).max()) if cmax is None else int(cmax), block_min)

    def cone_multi_stats(self):
        """Sweep accounting of the multi-workgroup eigen-kernels in the last solve, or of the last psd_project call (omc_last_cone_multi_stats)."""
        out = np.zeros(5, np.int64)
        _lib.check(self._lib.omc_last_cone_multi_stats(self._h, _lib.ptr(out)))
        return dict(calls=int(out[0]), last_sweeps=int(out[1]), exhausted=int(out[2]), max_sweeps=int(out[3]), device_us=int(out[4]))

    def plain_multi_stats(self):
        """The multi-workgroup eigen-kernels under breakpoint_vectors, round_Y and left_singular in the last such call, or under the
        harvests of the last solve (omc_last_plain_multi_stats); counters apart from cone_multi_stats()."""
        if not hasattr(self._lib, "omc_last_plain_multi_stats"):
            raise _lib.OmcError(-4, "this build of the library has no omc_last_plain_multi_stats")
        out = np.zeros(4, np.int64)
        _lib.check(self._lib.omc_last_plain_multi_stats(self._h, _lib.ptr(out)))
        return dict(calls=int(out[0]), max_sweeps=int(out[1]), exhausted=int(out[2]), device_us=int(out[3]))

    def alternating_minimization(self, U_initials, nodes=None, disjunctive_cuts_type="linear", eps=1e-5, max_iters=100,
                                 time_limit=3600.0, reference_quirk_q1=True):
        """Batch form of OMC.jl:1979-2279 (use_disjunctive_cuts = true).  Returns dicts with the reference's keys
        converged, U, V, solve_time, n_iters, max_iters, objectives (OMC.jl:2249-2257)."""
        n, m, k = self.n, self.m, self.k
        B = len(U_initials)
        nodes = nodes if nodes is not None else [[] for _ in range(B)]
        L, cx, cU, cd = _pack_cuts(nodes, n, k, disjunctive_cuts_type)
        U0 = np.ascontiguousarray(np.stack([np.asfortranarray(np.asarray(u, float).reshape(n, k)).ravel(order="F") for u in U_initials]))
        U = np.zeros((B, n * k)); V = np.zeros((B, k * m)); cv = np.zeros(B, np.int32); ni = np.zeros(B, np.int32)
        obj = np.zeros((B, max_iters)); tm = np.zeros(B)
        _lib.check(self._lib.omc_altmin_batch(self._h, B, CUT_TYPES[disjunctive_cuts_type], int(reference_quirk_q1), _lib.ptr(L),
                                              _lib.ptr(cx), _lib.ptr(cU), _lib.ptr(cd), _lib.ptr(U0), float(eps), int(max_iters),
                                              float(time_limit), _lib.ptr(U), _lib.ptr(V), _lib.ptr(cv), _lib.ptr(ni), _lib.ptr(obj), _lib.ptr(tm)))
        mo = np.full(B, np.nan)
        if time_limit > 0:
            _lib.check(self._lib.omc_altmin_master_objectives(self._h, B, _lib.ptr(mo)))
        # master_objective = evaluate_objective(U V) (OMC.jl:920-927), evaluated on the device from the factors
        return [dict(converged=bool(cv[b]), U=U[b].reshape((n, k), order="F"), V=V[b].reshape((k, m), order="F"),
                     solve_time=float(tm[b]), n_iters=int(ni[b]), max_iters=max_iters, objectives=list(obj[b, :ni[b] - (0 if cv[b] or ni[b] == 0 or not np.isnan(obj[b, ni[b] - 1]) else 1)]),
                     master_objective=float(mo[b])) for b in range(B)]

    def altmin_plan(self, max_cuts=0, nolds=False):
        """Launch plan of alternating_minimization for this instance with at most max_cuts cuts per problem (omc_altmin_plan, host only):
        kernel variant (1: rank 1, 2: ranks 2 - 4, 3: ranks 5 - 8), dynamic LDS bytes, bytes of global slab per problem, rows of model_U."""
        out = np.zeros(4, np.int64)
        _lib.check(self._lib.omc_altmin_plan(self.n, self.m, self.k, int(max_cuts), int(bool(nolds)), _lib.ptr(out)))
        return dict(variant=int(out[0]), lds_bytes=int(out[1]), slab_bytes=int(out[2]), Rmax=int(out[3]))

    # ---- objective -------------------------------------------------------------------------------------
    # ---- Shor minors (OMC.jl:2545-2640) ------------------------------------------------------------------------
    def shor_count(self, num_entries_present_list):
        cl = np.asarray(list(num_entries_present_list), dtype=np.int32)
        out = np.zeros(max(len(cl), 1), dtype=np.int64)
        _lib.check(self._lib.omc_shor_count(self._h, len(cl), _lib.ptr(cl), _lib.ptr(out)))
        return out[:len(cl)]

    def generate_rank1_matrix_completion_Shor_constraints_indexes(self, num_entries_present_list):
        """OMC.jl:2545-2612 on the device.  Returns an int64 array (count, 4) of 1-based (i1, i2, j1, j2) in the
        reference's push order (the instance's `indices` is the mask)."""
        cl = np.asarray(list(num_entries_present_list), dtype=np.int32)
        cnt = np.zeros(1, dtype=np.int64)
        _lib.check(self._lib.omc_shor_indexes(self._h, len(cl), _lib.ptr(cl), 0, None, _lib.ptr(cnt)))
        out = np.zeros((int(cnt[0]), 4), dtype=np.int64)
        if cnt[0] > 0:
            _lib.check(self._lib.omc_shor_indexes(self._h, len(cl), _lib.ptr(cl), int(cnt[0]), _lib.ptr(out), _lib.ptr(cnt)))
        return out

    def generate_violated_Shor_minors(self, X, num_entries_present_list, Shor_constraints_indexes, n_minors):
        """OMC.jl:2614-2640 on the device.  X has shape (k, n, m) as in the reference; returns [(score, (i1, i2, j1, j2)), ...]
        in decreasing (score, tuple) order, at most n_minors of them."""
        X = np.asarray(X, dtype=np.float64)
        if X.shape != (self.k, self.n, self.m):
            raise ValueError("Dimension mismatch.\nInput array X must have size (k, n, m).")
        Xf = np.asfortranarray(X).ravel(order="F")        # Julia Array{Float64,3} layout
        cl = np.asarray(list(num_entries_present_list), dtype=np.int32)
        ex = np.ascontiguousarray(np.asarray(list(Shor_constraints_indexes), dtype=np.int64).reshape(-1, 4))
        K = int(n_minors)
        sc = np.zeros(max(K, 1)); mi = np.zeros((max(K, 1), 4), dtype=np.int64); no = np.zeros(1, dtype=np.int32)
        _lib.check(self._lib.omc_violated_shor_minors(self._h, _lib.ptr(Xf), len(cl), _lib.ptr(cl), len(ex), _lib.ptr(ex) if len(ex) else None,
                                                      K, _lib.ptr(sc), _lib.ptr(mi), _lib.ptr(no)))
        return [(float(sc[r]), tuple(int(v) for v in mi[r])) for r in range(int(no[0]))]

    def shor_last_stats(self):
        ms = np.zeros(1); c = np.zeros(1, dtype=np.int64)
        _lib.check(self._lib.omc_shor_last_stats(self._h, _lib.ptr(ms), _lib.ptr(c)))
        return {"ms": float(ms[0]), "candidates": int(c[0])}

    def shor_last_select_stats(self):
        """How the last generate_violated_Shor_minors call selected (omc_shor_last_select_stats): `streamed` is 1 when no key per candidate
        was kept in device memory (knob OMC_SHOR_SELECT_KB), `peak_bytes` the key / survivor memory it asked for."""
        o = np.zeros(4, dtype=np.int64)
        _lib.check(self._lib.omc_shor_last_select_stats(self._h, _lib.ptr(o)))
        return {"streamed": int(o[0]), "tiles": int(o[1]), "compactions": int(o[2]), "peak_bytes": int(o[3])}

    def evaluate_objective(self, X):
        X = np.asarray(X, dtype=np.float64)
        single = X.ndim == 2
        Xs = [X] if single else list(X)
        for x in Xs:
            if x.shape != (self.n, self.m):
                raise ValueError("Dimension mismatch.\nInput matrix X must have size (n, m).")          # OMC.jl:2337-2348
        Xb = np.ascontiguousarray(np.stack([np.asfortranarray(x).ravel(order="F") for x in Xs]))
        out = np.zeros(len(Xs))
        _lib.check(self._lib.omc_evaluate_objective(self._h, len(Xs), _lib.ptr(Xb), _lib.ptr(out)))
        return float(out[0]) if single else out
