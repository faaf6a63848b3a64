"""Independent check of a node's dual certificate: numpy only, no GPU, no library call.  Base (disjunctive) mode first; the Shor-mode
certificate (ShorCertificate, shor_structure, sanitise_shor, shor_dual_bound) follows below with a header of its own.

The relaxation of a node (OMC.jl:1431-1943, disjunctive mode) minimises f(Y) = 1/2 sum_j a_j'(I + gamma Y[O_j,O_j])^-1 a_j over
0 <= Y <= I, tr Y <= k, [Y U; U' I] >= 0 and the node's linear rows <CY_r, Y> + <CU_r, U> <= rhs_r.  For ANY multipliers
    Lam   n x m, zero off the observed pattern,
    lam   one value >= 0 per row,
    Psi3  symmetric positive semidefinite of order r + k (Q, n x r, spans the columns of every CU_r),
the number
    M     = -gamma/2 Lam Lam' + sum_{aggregated rows} lam_r x_r x_r' - Q Psi3[:r,:r] Q'
    c_j   = (Q' sum_{r != trace} lam_r CU_r)[:, j] - 2 Psi3[:r, r+j]
    bound = <A, Lam> - 1/2 ||Lam||_F^2 + sum_{i<k} min(eig_i(M), 0) - sum_j ||c_j|| - sum_{r != trace} lam_r rhs_r - tr Psi3[r:, r:]
is a lower bound on the optimum: Fenchel's inequality f(Y) >= <A,Lam> - 1/2||Lam||^2 - gamma/2 <Y, Lam Lam'>, weak duality for the rows
and for the cone [Q'YQ Q'U; U'Q I] >= 0 (implied by [Y U; U' I] >= 0), and the minimum of the resulting linear function over the superset
{0 <= Y <= I, tr Y <= k} x {||(Q'U)_j|| <= 1}.  `dual_bound` first makes the multipliers admissible (`sanitise`), so what it returns is a
valid bound whatever produced the certificate; how far it falls below the engine's reported dual_bound, and the three defects, measure
the engine.

Rows of a node (OMC.jl:1558-1683), in the public order of include/omc.h:
    trace ; box rows, j outer, i inner, `lo` (-U_ij <= -lower_ij, where lower_ij > -1) before `hi` (U_ij <= upper_ij, where upper_ij < 1) ;
    per cut and column j: x'U_j <= hi_j then -x'U_j <= -lo_j, and after the k columns the aggregated row
    x'Y x - sum_j slope_j x'U_j <= sum_j intercept_j.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

DIR_NAMES = ["left", "middle", "right", "inner_left", "inner_right"]


@dataclass
class Certificate:
    """Multipliers behind one node's bound.  Lam: n x m dense (zero off the support); lam: R; Q: n x r; Psi3: (r + k) x (r + k);
    bound: what the engine reported for them (None for multipliers of the caller's own)."""
    Lam: np.ndarray
    lam: np.ndarray
    Q: np.ndarray
    Psi3: np.ndarray
    bound: float | None = None


def default_U_bounds(n, k):
    """U in [-1, 1] with U[n-k+j:, j] >= 0 (OMC.jl:1442-1449, 0-based)."""
    lo = -np.ones((n, k)); hi = np.ones((n, k))
    for j in range(k):
        lo[n - k + j:, j] = 0.0
    return lo, hi


def cut_piece(cut_type, direction, vhat, q1=True):
    """(lo, hi, slope, intercept) of one piece of the over-estimator of v^2 (OMC.jl:1580-1678): lo <= v <= hi, g(v) = slope v + intercept.
    q1: linear3 / right as OMC.jl:1675 writes it (g = a v); False: the secant (1 + a) v - a."""
    a = abs(vhat)
    table = {
        ("linear", "left"): (-1.0, vhat, vhat - 1.0, vhat),
        ("linear", "right"): (vhat, 1.0, vhat + 1.0, -vhat),
        ("linear2", "left"): (-1.0, -a, -(1.0 + a), -a),
        ("linear2", "middle"): (-a, a, 0.0, vhat * vhat),
        ("linear2", "right"): (a, 1.0, 1.0 + a, -a),
        ("linear3", "left"): (-1.0, -a, -(1.0 + a), -a),
        ("linear3", "inner_left"): (-a, 0.0, -a, 0.0),
        ("linear3", "inner_right"): (0.0, a, a, 0.0),
        ("linear3", "right"): (a, 1.0, a, 0.0) if q1 else (a, 1.0, 1.0 + a, -a),
    }
    if cut_type not in ("linear", "linear2", "linear3"):
        raise ValueError("Invalid input for disjunctive cuts type (OMC.jl:1456-1462)")
    if (cut_type, direction) not in table:
        raise ValueError(f"direction {direction!r} invalid for cut type {cut_type!r}")
    return table[(cut_type, direction)]


def node_rows(n, k, cuts, cut_type, U_lower=None, U_upper=None, q1=True):
    """The rows of a node in the public order: a list of (kind, x, CU, rhs) with kind in trace | box_lo | box_hi | hi | lo | cut,
    x the breakpoint vector of an aggregated row (None otherwise), CU the n x k coefficient on U."""
    dlo, dhi = default_U_bounds(n, k)
    U_lower = dlo if U_lower is None else np.asarray(U_lower, float)
    U_upper = dhi if U_upper is None else np.asarray(U_upper, float)
    if U_lower.shape != (n, k) or U_upper.shape != (n, k):
        raise ValueError("Dimension mismatch: U_lower / U_upper must be (n, k) (OMC.jl:1465-1477)")
    rows = [("trace", None, np.zeros((n, k)), float(k))]
    for j in range(k):
        for i in range(n):
            if U_lower[i, j] > -1.0:
                CU = np.zeros((n, k)); CU[i, j] = -1.0
                rows.append(("box_lo", None, CU, -float(U_lower[i, j])))
            if U_upper[i, j] < 1.0:
                CU = np.zeros((n, k)); CU[i, j] = 1.0
                rows.append(("box_hi", None, CU, float(U_upper[i, j])))
    for (x, Uhat, dirs) in cuts:
        x = np.asarray(x, float); Uhat = np.asarray(Uhat, float).reshape(n, k)
        if x.shape != (n,) or len(dirs) != k:
            raise ValueError("cut must be (x in R^n, Uhat in R^{n x k}, k directions) (OMC.jl:34)")
        vhat = Uhat.T @ x
        CUc = np.zeros((n, k)); rhs = 0.0
        for j in range(k):
            d = dirs[j] if isinstance(dirs[j], str) else DIR_NAMES[int(dirs[j])]
            lo, hi, sl, ic = cut_piece(cut_type, d, float(vhat[j]), q1)
            CUc[:, j] = -sl * x; rhs += ic
            CU = np.zeros((n, k)); CU[:, j] = x
            rows.append(("hi", None, CU, float(hi)))
            rows.append(("lo", None, -CU, -float(lo)))
        rows.append(("cut", x, CUc, float(rhs)))
    return rows


def row_basis(rows, n, k, tol=1e-10):
    """Q (n x r): modified Gram-Schmidt, twice, over the normalised nonzero columns of every CU_r in row order (what the engine's host code does)."""
    Q = []
    for (kind, _x, CU, _rhs) in rows:
        if kind == "trace":
            continue
        for j in range(k):
            nrm = np.linalg.norm(CU[:, j])
            if nrm == 0.0:
                continue
            v = CU[:, j] / nrm
            for _ in range(2):
                for q in Q:
                    v = v - (q @ v) * q
            nv = np.linalg.norm(v)
            if nv > tol and len(Q) < n:
                Q.append(v / nv)
    return np.stack(Q, 1) if Q else np.zeros((n, 0))


def defects(cert, indices):
    """How far the multipliers are from admissible: the mass of Lam off the support (sum of absolute values), min(lam), lambda_min(Psi3)."""
    indices = np.asarray(indices, bool)
    Psi = np.asarray(cert.Psi3, float)
    return dict(off_support=float(np.abs(np.asarray(cert.Lam, float)[~indices]).sum()),
                min_lam=float(np.min(cert.lam)) if len(cert.lam) else 0.0,
                psi_min_eig=float(np.linalg.eigvalsh(0.5 * (Psi + Psi.T))[0]) if Psi.size else 0.0)


def sanitise(cert, indices):
    """Admissible multipliers next to the given ones: Lam dropped off the support, lam clamped at 0, Psi3 replaced by its PSD part."""
    indices = np.asarray(indices, bool)
    Lam = np.where(indices, np.asarray(cert.Lam, float), 0.0)
    lam = np.maximum(np.asarray(cert.lam, float), 0.0)
    Psi = np.asarray(cert.Psi3, float)
    if Psi.size:
        w, V = np.linalg.eigh(0.5 * (Psi + Psi.T))
        Psi = (V * np.maximum(w, 0.0)) @ V.T
    return Certificate(Lam=Lam, lam=lam, Q=np.asarray(cert.Q, float), Psi3=Psi, bound=cert.bound)


def evaluate(A, indices, gamma, k, rows, cert):
    """The bound of the module docstring for the multipliers as they are (no sanitising)."""
    A = np.asarray(A, float); indices = np.asarray(indices, bool)
    n = A.shape[0]
    Lam = np.asarray(cert.Lam, float); lam = np.asarray(cert.lam, float); Q = np.asarray(cert.Q, float); Psi = np.asarray(cert.Psi3, float)
    r = Q.shape[1]
    if len(lam) != len(rows):
        raise ValueError(f"lam holds {len(lam)} multipliers, the node has {len(rows)} rows")
    if Psi.shape != (r + k, r + k):
        raise ValueError(f"Psi3 must be of order r + k = {r + k}")
    c0 = float((A * Lam).sum()) - 0.5 * float((Lam * Lam).sum())
    M = -0.5 * gamma * (Lam @ Lam.T)
    cU = np.zeros((n, k)); const = 0.0
    for (kind, x, CU, rhs), lv in zip(rows, lam):
        if kind == "trace" or lv == 0.0:
            continue
        if kind == "cut":
            M += lv * np.outer(x, x)
        cU += lv * CU
        const -= lv * rhs
    M -= Q @ Psi[:r, :r] @ Q.T
    cV = Q.T @ cU - 2.0 * Psi[:r, r:]
    const -= float(np.trace(Psi[r:, r:]))
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    return c0 + float(np.minimum(ev[:k], 0.0).sum()) - float(np.linalg.norm(cV, axis=0).sum()) + const


def dual_bound(A, indices, gamma, k, cuts, cut_type, cert, U_lower=None, U_upper=None, q1=True, want_defects=False):
    """A valid lower bound on the node's relaxation optimum from `cert`, whatever produced it: the multipliers are sanitised, then
    evaluated.  want_defects: also return defects(cert, indices) of the multipliers as given."""
    A = np.asarray(A, float)
    rows = node_rows(A.shape[0], k, cuts, cut_type, U_lower, U_upper, q1)
    val = evaluate(A, indices, gamma, k, rows, sanitise(cert, indices))
    return (val, defects(cert, indices)) if want_defects else val


def plan(n, k, nnz, max_cuts=0, nonstandard_box_rows=0):
    """The strides of omc_certificate_plan computed in Python: doubles of Lam, lam, Q and Psi3 per node, bytes the arena holds per node, rmax."""
    Rmax = 1 + k * (k + 1) // 2 + nonstandard_box_rows + max_cuts * (2 * k + 1)
    rmax = max(1, min(n, k + nonstandard_box_rows + max_cuts))
    psi = (rmax + k) ** 2
    return dict(Lam=nnz, lam=Rmax, Q=n * rmax, Psi3=psi, bytes_per_node=8 * (1 + nnz + Rmax + psi) + 4, rmax=rmax)


# ---- Shor mode (rank 1) ------------------------------------------------------------------------------------------------------------------------
# The program of a node with add_Shor_valid_inequalities = true (OMC.jl:1503-1525 variables, 1755-1779 cones, 1838-1846 objective), reduced as
# DESIGN.md section 3.7 argues: W lives on the coordinates C of the minors; off C the rotated cones, W >= 0 and Theta_jj = sum_i W_ij collapse to
# one paraboloid per column, t_j = Theta_jj - sum_{C_j} W >= ||X[S_j, j]||^2 (S_j: SOC rows of the column outside C), whose slack sits on the
# cheapest entry outside C.  Column types: 0 an unobserved entry outside C exists (slack is free; observed SOC entries keep 1/2 X^2 as a quadratic
# term), 1 entries outside C exist and all are observed (slack costs 1/2), 2 the whole column is in C (Theta_jj = sum_C W is an equality).
#
# For ANY multipliers
#     Gam_q   symmetric positive semidefinite of order 5, one per minor (rows: 1, (i1,j1), (i1,j2), (i2,j1), (i2,j2)),
#     zeta_j  >= 0 on the paraboloid of a type-0/1 column, linearised at xi_j,
#     lam, Q, Psi3 as in the base certificate,
# the steps below give a lower bound on the optimum of the program of scale * A, which is scale^2 times the node's:
#   spread   the entries of Gam_q that multiply V1, V2, V3 must cancel over the blocks that share the variable: each residual is averaged over
#            those blocks and subtracted, and the block is shifted by the Frobenius norm of what was subtracted (it stays PSD); a block that
#            is still indefinite after that (its input was) is shifted further by its most negative eigenvalue -- a multiple of the identity
#            leaves the entries on V1, V2, V3 alone, so the cancellation holds and the block that enters the bound is PSD whatever came in;
#   zeta     stationarity in W on C asks zeta_j >= sum_q Gam_q[p,p] - cW_ij: zeta_j is raised to the largest of them (type 2: set to it);
#   mu, phi  [[Phi_j, phi_j], [phi_j', mu_j]] >= 0 multiplies [[Y, X_j], [X_j', Theta_jj]] >= 0: stationarity in Theta fixes mu_j = cT_j - zeta_j,
#            in X it fixes phi_j (the gradient q Xbar of a quadratic term stays with it: -1/2 q Xbar^2); mu_j <= 0 with phi_j != 0 has no
#            admissible Phi_j and the bound is -inf; else Phi_j = phi_j phi_j' / mu_j and M = -sum_j Phi_j + cut rows - Q Psi3_11 Q';
#   minimum  of what is left over {0 <= Y <= I, tr Y <= 1} x {||(Q'U)|| <= 1}: the smallest eigenvalue of M where negative, and ||c||.
@dataclass
class ShorCertificate:
    """Multipliers behind one Shor-mode node's bound, in the engine's scaled variables.  Gam: (nq, 5, 5); zeta: m; xi, Xbar: n x m; lam, Q,
    Psi3 as in Certificate; scale: the engine solved the program of scale * A; bound: the reported (unscaled) dual_bound."""
    scale: float
    lam: np.ndarray
    Q: np.ndarray
    Psi3: np.ndarray
    Gam: np.ndarray
    zeta: np.ndarray
    xi: np.ndarray
    Xbar: np.ndarray
    bound: float | None = None


# packed index of (r, c), r <= c, in the upper triangle by columns (include/omc.h): c (c + 1) / 2 + r
_TRI = [(r, c) for c in range(5) for r in range(c + 1)]


def unpack_gam(packed, nq):
    """(15, stride) entry-major packed upper triangles -> (nq, 5, 5) symmetric matrices."""
    packed = np.asarray(packed, float)
    G = np.zeros((nq, 5, 5))
    for e, (r, c) in enumerate(_TRI):
        G[:, r, c] = packed[e, :nq]; G[:, c, r] = packed[e, :nq]
    return G


def pack_gam(Gam, stride=None):
    """The inverse of unpack_gam for symmetric blocks (the upper triangle is read)."""
    Gam = np.asarray(Gam, float).reshape(-1, 5, 5)
    out = np.zeros((15, len(Gam) if stride is None else stride))
    for e, (r, c) in enumerate(_TRI):
        out[e, :len(Gam)] = Gam[:, r, c]
    return out


@dataclass
class ShorStructure:
    """What the formula needs of a node's lists: key ids of the V1 / V2 variables of every minor and how many blocks share each, the
    coordinates of the four entries of every minor (block order (i1,j1), (i1,j2), (i2,j1), (i2,j2)), inC, inS, the column types."""
    nq: int
    k12: np.ndarray
    k34: np.ndarray
    k13: np.ndarray
    k24: np.ndarray
    cnt1: np.ndarray
    cnt2: np.ndarray
    ci: np.ndarray
    cj: np.ndarray
    inC: np.ndarray
    inS: np.ndarray
    ctype: np.ndarray


def shor_structure(n, m, mask, shor_idx, soc_idx=None):
    """shor_idx: (nq, 4) 1-based (i1, i2, j1, j2); soc_idx: (ns, 2) 1-based (i, j), or None for "every coordinate outside the minors"
    (what the reference's driver builds, OMC.jl:656-673)."""
    mask = np.asarray(mask, bool)
    q = np.asarray(shor_idx if shor_idx is not None and len(shor_idx) else np.zeros((0, 4)), np.int64).reshape(-1, 4) - 1
    nq = len(q)
    i1, i2, j1, j2 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    if nq and not ((0 <= i1).all() and (i1 < i2).all() and (i2 < n).all() and (0 <= j1).all() and (j1 < j2).all() and (j2 < m).all()):
        raise ValueError("Shor minors must satisfy 1 <= i1 < i2 <= n, 1 <= j1 < j2 <= m (OMC.jl:2556-2603)")
    if nq and len(np.unique(q, axis=0)) != nq:
        raise ValueError("duplicate Shor minor")
    # V1[i, (j1, j2)] sits at (1,2) for i1 and (3,4) for i2; V2[(i1, i2), j] at (1,3) for j1 and (2,4) for j2 (OMC.jl:1772-1776)
    a1 = np.concatenate([np.stack([i1, j1, j2], 1), np.stack([i2, j1, j2], 1)])
    a2 = np.concatenate([np.stack([i1, i2, j1], 1), np.stack([i1, i2, j2], 1)])
    if nq:
        u1, inv1 = np.unique(a1, axis=0, return_inverse=True); u2, inv2 = np.unique(a2, axis=0, return_inverse=True)
        inv1 = np.asarray(inv1).ravel(); inv2 = np.asarray(inv2).ravel()
    else:
        u1 = u2 = np.zeros((0, 3), np.int64); inv1 = inv2 = np.zeros(0, np.int64)
    ci = np.stack([i1, i1, i2, i2], 1); cj = np.stack([j1, j2, j1, j2], 1)
    inC = np.zeros((n, m), bool)
    inC[ci.ravel(), cj.ravel()] = True
    if soc_idx is None:
        soc = ~inC
    else:
        s = np.asarray(soc_idx, np.int64).reshape(-1, 2) - 1
        if len(s) and not ((0 <= s[:, 0]).all() and (s[:, 0] < n).all() and (0 <= s[:, 1]).all() and (s[:, 1] < m).all()):
            raise ValueError("SOC coordinates out of range")
        soc = np.zeros((n, m), bool)
        soc[s[:, 0], s[:, 1]] = True
    out_of_C = ~inC
    ctype = np.where((out_of_C & ~mask).any(0), 0, np.where(out_of_C.any(0), 1, 2))
    return ShorStructure(nq=nq, k12=inv1[:nq], k34=inv1[nq:], k13=inv2[:nq], k24=inv2[nq:],
                         cnt1=np.bincount(inv1, minlength=len(u1)).astype(float), cnt2=np.bincount(inv2, minlength=len(u2)).astype(float),
                         ci=ci, cj=cj, inC=inC, inS=soc & ~inC, ctype=ctype)


def _v_residuals(st, Gm):
    """Per key of V1 / V2 and per minor for V3: the mean over the blocks that share the variable of the entries that multiply it."""
    r1 = np.zeros(len(st.cnt1)); r2 = np.zeros(len(st.cnt2))
    np.add.at(r1, st.k12, Gm[:, 1, 2]); np.add.at(r1, st.k34, Gm[:, 3, 4])
    np.add.at(r2, st.k13, Gm[:, 1, 3]); np.add.at(r2, st.k24, Gm[:, 2, 4])
    return r1 / np.maximum(st.cnt1, 1.0), r2 / np.maximum(st.cnt2, 1.0), 0.5 * (Gm[:, 1, 4] + Gm[:, 2, 3])


def sanitise_shor(cert, st):
    """Admissible multipliers next to the given ones, and the defects of the given ones: (ShorCertificate, dict).  PSD part of every
    symmetrised Gam_q, zeta clamped at 0 on the type-0/1 columns, lam clamped at 0, PSD part of Psi3; a scale that is not positive and finite
    becomes nan (shor_dual_bound then returns -inf).  Defects: gam_min_eig (smallest eigenvalue over the blocks), min_zeta (type-0/1 columns),
    min_lam, psi_min_eig, v_residual (largest |mean entry| that fails to cancel in V1 / V2 / V3, before the spread)."""
    nq = st.nq
    Gam = np.asarray(cert.Gam, float).reshape(-1, 5, 5)
    if len(Gam) != nq:
        raise ValueError(f"Gam holds {len(Gam)} blocks, the node has {nq} minors")
    Gm = 0.5 * (Gam + np.transpose(Gam, (0, 2, 1)))
    df = dict(gam_min_eig=0.0, v_residual=0.0)
    if nq:
        e1, e2, e3 = _v_residuals(st, Gm)
        df["v_residual"] = float(max(np.abs(e1).max(), np.abs(e2).max(), np.abs(e3).max()))
        w, V = np.linalg.eigh(Gm)
        df["gam_min_eig"] = float(w.min())
        # the PSD part as "the block minus its negative part": a block that is PSD up to rounding comes back unchanged up to that rounding,
        # where rebuilding V max(w, 0) V' would round every entry again
        Gm = Gm - np.einsum("qij,qj,qkj->qik", V, np.minimum(w, 0.0), V)
    zeta = np.asarray(cert.zeta, float).copy()
    t01 = st.ctype != 2
    df["min_zeta"] = float(zeta[t01].min()) if t01.any() else 0.0
    zeta[t01] = np.maximum(zeta[t01], 0.0)
    lam = np.asarray(cert.lam, float)
    df["min_lam"] = float(lam.min()) if len(lam) else 0.0
    Psi = np.asarray(cert.Psi3, float)
    df["psi_min_eig"] = 0.0
    if Psi.size:
        w, V = np.linalg.eigh(0.5 * (Psi + Psi.T))
        df["psi_min_eig"] = float(w[0])
        Psi = (V * np.maximum(w, 0.0)) @ V.T
    sc = float(cert.scale)
    if not (np.isfinite(sc) and sc > 0.0):
        sc = float("nan")
    return ShorCertificate(scale=sc, lam=np.maximum(lam, 0.0), Q=np.asarray(cert.Q, float), Psi3=Psi, Gam=Gm, zeta=zeta,
                           xi=np.asarray(cert.xi, float), Xbar=np.asarray(cert.Xbar, float), bound=cert.bound), df


def evaluate_shor(A, mask, gamma, rows, st, cert, want_terms=False):
    """Steps 2-8 of shor_dual_bound for the multipliers as they are (no sanitising).  The blocks need not be PSD: the shift of step 2 covers
    what is left of their negative part after the spread, so the value is a valid bound for any symmetric Gam; zeta, lam and Psi3 are taken
    as admissible.  want_terms: (value, terms) with terms = (constant, min(eig_0(M), 0), ||c||, min_j mu_j) in the scaled variables, so that
    value * scale^2 = constant + second - third (omc_shor_dual_bound_batch reports the same four); entries not reached before a -inf are nan."""
    terms = [np.nan] * 4

    def out(v):
        return (v, tuple(terms)) if want_terms else v

    A = np.asarray(A, float); mask = np.asarray(mask, bool)
    n, m = A.shape
    sc = float(cert.scale)
    if not (np.isfinite(sc) and sc > 0.0):
        return out(-np.inf)
    Q = np.asarray(cert.Q, float); Psi = np.asarray(cert.Psi3, float); lam = np.asarray(cert.lam, float)
    r = Q.shape[1]
    if len(lam) != len(rows):
        raise ValueError(f"lam holds {len(lam)} multipliers, the node has {len(rows)} rows")
    if Psi.shape != (r + 1, r + 1):
        raise ValueError(f"Psi3 must be of order r + 1 = {r + 1}")
    Ah = A * sc
    inC, inS, ctype = st.inC, st.inS, st.ctype
    t0 = (ctype == 0)[None, :]; t1 = (ctype == 1)[None, :]; t01 = (ctype != 2)[None, :]
    qX = np.where(mask & inS & t0, 1.0, 0.0)
    cX = np.where(mask, -Ah, 0.0)
    cW = np.where(mask & inC, 0.5, 0.0) - np.where(inC & t1, 0.5, 0.0)
    cT = 1.0 / (2.0 * gamma) + np.where(ctype == 1, 0.5, 0.0)
    const = 0.5 * float((Ah[mask] ** 2).sum())
    # 2. spread and shift
    gdiag = np.zeros((n, m)); g0 = np.zeros((n, m))
    if st.nq:
        Gm = np.asarray(cert.Gam, float).reshape(-1, 5, 5)
        Gm = 0.5 * (Gm + np.transpose(Gm, (0, 2, 1)))
        e1, e2, e3 = _v_residuals(st, Gm)
        E = np.zeros_like(Gm)
        E[:, 1, 2] = E[:, 2, 1] = e1[st.k12]; E[:, 3, 4] = E[:, 4, 3] = e1[st.k34]
        E[:, 1, 3] = E[:, 3, 1] = e2[st.k13]; E[:, 2, 4] = E[:, 4, 2] = e2[st.k24]
        E[:, 1, 4] = E[:, 4, 1] = e3; E[:, 2, 3] = E[:, 3, 2] = e3
        shift = np.sqrt((E * E).sum((1, 2)))
        Gm = Gm - E + shift[:, None, None] * np.eye(5)[None]
        if not np.isfinite(Gm).all():
            return out(-np.inf)
        low = np.linalg.eigvalsh(Gm)[:, 0]                      # 0 for a PSD input: ||E||_F exceeds the spectral norm of the trace-free E
        Gm = Gm + np.maximum(-low, 0.0)[:, None, None] * np.eye(5)[None]
        const -= float(Gm[:, 0, 0].sum())                       # the block's (0,0) entry multiplies the constant 1
        np.add.at(g0, (st.ci, st.cj), Gm[:, 0, 1:5])
        np.add.at(gdiag, (st.ci, st.cj), Gm[:, [1, 2, 3, 4], [1, 2, 3, 4]])
    # 3. zeta
    zmin = np.where(inC, gdiag - cW, -np.inf).max(0)
    zadm = np.asarray(cert.zeta, float)
    zeta = np.where(ctype == 2, zmin, np.maximum(zadm, zmin))
    # 4. mu
    mu = cT - zeta
    terms[3] = float(np.min(mu))
    # 5. phi and M
    xi = np.where(inS & t01, np.asarray(cert.xi, float), 0.0)
    Xbar = np.asarray(cert.Xbar, float)
    const -= float((zeta * (xi * xi).sum(0)).sum())
    phi = 0.5 * (cX + qX * Xbar) + zeta[None, :] * xi - g0
    const -= 0.5 * float((qX * Xbar * Xbar).sum())
    bad = ~(mu > 0.0)
    if bad.any():
        if not np.isfinite(phi[:, bad]).all() or np.abs(phi[:, bad]).max() > 0.0:
            return out(-np.inf)
        mu = np.where(bad, 1.0, mu)
    M = -(phi / mu[None, :]) @ phi.T
    # 6. rows and the small cone
    cU = np.zeros((n, 1))
    for (kind, x, CU, rhs), lv in zip(rows, lam):
        if kind == "trace" or lv == 0.0:
            continue
        if kind == "cut":
            M += lv * np.outer(x, x)
        cU += lv * CU
        const -= lv * rhs
    M -= Q @ Psi[:r, :r] @ Q.T
    cV = Q.T @ cU - 2.0 * Psi[:r, r:]
    const -= float(np.trace(Psi[r:, r:]))
    # 7. the minimum over the simple set
    if not np.isfinite(M).all():
        return out(-np.inf)
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    terms[0] = const; terms[1] = float(min(ev[0], 0.0)); terms[2] = float(np.linalg.norm(cV, axis=0).sum())
    val = terms[0] + terms[1] - terms[2]
    # 8. back to the node's own scale
    return out(val / (sc * sc) if np.isfinite(val) else -np.inf)


def shor_dual_bound(A, mask, gamma, node, cut_type, shor_idx, soc_idx, cert, U_lower=None, U_upper=None, q1=True, want_defects=False):
    """A valid lower bound on the optimum of the node's Shor-mode relaxation (rank 1) from `cert`, whatever produced it: sanitise, then the
    steps of the comment above.  The blocks are made admissible in two ways and the better bound is returned (the larger of two valid lower
    bounds is one): by their PSD part before the spread, and as given (symmetrised), with the shift of step 2 paying for what is left of
    their negative part after it.  The first is the tighter one for blocks that are far from PSD; the second changes nothing in blocks that
    are PSD up to rounding, where the PSD part moves every one of them by its rounding.  want_defects: also the defects of the multipliers
    as given (sanitise_shor)."""
    A = np.asarray(A, float)
    n, m = A.shape
    st = shor_structure(n, m, mask, shor_idx, soc_idx)
    rows = node_rows(n, 1, node, cut_type, U_lower, U_upper, q1)
    clean, df = sanitise_shor(cert, st)
    val = evaluate_shor(A, mask, gamma, rows, st, clean)
    if st.nq:
        Gam = np.asarray(cert.Gam, float).reshape(-1, 5, 5)
        val = max(val, evaluate_shor(A, mask, gamma, rows, st, replace(clean, Gam=0.5 * (Gam + np.transpose(Gam, (0, 2, 1))))))
    return (val, df) if want_defects else val


def shor_plan(n, m, k, nq_stride, max_cuts=0, nonstandard_box_rows=0):
    """The strides of omc_shor_certificate_plan computed in Python (doubles), bytes per node of the arena and per slot, rmax."""
    Rmax = 1 + k * (k + 1) // 2 + nonstandard_box_rows + max_cuts * (2 * k + 1)
    rmax = max(1, min(n, k + nonstandard_box_rows + max_cuts))
    psi = (rmax + k) ** 2
    per = 15 * nq_stride + m + 2 * n * m + Rmax + psi
    return dict(lam=Rmax, Q=n * rmax, Psi3=psi, Gam=15 * nq_stride, zeta=m, xi=n * m, Xbar=n * m, bytes_per_node=8 * (1 + per) + 8,
                bytes_per_slot=8 * (2 + per) + 8, rmax=rmax)
