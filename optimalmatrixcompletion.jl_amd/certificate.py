"""Independent check of a node's dual certificate: numpy only, no GPU, no library call.

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

from dataclasses import dataclass

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
