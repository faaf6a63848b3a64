"""References for one V-step and one U-step of alternating_minimization (OMC.jl:2192-2232), independent of the algorithm the kernels and
omc_oracle.py share.  numpy and scipy only; the product path never imports this module.

  * v_step_ref: the normal equations of every column in long double, solved by elimination with pivoting on the diagonal (the matrices are
    positive semidefinite, so the largest entry of every Schur complement is on its diagonal: this is complete pivoting).  A pivot at the
    rounding level of the long-double arithmetic ends the elimination: the remaining components are 0, which is a minimiser because the
    right-hand side lies in the range of the matrix.  With every column come the float64 condition number and e_ref, the largest error,
    against the long-double solution, of np.linalg.solve and of float64 restatements of the kernels' unpivoted Gauss-Jordan inverse that
    differ in how the normal equations are added up (numpy; entry after entry; the opposite order; entry after entry with fused
    multiply-adds, the device compiler's contraction).
  * u_step_ref: model_U is a convex QP with convex quadratic constraints, so a point with multipliers that satisfy the KKT conditions is
    its minimiser.  From any approximate solution the multipliers (mu, theta) >= 0 are recovered by non-negative least squares on the
    stationarity system; U_ref is then the row-wise minimiser of the Lagrangian in long double, (H_i + S(theta)) u_i = g_i - (C' mu)_i,
    and up to two Newton steps on the active constraints' values take the multipliers from the seed's accuracy to the rounding level.
    Stationarity holds by construction; what certifies U_ref is its feasibility and complementarity, which are returned with it.
  * first_order_stop_term: how far the kernels' stop rules allow U to be from the minimiser, to first order, from the reference's own
    derivatives dU/dtheta.
  * objectives_ref: model_U's objective and evaluate_objective(U V) in long double with the error of their float64 restatements."""
import math

import numpy as np

import omc_oracle as orc

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "omc_altmin_ref needs an 80-bit or wider long double (eps = %g here)" % float(np.finfo(LD).eps)
U_RND = 1.1e-16
NEWTON_TOL = 1e-12        # the dual Newton loop of k_altmin_k / k_altmin_w ends at max_c |min(theta_c, -q_c)| <= 1e-12
BISECT_WIDTH = 1e-15      # k_altmin ends the bisection of the ball multiplier at width 1e-15 max(1, theta)
NNQP_TOL = 1e-13          # wave_nnqp ends when no row outside the passive set is violated by more than 1e-13 max |C u0 - d|
NEAR_ACTIVE = 1e-7        # slack below which a constraint of the seed may carry a multiplier (the seed is good to ~1e-12)
ACTIVE_REL = 1e-8        # a constraint counts as active if its multiplier exceeds this fraction of the largest


# ---- V-step -----------------------------------------------------------------------------------------------------------------------------
def solve_psd_ld(M, b):
    """A minimiser of 1/2 v'Mv - b'v for symmetric positive semidefinite M (long double) with b in its range; returns (v, rank)."""
    k = M.shape[0]
    A = np.array(M, LD); r = np.array(b, LD)
    perm = list(range(k))
    top = max(float(np.max(np.diag(A))), 0.0)
    rank = 0
    for p in range(k):
        q = p + int(np.argmax(np.diag(A)[p:]))
        if not (A[q, q] > LD(64 * k) * np.finfo(LD).eps * LD(top)) or top == 0.0:
            break
        if q != p:
            A[[p, q], :] = A[[q, p], :]; A[:, [p, q]] = A[:, [q, p]]; r[[p, q]] = r[[q, p]]; perm[p], perm[q] = perm[q], perm[p]
        for i in range(p + 1, k):
            f = A[i, p] / A[p, p]
            A[i, p:] -= f * A[p, p:]; r[i] -= f * r[p]
        rank += 1
    x = np.zeros(k, LD)
    for p in range(rank - 1, -1, -1):
        x[p] = (r[p] - A[p, p + 1:rank] @ x[p + 1:rank]) / A[p, p]
    v = np.zeros(k, LD)
    v[perm] = x
    return v, rank


def _fma(a, b, c):
    """a b + c with one rounding to float64, as a fused multiply-add gives it (the product is formed in long double: 64 of its 106 bits,
    so a result can differ from the true fused one where the double rounding matters, which is rare)"""
    return np.asarray(np.asarray(a, LD) * np.asarray(b, LD) + np.asarray(c, LD), np.float64)


def gauss_jordan_restated(M, b, fused=False):
    """float64 restatement of ak_inv / aw_inv8 followed by the product with the right-hand side: in-place unpivoted Gauss-Jordan inverse.
    fused: every a - f b and every step of the final dot products is one fused multiply-add, as the device compiler contracts them."""
    a = np.array(M, np.float64); k = a.shape[0]
    b = np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        for p in range(k):
            d = 1.0 / a[p, p]
            a[p, p] = 1.0
            a[p, :] *= d
            for r in range(k):
                if r == p:
                    continue
                f = a[r, p]; a[r, p] = 0.0
                a[r, :] = _fma(-f, a[p, :], a[r, :]) if fused else a[r, :] - f * a[p, :]
        if not fused:
            return a @ b
        acc = np.zeros(k)
        for c in range(k):
            acc = _fma(a[:, c], b[c], acc)
        return acc


def v_step_ref(A, mask, gamma, U):
    """model_V per column in long double.  Returns dict(V (k, m) long double, rank (m,), cond (m,), e_ref (m,))."""
    A = np.asarray(A, np.float64); mask = np.asarray(mask, bool); U = np.asarray(U, np.float64)
    n, k = U.shape; m = A.shape[1]
    Ul = np.asarray(U, LD)
    UtU = (Ul.T @ Ul) / LD(gamma); UtU64 = U.T @ U / gamma
    V = np.zeros((k, m), LD); rank = np.zeros(m, int); cond = np.zeros(m); e_ref = np.zeros(m)
    for j in range(m):
        o = np.flatnonzero(mask[:, j])
        Uo = Ul[o, :]
        M = Uo.T @ Uo + UtU
        b = Uo.T @ np.asarray(A[o, j], LD)
        V[:, j], rank[j] = solve_psd_ld(M, b)
        M64 = U[o, :].T @ U[o, :] + UtU64; b64 = U[o, :].T @ A[o, j]
        # the same sums one entry after the other, as a thread of the kernels forms them, and in the opposite order: which order a
        # correct implementation takes is its own business, so the restatement's error is the largest over these three
        outer = U[o, :, None] * U[o, None, :]; prod = U[o, :] * A[o, j][:, None]
        forms = [(M64, b64)]
        for sl in (slice(None), slice(None, None, -1)):
            forms.append((np.cumsum(np.concatenate([UtU64[None], outer[sl]]), axis=0)[-1],
                          np.cumsum(np.concatenate([np.zeros((1, k)), prod[sl]]), axis=0)[-1]))
        Mf, bf = UtU64.copy(), np.zeros(k)             # ... and in order with fused multiply-adds
        for i in o:
            Mf = _fma(U[i, :, None], U[i, None, :], Mf); bf = _fma(U[i, :], A[i, j], bf)
        err = lambda x: float(np.sqrt(((np.asarray(x, LD) - V[:, j]) ** 2).sum()))
        with np.errstate(all="ignore"):
            cond[j] = np.linalg.cond(M64) if np.isfinite(M64).all() and M64.any() else np.inf
            if rank[j] == k:
                es = [err(gauss_jordan_restated(Mq, bq)) for Mq, bq in forms] + [err(gauss_jordan_restated(Mf, bf, fused=True))]
                if k == 1:                 # k_altmin divides: num / den
                    es += [err(bq / Mq[0]) for Mq, bq in forms + [(Mf, bf)]]
                try:
                    es.append(err(np.linalg.solve(M64, b64)))
                except np.linalg.LinAlgError:
                    es.append(np.inf)
                e_ref[j] = max(es)
            else:
                e_ref[j] = np.nan
    return dict(V=V, rank=rank, cond=cond, e_ref=e_ref)


# ---- U-step -----------------------------------------------------------------------------------------------------------------------------
def ustep_data(inst, V, cuts=(), cut_type="linear"):
    """model_U's data: H (n, k, k), g (n, k) in long double; C (R, n k) and d (R,), the rows omc_altmin_batch builds (symmetry breaking, then
    per cut and column the two bounds); kinds (R,) 'sym' | 'cut'; W (k^2, k), rad (k^2,) of quadratic_constraint_vectors."""
    n, k = inst.n, inst.k
    Vl = np.asarray(V, LD)
    VVt = (Vl @ Vl.T) / LD(inst.gamma)
    H = np.zeros((n, k, k), LD); g = np.zeros((n, k), LD)
    for i in range(n):
        o = np.flatnonzero(inst.indices[i, :])
        Vo = Vl[:, o]
        H[i] = Vo @ Vo.T + VVt
        g[i] = Vo @ np.asarray(inst.A[i, o], LD)
    rows = orc.build_rows(inst, cuts, cut_type)
    sel = [r for r in range(len(rows)) if rows.kinds[r] in ("box_lo", "box_hi", "hi", "lo")]
    C = np.array([rows.CU[r].ravel() for r in sel]).reshape(len(sel), n * k)
    d = np.array([rows.rhs[r] for r in sel])
    kinds = np.array(["sym" if rows.kinds[r].startswith("box") else "cut" for r in sel])
    W, rad = orc.quadratic_constraint_vectors(k)
    return dict(H=H, g=g, C=C, d=d, kinds=kinds, W=W, rad=rad)


def _lagrangian_minimiser(D, mu, theta):
    H, g, C, W = D["H"], D["g"], D["C"], D["W"]
    n, k = g.shape
    S = np.zeros((k, k), LD)
    for c in range(len(theta)):
        S += LD(2.0) * LD(theta[c]) * np.outer(np.asarray(W[c], LD), np.asarray(W[c], LD))
    rhs = g - (np.asarray(C, LD).T @ np.asarray(mu, LD)).reshape(n, k) if len(mu) else g.copy()
    U = np.zeros((n, k), LD)
    for i in range(n):
        U[i], _ = solve_psd_ld(H[i] + S, rhs[i])
    return U


def _multipliers(D, U):
    """(mu, theta) >= 0 closest, in least squares, to stationarity at U; the columns are scaled to unit norm for scipy's nnls.  Only
    constraints within NEAR_ACTIVE of their bound at U may carry a multiplier: where the active gradients are linearly dependent (n = k:
    a whole triangle of sign rows), nnls would otherwise be free to express stationarity through a constraint that has slack."""
    from scipy.optimize import nnls
    H, g, C, d, W, rad = D["H"], D["g"], D["C"], D["d"], D["W"], D["rad"]
    n, k = g.shape
    Ul = np.asarray(U, LD)
    b = np.asarray((g - np.einsum("iab,ib->ia", H, Ul)).ravel(), np.float64)
    rowv = np.asarray(np.asarray(C, LD) @ Ul.ravel() - np.asarray(d, LD), np.float64) if len(d) else np.zeros(0)
    q = np.asarray(((Ul @ np.asarray(W, LD).T) ** 2).sum(0) - np.asarray(rad, LD), np.float64)
    ra = np.flatnonzero(rowv >= -NEAR_ACTIVE); qa = np.flatnonzero(q >= -NEAR_ACTIVE)
    mu = np.zeros(C.shape[0]); theta = np.zeros(len(W))
    if len(ra) + len(qa) == 0:
        return mu, theta
    cols = [C[r] for r in ra] + [np.asarray(2.0 * (Ul @ np.outer(W[c], W[c])), np.float64).ravel() for c in qa]
    M = np.array(cols).T
    nrm = np.sqrt((M * M).sum(0)); nrm[nrm == 0.0] = 1.0
    x, _ = nnls(M / nrm, b, maxiter=50 * M.shape[1])
    x = x / nrm
    mu[ra] = x[:len(ra)]; theta[qa] = x[len(ra):]
    return mu, theta


def _polish(D, U, mu, theta):
    """One Newton step on the active constraints' values F = (C_A u - d_A, q_a) as functions of their multipliers z = (mu_A, theta_a), with
    u = K(theta)^-1 (g - C_A' mu_A): dF/dz = -N K^-1 N' for the rows N = [C_A; B_a], B_c = vec(2 U w_c w_c').  The matrix is formed in float64
    (a Newton step tolerates that), F and the new point in long double.  nnls leaves the multipliers at the seed's accuracy; this takes
    the constraint values of the reference to the rounding level."""
    H, C, d, W, rad = D["H"], D["C"], D["d"], D["W"], D["rad"]
    n, k = U.shape
    top = max([float(x) for x in mu] + [float(x) for x in theta] + [0.0])
    ra = np.flatnonzero(np.asarray(mu, np.float64) > ACTIVE_REL * top); qa = np.flatnonzero(np.asarray(theta, np.float64) > ACTIVE_REL * top)
    if top == 0.0 or len(ra) + len(qa) == 0:
        return mu, theta, U
    U64 = np.asarray(U, np.float64)
    S = 2.0 * np.einsum("c,ca,cb->ab", np.asarray(theta, np.float64), W, W)
    Kinv = np.linalg.inv(np.asarray(H, np.float64) + S[None])
    N = np.array([C[r] for r in ra] + [(2.0 * U64 @ np.outer(W[c], W[c])).ravel() for c in qa]).reshape(len(ra) + len(qa), n, k)
    KN = np.einsum("iab,rib->ria", Kinv, N)
    Jm = np.einsum("ria,sia->rs", N, KN)
    Ul = np.asarray(U, LD)
    F = np.concatenate([np.asarray(C[ra], LD) @ Ul.ravel() - np.asarray(d[ra], LD),
                        ((Ul @ np.asarray(W[qa], LD).T) ** 2).sum(0) - np.asarray(rad[qa], LD)])
    dz = np.linalg.lstsq(Jm, np.asarray(F, np.float64), rcond=None)[0]
    mu0, theta0 = mu, theta
    mu = np.zeros(len(mu0), LD); theta = np.zeros(len(theta0), LD)       # multipliers below the activity threshold are dropped
    mu[ra] = mu0[ra]; theta[qa] = theta0[qa]
    mu[ra] =np.maximum(mu[ra] + np.asarray(dz[:len(ra)], LD), 0); theta[qa] = np.maximum(theta[qa] + np.asarray(dz[len(ra):], LD), 0)
    return mu, theta, _lagrangian_minimiser(D, mu, theta)


def certificate(D, U, mu, theta):
    """KKT quantities of (U, mu, theta) for model_U, evaluated in long double."""
    H, g, C, d, W, rad = D["H"], D["g"], D["C"], D["d"], D["W"], D["rad"]
    n, k = g.shape
    Ul = np.asarray(U, LD)
    S = sum((LD(2.0) * LD(theta[c]) * np.outer(np.asarray(W[c], LD), np.asarray(W[c], LD)) for c in range(len(theta))), np.zeros((k, k), LD))
    grad = np.einsum("iab,ib->ia", H, Ul) - g + Ul @ S
    if len(mu):
        grad = grad + (np.asarray(C, LD).T @ np.asarray(mu, LD)).reshape(n, k)
    rowv = np.asarray(C, LD) @ Ul.ravel() - np.asarray(d, LD) if len(d) else np.zeros(0, LD)
    q = ((Ul @ np.asarray(W, LD).T) ** 2).sum(0) - np.asarray(rad, LD)
    gn = float(np.sqrt((g * g).sum()))
    top = max([float(x) for x in mu] + [float(x) for x in theta] + [0.0])
    return dict(stationarity=float(np.sqrt((grad * grad).sum())) / max(gn, 1e-300),
                row_violation=max(float(rowv.max()) if len(rowv) else 0.0, 0.0), quad_violation=max(float(q.max()), 0.0),
                complementarity=float(np.abs(np.asarray(mu, LD) * rowv).sum() + np.abs(np.asarray(theta, LD) * q).sum()),
                rowv=np.asarray(rowv, np.float64), q=np.asarray(q, np.float64),
                active_rows=np.asarray(mu) > ACTIVE_REL * top if top > 0 else np.zeros(len(mu), bool),
                active_quad=np.asarray(theta) > ACTIVE_REL * top if top > 0 else np.zeros(len(theta), bool))


def u_step_ref(inst, V, cuts=(), cut_type="linear", seed=None):
    """model_U for the factor V.  seed: any approximate solution (default: the oracle's altmin_u_step, on the CPU).  Returns dict(U long
    double, mu, theta, data, seed, seed_info, and the certificate's entries)."""
    D = ustep_data(inst, V, cuts, cut_type)
    info = {}
    if seed is None:
        seed, _, info = orc.altmin_u_step(inst, np.asarray(V, np.float64), cuts, cut_type)
    U = np.asarray(seed, LD)
    for _ in range(2):                    # multipliers from the seed, then once more from the reference itself
        mu, theta = _multipliers(D, U)
        U = _lagrangian_minimiser(D, mu, theta)
    mu, theta = np.asarray(mu, LD), np.asarray(theta, LD)
    worst = lambda c: max(c["row_violation"], c["quad_violation"], c["complementarity"])
    out = certificate(D, U, mu, theta)
    for _ in range(2):                    # a Newton step is kept only if the certificate improves (degenerate active sets may not)
        mu2, theta2, U2 = _polish(D, U, mu, theta)
        out2 = certificate(D, U2, mu2, theta2)
        if not worst(out2) < worst(out):
            break
        mu, theta, U, out = mu2, theta2, U2, out2
    out.update(U=U, mu=mu, theta=theta, data=D, seed=np.asarray(seed, np.float64), seed_info=info)
    return out


def first_order_stop_term(ref):
    """Bound, to first order, on ||U - U_ref||_F for a U-step that ends by the kernels' stop rule instead of at the minimiser.

    For fixed multipliers theta of the quadratic constraints and the active rows C_A of the reference, U(theta) = P K^-1 g with
    K = blockdiag(H_i + S(theta)) and P K^-1 = K^-1 - K^-1 C_A' (C_A K^-1 C_A')^-1 C_A K^-1, so D_c = dU/dtheta_c = -P K^-1 b_c with
    b_c = vec(2 U w_c w_c') (without rows: -(H_i + S)^-1 2 w_c w_c' u_i), and dq/dtheta = J = B' D.  The Newton loop ends with
    |q_a| <= 1e-12 on the active constraints a and theta_i <= 1e-12 on the others, hence
        ||dtheta_a|| <= ||J_aa^-1|| (sqrt(n_a) + ||J_ai|| sqrt(n_i)) 1e-12,   ||dU||_F <= ||D_a|| ||dtheta_a|| + ||D_i|| sqrt(n_i) 1e-12.
    At k = 1 the ball multiplier is bisected to a width of 1e-15 max(1, theta): ||dU|| <= ||D|| 1e-15 max(1, theta).  An active set on
    which J_aa is singular gives inf (nothing is promised there).  The rows have a stop rule of their own (see term_rows below), which
    is the whole term where no quadratic constraint is active."""
    D = ref["data"]
    H, W = np.asarray(D["H"], np.float64), D["W"]
    n, k = ref["U"].shape
    U = np.asarray(ref["U"], np.float64); theta = np.asarray(ref["theta"], np.float64); act = np.asarray(ref["active_quad"], bool)
    S = 2.0 * np.einsum("c,ca,cb->ab", theta, W, W)
    Kinv = np.linalg.inv(H + S[None])                                  # (n, k, k)
    CA = D["C"][np.asarray(ref["active_rows"], bool)].reshape(-1, n, k)

    def apply_PKinv(b):
        y = np.einsum("iab,ib->ia", Kinv, b)
        if len(CA):
            T = np.einsum("ria,iab->rib", CA, Kinv)
            G = np.einsum("rib,sib->rs", T, CA)
            lam = np.linalg.lstsq(G, np.einsum("ria,ia->r", CA, y), rcond=None)[0]
            y = y - np.einsum("r,rib->ib", lam, T)
        return y

    Bm = np.array([(2.0 * U @ np.outer(W[c], W[c])).ravel() for c in range(len(W))]).T          # (n k, k^2)
    Dm = np.array([-apply_PKinv(Bm[:, c].reshape(n, k)).ravel() for c in range(len(W))]).T
    ia = np.flatnonzero(act); ii = np.flatnonzero(~act)
    nD = lambda idx: float(np.linalg.norm(Dm[:, idx], 2)) if len(idx) else 0.0
    # the rows: wave_nnqp (and the oracle's nnqp) stop when no row outside the passive set is violated by more than 1e-13 max |C u0 - d|,
    # u0 = K^-1 g.  Taking such a row r in moves U by its violation times K^-1 C_r' / (C_r K^-1 C_r')
    term_rows = 0.0
    Call = D["C"].reshape(-1, n, k)
    if len(Call):
        u0 = np.einsum("iab,ib->ia", Kinv, np.asarray(D["g"], np.float64))
        cmax = float(np.abs(np.einsum("ria,ia->r", Call, u0) - D["d"]).max())
        KC = np.einsum("iab,rib->ria", Kinv, Call)
        den = np.einsum("ria,ria->r", Call, KC); num = np.sqrt(np.einsum("ria,ria->r", KC, KC))
        rest = ~np.asarray(ref["active_rows"], bool)
        if rest.any():
            term_rows = NNQP_TOL * cmax * math.sqrt(rest.sum()) * float((num[rest] / den[rest]).max())
    if k == 1:
        return term_rows + (nD(np.arange(1)) * BISECT_WIDTH * max(1.0, float(theta[0])) if act[0] else 0.0)
    term = term_rows + nD(ii) * math.sqrt(len(ii)) * NEWTON_TOL
    if len(ia):
        J = Bm.T @ Dm
        Jaa = J[np.ix_(ia, ia)]
        sv = np.linalg.svd(Jaa, compute_uv=False)
        if not (sv[-1] > 1e-12 * sv[0]):
            return math.inf
        Jai = float(np.linalg.norm(J[np.ix_(ia, ii)], 2)) if len(ii) else 0.0
        term += nD(ia) * (math.sqrt(len(ia)) + Jai * math.sqrt(len(ii))) * NEWTON_TOL / float(sv[-1])
    return term


# ---- objectives -------------------------------------------------------------------------------------------------------------------------
def objectives_ref(inst, U, V):
    """Long-double values at the float64 factors (U, V) of model_U's objective, 1/2 sum_i u_i'H_i u_i - g_i'u_i + 1/2 sum_Omega A^2, and of the
    master objective evaluate_objective(U V); with each e_ref, the largest error of its float64 restatements (below), not taken below one
    rounding of the result."""
    D = ustep_data(inst, V)
    Ul = np.asarray(U, LD); Vl = np.asarray(V, LD)
    HU = np.einsum("iab,ib->ia", D["H"], Ul)
    sumA2 = (np.asarray(inst.A[inst.indices], LD) ** 2).sum()
    mu_ld = LD(0.5) * (Ul * HU).sum() - (D["g"] * Ul).sum() + LD(0.5) * sumA2
    H64, g64, const = orc._ustep_quadratic(inst, np.asarray(V, np.float64))
    U64 = np.asarray(U, np.float64); V64 = np.asarray(V, np.float64)
    # float64 restatements of model_U's value.  H_i and g_i as numpy forms them and one entry after the other (a thread of the kernels);
    # the row terms u_i'(H_i u_i / 2 - g_i) added pairwise, in order and in the opposite order; the oracle's einsum; the residual form.
    # They are all correct implementations; which order one takes is its own business, so e_ref is the largest of their errors.
    n, k = U64.shape
    VVt = V64 @ V64.T / inst.gamma
    Hs = np.zeros_like(H64); gs = np.zeros_like(g64)
    for i in range(n):
        o = np.flatnonzero(inst.indices[i, :]); Vo = V64[:, o].T
        Hs[i] = np.cumsum(np.concatenate([VVt[None], Vo[:, :, None] * Vo[:, None, :]]), axis=0)[-1]
        gs[i] = np.cumsum(np.concatenate([np.zeros((1, k)), Vo * inst.A[i, o][:, None]]), axis=0)[-1]
    mu_64 = [0.5 * float(np.einsum("ia,iab,ib->", U64, H64, U64)) - float((g64 * U64).sum()) + const, orc.altmin_objective(inst, U64, V64)]
    # 1/2 sum A^2 likewise: numpy's pairwise sum (const), and one entry after the other down the columns, as the library's host code adds it
    const_seq = 0.5 * float(np.cumsum(inst.A.T[inst.indices.T] ** 2)[-1])
    for Hf, gf, cf in ((H64, g64, const), (Hs, gs, const_seq)):
        t = np.array([float(U64[i] @ (0.5 * (Hf[i] @ U64[i]) - gf[i])) for i in range(n)])
        mu_64 += [float(t.sum()) + cf, float(np.cumsum(t)[-1]) + cf, float(np.cumsum(t[::-1])[-1]) + cf]
    X = Ul @ Vl
    Rs = (X - np.asarray(inst.A, LD))[inst.indices]
    ma_ld = LD(0.5) * (Rs * Rs).sum() + (X * X).sum() / (LD(2.0) * LD(inst.gamma))
    # ... and of the master objective: omc_oracle's on the product, and the kernels' from the factors, fit / 2 + tr((U'U)(V V')) / (2 gamma),
    # the squared residuals added pairwise, in order and in the opposite order
    X64 = U64 @ V64
    sq = ((X64 - inst.A)[inst.indices]) ** 2
    reg = float(((U64.T @ U64) * (V64 @ V64.T)).sum()) / (2.0 * inst.gamma)
    ma_64 = [orc.evaluate_objective(X64, inst.A, inst.indices, inst.gamma)] + [0.5 * f + reg for f in (float(sq.sum()), float(np.cumsum(sq)[-1]),
                                                                                                       float(np.cumsum(sq[::-1])[-1]))]
    # Neither e_ref is taken below the rounding of the result itself: model_U's value is returned as q + 1/2 sum A^2, two float64 numbers of
    # magnitude |q| and 1/2 sum A^2 that cancel in part, so one unit is u (|u'Hu| / 2 + |g'u| + 1/2 sum A^2); the master's terms are all
    # non-negative, so u times the value.  (Restatements that all happen to round correctly would otherwise ask for less than half an ulp.)
    floor_u = U_RND * float(LD(0.5) * np.abs((Ul * HU).sum()) + np.abs((D["g"] * Ul).sum()) + LD(0.5) * sumA2)
    return dict(model_U=float(mu_ld), model_U_e_ref=max([abs(float(LD(x) - mu_ld)) for x in mu_64] + [floor_u]),
                master=float(ma_ld), master_e_ref=max([abs(float(LD(x) - ma_ld)) for x in ma_64] + [U_RND * float(ma_ld)]))
