"""State of the Shor-mode relaxation after t iterations, and a measure of the reference's own error  --  TEST INFRASTRUCTURE ONLY.

The reference is oracle/omc_oracle_shor.py (float64, the same splitting from the same start as csrc/omc_shor_relax.hip):
sdp_relaxation_shor(..., max_iters = t) returns the whole state at iteration t.  What it lacks is e_ref, its own distance from the exact
state of the same map.  Two sources, the larger is taken:

  perturbation spread   the oracle on five seeded copies of the input whose A is perturbed entry by entry by 2^-52-level relative noise;
                        per array the largest distance to the unperturbed run.  Every step of the oracle is backward stable, so the spread
                        is the conditioning of the t-step map times the unit round-off.
  high precision        shor_state_mp: the same iteration restated at 50 digits with mpmath (mp.eigsy for every projection on a cone,
                        bisection to full precision for the paraboloid, the NNQP of the node's rows by enumeration of its active sets).
                        Used at the root (tests/test_shor_iter_cpu.py: case A, t <= 3).

Nothing here is imported by the product path."""
from __future__ import annotations

import itertools

import numpy as np

import omc_oracle as base
import omc_oracle_shor as sh

U_RND = 2.0 ** -53
ARRAYS = ("X", "W", "Theta", "Y", "U", "V1", "V2", "V3")
SCALARS = ("objective", "rp", "rd", "dual_bound")
N_COPIES = 5


def shor_params(t, **kw):
    return sh.ShorParams(eps_gap=1e-12, max_iters=int(t), **kw)


def shor_state(inst, minors, soc, cuts=(), t=1, **kw):
    """The oracle's state after t iterations: the arrays of ARRAYS (unscaled, as the engine returns them), the scalars of SCALARS (rp, rd in
    the scaled variables, as omc_debug_residuals gives them; dual_bound = the bound of the check at iteration t, not the running maximum),
    rho, iters, n_bumps, the structure and what the stop term of tests/test_shor_iter.py needs."""
    r = sh.sdp_relaxation_shor(inst, minors, soc, cuts=list(cuts), params=shor_params(t, **kw))
    out = {key: np.asarray(r[key], float) for key in ARRAYS}
    out.update(objective=float(r["objective"]), rp=float(r["rp"]), rd=float(r["rd"]), dual_bound=float(r["hist"][-1][2]), rho=float(r["rho"]),
               iters=int(r["iters"]), n_bumps=int(r["n_bumps"]), structure=r["structure"], rows=r["rows"], scale=float(r["scale"]),
               cone_inputs=r["cone_inputs"], check_iters=[h[0] for h in r["hist"]])
    return out


def perturbed_instance(inst, seed):
    rng = np.random.default_rng(1000 + seed)
    A = inst.A * (1.0 + 2.0 ** -52 * rng.uniform(-1.0, 1.0, inst.A.shape))
    return base.Instance(A, inst.indices, inst.gamma, inst.k)


def distance(a, b):
    """Frobenius distance of two arrays, |a - b| of two scalars; inf when exactly one side is not finite, 0 when both are the same infinity."""
    a = np.asarray(a, float); b = np.asarray(b, float)
    if a.shape != b.shape:
        return float("inf")
    fa, fb = np.isfinite(a), np.isfinite(b)
    if not (fa == fb).all():
        return float("inf")
    if not fa.all() and not np.array_equal(a[~fa], b[~fb]):
        return float("inf")
    d = np.where(fa, a, 0.0) - np.where(fb, b, 0.0)
    return float(np.sqrt((d * d).sum()))


def perturbation_spread(inst, minors, soc, cuts=(), t=1, ref=None, **kw):
    """{name: largest distance of the N_COPIES perturbed runs to the unperturbed one} over ARRAYS and SCALARS."""
    ref = ref or shor_state(inst, minors, soc, cuts, t, **kw)
    out = {key: 0.0 for key in ARRAYS + SCALARS}
    for c in range(N_COPIES):
        r = shor_state(perturbed_instance(inst, c), minors, soc, cuts, t, **kw)
        for key in out:
            out[key] = max(out[key], distance(r[key], ref[key]))
    return out


def representation_floor(ref):
    """u / 2 ||S||_F per array, u / 2 |s| per scalar: what rounding the exact state to float64 alone costs.  A spread below it says that the
    array does not depend on A at this iteration (Y after one iteration), not that the oracle is exact there."""
    out = {}
    for key in ARRAYS + SCALARS:
        v = np.asarray(ref[key], float)
        out[key] = 0.5 * U_RND * float(np.sqrt((np.where(np.isfinite(v), v, 0.0) ** 2).sum()))
    return out


def sensitivity(inst, minors, soc, cuts=(), t=1, key="dual_bound", ref=None, rel=1e-9, **kw):
    """Largest |change of a scalar| over the change of the scaled point (||dX|| sc + ||dTheta|| sc^2 + ||dW|| sc^2 + ||dY||) over five copies whose A
    carries `rel` relative noise: a first-order Lipschitz figure of the reference, for the stop term of a scalar that has no closed form."""
    ref = ref or shor_state(inst, minors, soc, cuts, t, **kw)
    sc = ref["scale"]; worst = 0.0
    for c in range(N_COPIES):
        rng = np.random.default_rng(2000 + c)
        A = inst.A * (1.0 + rel * rng.uniform(-1.0, 1.0, inst.A.shape))
        r = shor_state(base.Instance(A, inst.indices, inst.gamma, inst.k), minors, soc, cuts, t, **kw)
        den = (distance(r["X"], ref["X"]) * sc + (distance(r["Theta"], ref["Theta"]) + distance(r["W"], ref["W"])) * sc * sc + distance(r["Y"], ref["Y"]))
        num = distance(r[key], ref[key])
        if np.isfinite(num) and den > 0:
            worst = max(worst, num / den)
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------------
# the iteration at 50 digits (numpy object arrays of mpmath numbers; every input is converted exactly)
# ----------------------------------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    return mpmath


def _o(a):
    mp = _mp()
    a = np.asarray(a, float)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = mp.mpf(float(a[idx]))
    return out


def _z(*shape):
    mp = _mp()
    out = np.empty(shape, dtype=object)
    out.fill(mp.mpf(0))
    return out


def _eye(n):
    mp = _mp()
    out = _z(n, n)
    for i in range(n):
        out[i, i] = mp.mpf(1)
    return out


def _spectral(M, f):
    """f applied to the eigenvalues of the symmetric part of M."""
    mp = _mp()
    n = M.shape[0]
    if n == 0:
        return M.copy()
    S = (M + M.T) / mp.mpf(2)
    w, V = mp.eigsy(mp.matrix(S.tolist()))
    Vo = np.array(V.tolist(), dtype=object).reshape(n, n)
    wo = np.array([f(w[i]) for i in range(n)], dtype=object)
    return (Vo * wo[None, :]) @ Vo.T


def _fro2(M):
    mp = _mp()
    return sum((x * x for x in np.asarray(M, dtype=object).ravel()), mp.mpf(0))


def _paraboloid(xi, t):
    mp = _mp()
    s = sum((x * x for x in xi), mp.mpf(0))
    if t >= s:
        return xi, t, mp.mpf(0)
    lo = max(mp.mpf(0), -t); hi = max(mp.mpf(1), 2 * lo + 1)
    f = lambda nu: s / (1 + 2 * nu) ** 2 - t - nu
    while f(hi) > 0:
        hi *= 2
    for _ in range(4 * mp.mp.prec // 3 + 40):
        mid = (lo + hi) / 2
        if f(mid) > 0:
            lo = mid
        else:
            hi = mid
    nu = (lo + hi) / 2
    return np.array([x / (1 + 2 * nu) for x in xi], dtype=object), t + nu, nu


def _solve(G, c):
    mp = _mp()
    return np.array(list(mp.lu_solve(mp.matrix(G.tolist()), mp.matrix([[x] for x in c]))), dtype=object)


def _nnqp(G, c):
    """min 1/2 l'Gl - c'l, l >= 0, by enumeration of the active sets (R <= 6): the set whose solution is positive and whose
    complement has a non-positive gradient; among several (degenerate rows) the one of lowest value."""
    mp = _mp()
    R = len(c)
    if R > 6:
        raise ValueError("shor_state_mp enumerates active sets: at most 6 rows")
    best = None
    for size in range(R + 1):
        for P in itertools.combinations(range(R), size):
            lam = np.array([mp.mpf(0)] * R, dtype=object)
            if P:
                idx = list(P)
                try:
                    s = _solve(G[np.ix_(idx, idx)], c[idx])
                except ZeroDivisionError:
                    continue
                if min(s) <= 0:
                    continue
                lam[idx] = s
            w = c - G @ lam
            if all(w[r] <= mp.mpf(10) ** (-mp.mp.dps + 8) * max(1, max(abs(x) for x in c)) for r in range(R) if r not in P):
                val = (lam @ G @ lam) / 2 - c @ lam
                if best is None or val < best[0]:
                    best = (val, lam)
    return best[1]


def shor_state_mp(inst, minors, soc, t, digits=50, **kw):
    """sdp_relaxation_shor restated at `digits` digits: a node without cuts (trace row and the default box rows), rank 1.  Returns ARRAYS and
    objective, rp, rd as mpmath numbers in numpy object arrays.  The scale and the penalties are the oracle's float64 values, taken exactly:
    they are parameters of the map, not results of it."""
    mp = _mp()
    mp.mp.dps = digits
    p = shor_params(t, **kw)
    n, m, k, g = inst.n, inst.m, inst.k, inst.gamma
    assert k == 1
    N = n + m
    mask = inst.indices
    st = sh.ShorStructure(n, m, minors, soc, mask)
    nq = st.nq
    rows = base.build_rows(inst, (), "linear", None, None, p.reference_quirk_q1)
    R = len(rows)
    Qf = base.row_subspace(rows, n, k)
    r = Qf.shape[1]
    sc = mp.mpf(p.scale if p.scale > 0 else sh.shor_scale(inst))
    s2 = sc * sc
    F = lambda x: mp.mpf(float(x))
    Q = _o(Qf)
    Ah = _o(inst.A) * sc
    inC, inS, ctype = st.inC, st.inS, st.ctype
    t01 = ctype != 2
    one, zero, half = mp.mpf(1), mp.mpf(0), mp.mpf(1) / 2
    qX = _o(np.where(mask & inS & (ctype == 0)[None, :], 1.0, 0.0))
    cX = np.where(mask, -Ah, zero)
    cW = _o(np.where(mask & inC, 0.5, 0.0) - np.where(inC & (ctype == 1)[None, :], 0.5, 0.0))
    cT = np.array([one / (2 * F(g)) + (half if ctype[j] == 1 else zero) for j in range(m)], dtype=object)
    const0 = half * sum((Ah[i, j] ** 2 for i in range(n) for j in range(m) if mask[i, j]), zero)
    rho = F(p.rho); rx = F(p.relax); r5 = F(p.r5)
    r4 = F(p.r4 if p.r4 > 0 else min(40.0, max(0.25, 75.0 * n * m / (4.0 * max(nq, 1)))))
    wY = mp.mpf(3)
    cntC = _o(st.cntC); inSo = _o(inS.astype(float))
    wX = 2 + 2 * r4 * cntC + r5 * inSo
    wW = r4 * cntC
    iwW = _z(n, m)
    for i in range(n):
        for j in range(m):
            if inC[i, j]:
                iwW[i, j] = one / wW[i, j]
    siw = 1 + iwW.sum(0)
    AY = _z(R, n * n); AU = _z(R, n * k); b = _o(np.array(rows.rhs, float))
    for rr in range(R):
        if rows.kinds[rr] == "trace":
            AY[rr] = _eye(n).ravel()
        elif rows.kinds[rr] == "cut":
            raise ValueError("shor_state_mp: root nodes only")
        AU[rr] = _o(rows.CU[rr]).ravel()
    G1 = (AY / wY) @ AY.T + (AU / 2) @ AU.T
    Y = _eye(n) * (F(k) / n); X = _z(n, m); Th = _z(m, m); W = _z(n, m)
    V1 = _z(st.nv1); V2 = _z(st.nv2); V3 = _z(nq); Vt = _z(r, k)
    D0 = _z(N, N); D1 = _z(n, n); D3 = _z(n, n); D3V = _z(r, k); D3T = _z(k, k)
    Dq = _z(nq, 5, 5); D5x = _z(n, m); D5t = _z(m)
    Ik = _eye(k)
    pos = lambda x: max(x, zero)
    clip = lambda x: min(max(x, zero), one)

    def blocks(Xa, Wa, V1a, V2a, V3a):
        M = _z(nq, 5, 5)
        for q in range(nq):
            M[q, 0, 0] = one
            for pp in range(4):
                i, j = st.ci[q, pp], st.cj[q, pp]
                M[q, 0, pp + 1] = M[q, pp + 1, 0] = Xa[i, j]
                M[q, pp + 1, pp + 1] = Wa[i, j]
            M[q, 1, 2] = M[q, 2, 1] = V1a[st.k12[q]]; M[q, 3, 4] = M[q, 4, 3] = V1a[st.k34[q]]
            M[q, 1, 3] = M[q, 3, 1] = V2a[st.k13[q]]; M[q, 2, 4] = M[q, 4, 2] = V2a[st.k24[q]]
            M[q, 1, 4] = M[q, 4, 1] = M[q, 2, 3] = M[q, 3, 2] = V3a[q]
        return M

    rp = rd = zero
    n_bumps = 0; last_bump = 0
    for it in range(1, p.max_iters + 1):
        G = np.block([[Y, X], [X.T, Th]])
        P0 = _spectral(G - D0, pos)
        P1 = _spectral(Y - D1, clip)
        Min = Y - D3
        S_in = Q.T @ Min @ Q; V_in = Vt - D3V
        M3 = np.block([[S_in, V_in], [V_in.T, Ik - D3T]])
        M3s = (M3 + M3.T) / 2
        P3 = _spectral(M3, pos)
        Q3 = P3 - M3s
        dS = Q3[:r, :r]; W3V = P3[:r, r:]; W3T = P3[r:, r:]
        QdQ = Q @ dS @ Q.T
        if nq:
            Mq = blocks(X, W, V1, V2, V3)
            Inq = Mq - Dq
            Pq = _z(nq, 5, 5)
            for q in range(nq):
                Pq[q] = _spectral(Inq[q], pos)
        tcur = np.array([Th[j, j] for j in range(m)], dtype=object) - W.sum(0)
        P5x = _z(n, m); P5t = _z(m)
        for j in range(m):
            if ctype[j] == 2:
                continue
            Sj = np.flatnonzero(inS[:, j])
            xi, tt, _ = _paraboloid((X[:, j] - D5x[:, j])[Sj], tcur[j] - D5t[j])
            for a, i in enumerate(Sj):
                P5x[i, j] = xi[a]
            P5t[j] = tt
        T0 = rx * P0 + (1 - rx) * G + D0
        tY = (T0[:n, :n] + (rx * P1 + (1 - rx) * Y + D1) + (Y + (1 - rx) * D3 + rx * QdQ)) / wY
        T5x = np.where(inS, rx * P5x + (1 - rx) * X + D5x, zero)
        T5t = rx * P5t + (1 - rx) * tcur + D5t
        tX = 2 * T0[:n, n:] + r5 * T5x
        tW = _z(n, m)
        tTh = T0[n:, n:]
        if nq:
            Tq = rx * Pq + (1 - rx) * Mq + Dq
            s1 = _z(st.nv1); s2_ = _z(st.nv2)
            for q in range(nq):
                for pp in range(4):
                    i, j = st.ci[q, pp], st.cj[q, pp]
                    tX[i, j] = tX[i, j] + 2 * r4 * Tq[q, 0, pp + 1]
                    tW[i, j] = tW[i, j] + r4 * Tq[q, pp + 1, pp + 1]
                s1[st.k12[q]] += Tq[q, 1, 2]; s1[st.k34[q]] += Tq[q, 3, 4]
                s2_[st.k13[q]] += Tq[q, 1, 3]; s2_[st.k24[q]] += Tq[q, 2, 4]
            V1n = s1 / _o(st.cnt1); V2n = s2_ / _o(st.cnt2)
            V3n = np.array([(Tq[q, 1, 4] + Tq[q, 2, 3]) / 2 for q in range(nq)], dtype=object)
        else:
            V1n, V2n, V3n = V1, V2, V3
        Xn = (tX - cX / rho) / (wX + qX / rho)
        thbar = np.array([tTh[j, j] for j in range(m)], dtype=object) - cT / rho
        wbar = (tW * iwW) - np.where(inC, cW * iwW, zero) / rho
        base_ = thbar - wbar.sum(0)
        u = np.array([(base_[j] - T5t[j]) / (1 + r5 * siw[j]) if t01[j] else base_[j] / siw[j] for j in range(m)], dtype=object)
        cpl = np.array([r5 * u[j] if t01[j] else u[j] for j in range(m)], dtype=object)
        thn = thbar - cpl
        Wn = np.where(inC, wbar + cpl[None, :] * iwW, zero)
        Thn = (tTh + tTh.T) / 2
        for j in range(m):
            Thn[j, j] = thn[j]
        tV = rx * W3V + (1 - rx) * Vt + D3V
        tU = Q @ tV
        c = AY @ tY.ravel() + AU @ tU.ravel() - b
        mu = _nnqp(G1, c)
        Yn = tY - ((AY.T @ mu) / wY).reshape(n, n)
        Yn = (Yn + Yn.T) / 2
        Vn = tV - Q.T @ ((AU.T @ mu) / 2).reshape(n, k)
        Gn = np.block([[Yn, Xn], [Xn.T, Thn]])
        D0 = T0 - Gn
        D1 = D1 + rx * P1 + (1 - rx) * Y - Yn
        D3n = (1 - rx) * D3 + Y + rx * QdQ - Yn
        D3V = D3V + rx * W3V + (1 - rx) * Vt - Vn
        D3T = D3T + rx * (W3T - Ik)
        tnew = thn - Wn.sum(0)
        D5x = np.where(inS, T5x - Xn, zero)
        D5t = np.array([T5t[j] - tnew[j] if t01[j] else zero for j in range(m)], dtype=object)
        rp2 = (_fro2(P0 - Gn) + _fro2(P1 - Yn) + _fro2(Min + QdQ - Yn) + 2 * _fro2(W3V - Vn) + _fro2(W3T - Ik)
               + _fro2(np.where(inS, P5x - Xn, zero)) + _fro2([P5t[j] - tnew[j] for j in range(m) if t01[j]]))
        rd2 = _fro2(Gn - G) + 2 * _fro2(Vn - Vt) + _fro2(Wn - W)
        D3 = D3n
        if nq:
            Mqn = blocks(Xn, Wn, V1n, V2n, V3n)
            Dq = Tq - Mqn
            rp2 += _fro2(Pq - Mqn)
        rp = mp.sqrt(rp2); rd = mp.sqrt(rd2)
        Y, X, Th, W, V1, V2, V3, Vt = Yn, Xn, Thn, Wn, V1n, V2n, V3n, Vn
        if (it % p.check_every == 0 or it == p.max_iters) and it < p.max_iters:
            if (p.bump_max and it >= p.bump_after and n_bumps < p.bump_max and it - last_bump >= p.check_every * p.bump_window
                    and rp > F(p.bump_ratio) * rd):
                fac = F(p.bump_factor)
                rho = rho * fac
                D0 = D0 / fac; D1 = D1 / fac; D3 = D3 / fac; D3V = D3V / fac; D3T = D3T / fac; Dq = Dq / fac; D5x = D5x / fac; D5t = D5t / fac
                n_bumps += 1; last_bump = it
    obj_s = const0 + (cX * X).sum() + half * (qX * X * X).sum() + (cW * W).sum() + sum((cT[j] * Th[j, j] for j in range(m)), zero)
    Xo = X / sc; Tho = Th / s2; Wc = W / s2
    Wo = np.where(inC, Wc, np.where(inS, Xo * Xo, zero))
    for j in range(m):
        if ctype[j] == 2:
            continue
        e = Tho[j, j] - Wo[:, j].sum()
        nonC = np.flatnonzero(~inC[:, j])
        un = [i for i in nonC if not mask[i, j]]
        i0 = un[0] if un else nonC[0]
        Wo[i0, j] = Wo[i0, j] + e
    if r:
        S = Q.T @ Y @ Q
        Sp = _spectral(S, lambda x: one / x if x > mp.mpf(10) ** -12 else zero)
        U = Y @ (Q @ (Sp @ Vt))
    else:
        U = _z(n, k)
    return dict(X=Xo, W=Wo, Theta=Tho, Y=Y, U=U, V1=V1 / s2, V2=V2 / s2, V3=V3 / s2, objective=obj_s / s2, rp=rp, rd=rd, n_bumps=n_bumps, rho=rho)


def distance_to_mp(ref, hp):
    """{name: ||float64 array - high-precision array||_F, computed at the high precision} for what shor_state_mp returns."""
    mp = _mp()
    out = {}
    for key in ARRAYS + ("objective", "rp", "rd"):
        a = _o(np.asarray(ref[key], float)).ravel()
        b = np.empty(a.shape, dtype=object)
        b[:] = list(np.asarray(hp[key], dtype=object).ravel()) if a.size > 1 or isinstance(hp[key], np.ndarray) else [hp[key]]
        out[key] = float(mp.sqrt(_fro2(a - b)))
    return out
