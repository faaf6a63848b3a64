"""References for the plain device operations around the relaxation -- separation (eigs(U U' - Y), OMC.jl:1274, 2466-2477), rounding
(svd(Y).U[:, 1:k], OMC.jl:873), left singular vectors (svd(X).U[:, 1:k], OMC.jl:524, 564, 921) and the objective scan (OMC.jl:2352-2358).
numpy only; the product path never imports this module.

Three kinds of reference:
  * eigenvalues in long double: Rayleigh quotients, evaluated in long double, of LAPACK's eigenvectors of the float64 matrix.  The quotient
    is quadratic in the eigenvector error, so it is good to about 1e-19 ||M|| where the eigenvalues are separated (and inside a cluster the
    error only mixes vectors of nearly equal eigenvalue);
  * a plain float64 restatement of the kernel's algorithm (Hestenes one-sided Jacobi on M + sigma I, sigma = 1.5 ||M||_F, rotation rule
    g^2 > tau^2 a b with tau = 1e-14, at most 30 sweeps, eigenvalue = column norm - sigma): how accurate a correct implementation is.  Its
    error grows about linearly in the order (the cancellation in norm - sigma), so a bound c u ||M|| with a constant c would be wrong;
  * the objective by math.fsum over long-double products.
and seeded input builders with planted spectra, so the gaps a vector comparison needs hold by construction."""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, (
    "omc_plain_ref: np.longdouble has eps = %g on this platform (64-bit long double?); the high-precision references need an 80-bit "
    "or wider long double" % float(np.finfo(LD).eps))

U_RND = 1.1e-16
TAU = 1e-14
MAX_SWEEPS = 30


# ---- matrices as the kernel forms them ------------------------------------------------------------------------------------------------
def sep_matrix(Y, U):
    """float64 U U' - Y, symmetrised (cone_M_entry / eig_frontend)."""
    M = U @ U.T - Y
    return 0.5 * (M + M.T)


def sep_matrix_ld(Y, U):
    Ul = np.asarray(U, LD); M = Ul @ Ul.T - np.asarray(Y, LD)
    return (M + M.T) * LD(0.5)


def sym(M):
    return 0.5 * (M + M.T)


def sym_ld(M):
    Ml = np.asarray(M, LD)
    return (Ml + Ml.T) * LD(0.5)


def gram_ld(X):
    Xl = np.asarray(X, LD)
    return Xl @ Xl.T


def fro(M):
    return float(np.sqrt((np.asarray(M, LD) ** 2).sum()))


# ---- high-precision eigenvalues ----------------------------------------------------------------------------------------------------
def rayleigh_eigvals(M_ld):
    """Ascending eigenvalues of the symmetric long-double matrix M_ld (see the module docstring), as long doubles, and LAPACK's float64
    eigenvectors in the same order."""
    M_ld = np.asarray(M_ld, LD)
    _, V = np.linalg.eigh(np.asarray(M_ld, np.float64))
    Vl = np.asarray(V, LD)
    lam = ((Vl * (M_ld @ Vl)).sum(axis=0)) / (Vl * Vl).sum(axis=0)
    order = np.argsort(lam, kind="stable")
    return lam[order], V[:, order]


# ---- the kernel's algorithm, restated ------------------------------------------------------------------------------------------------
def shift_of(M):
    """sigma of eig_frontend: 1.5 ||M||_F, and 1 for the exact zero matrix."""
    f = float(np.sqrt((M * M).sum()))
    return 1.0 if f == 0.0 else 1.5 * f


def jacobi_restated(M, tau=TAU, max_sweeps=MAX_SWEEPS):
    """Hestenes one-sided Jacobi on G = M + sigma I (M symmetric float64).  Round-robin pair order: the pairs of one step are disjoint, so
    taking them together is the cyclic order pair after pair.  Returns (eigenvalues ascending, unit eigenvectors as columns in that order,
    sweeps); the sweep without a rotation that ends the loop is counted, as the kernel counts it."""
    M = np.asarray(M, np.float64)
    N = M.shape[0]
    sigma = shift_of(M)
    G = M + sigma * np.eye(N)
    Np = (N + 1) & ~1
    ring = list(range(1, Np))
    sweeps = 0
    tau2 = tau * tau
    while sweeps < max_sweeps:
        sweeps += 1
        rotated = False
        for step in range(Np - 1):
            arr = [0] + ring[step:] + ring[:step]
            p = np.array(arr[: Np // 2]); q = np.array(arr[Np // 2:][::-1])
            keep = (p < N) & (q < N)
            p, q = p[keep], q[keep]
            gp, gq = G[:, p], G[:, q]
            a = (gp * gp).sum(axis=0); b = (gq * gq).sum(axis=0); g = (gp * gq).sum(axis=0)
            rot = (g * g > tau2 * a * b) & (a > 0.0) & (b > 0.0)
            if not rot.any():
                continue
            rotated = True
            p, q, gp, gq, a, b, g = p[rot], q[rot], gp[:, rot], gq[:, rot], a[rot], b[rot], g[rot]
            zeta = (b - a) / (2.0 * g)
            t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            c = 1.0 / np.sqrt(1.0 + t * t); s = c * t
            G[:, p] = c * gp - s * gq
            G[:, q] = s * gp + c * gq
        if not rotated:
            break
    nrm = np.sqrt((G * G).sum(axis=0))
    lam = nrm - sigma
    order = np.argsort(lam, kind="stable")
    return lam[order], (G / nrm)[:, order], sweeps


def lapack_shifted(M):
    """LAPACK on the shifted matrix, shift removed: the other float64 computation of the same quantity."""
    sigma = shift_of(M)
    return np.linalg.eigvalsh(M + sigma * np.eye(M.shape[0])) - sigma


def reference_error(M, lam_ld, restated=None):
    """e_ref of an input: the larger of the two float64 computations' errors (whole spectrum, ascending order against ascending order)
    against the long-double values.  Returns (e_ref, restatement error, LAPACK error, sweeps)."""
    lj, _, sw = restated if restated is not None else jacobi_restated(M)
    ej = float(np.abs(np.asarray(lj, LD) - lam_ld).max())
    el = float(np.abs(np.asarray(lapack_shifted(M), LD) - lam_ld).max())
    return max(ej, el), ej, el, sw


# ---- objective ---------------------------------------------------------------------------------------------------------------------------
def objective_ref(X, A, mask, gamma):
    """1/2 sum_Omega (X - A)^2 + ||X||_F^2 / (2 gamma): long-double products, summed by math.fsum.  fsum rounds its exact sum to a double,
    so it is called twice -- the sum s, then the sum of the terms and -s, the remainder -- on the float64 heads of the products, and once
    on their tails: the result is good to the long double's own rounding."""
    Xl = np.asarray(X, LD); D = (Xl - np.asarray(A, LD))[np.asarray(mask, bool)]

    def fsum_ld(v):
        hi = np.asarray(v, np.float64)
        lo = np.asarray(v - np.asarray(hi, LD), np.float64).ravel().tolist()
        terms = hi.ravel().tolist()
        s = math.fsum(terms)
        terms.append(-s)
        return LD(s) + (LD(math.fsum(terms)) + LD(math.fsum(lo)))

    return fsum_ld(D * D) * LD(0.5) + fsum_ld(Xl * Xl) / (LD(2.0) * LD(gamma))


# ---- input builders ----------------------------------------------------------------------------------------------------------------------
def orthogonal(N, rng):
    return np.linalg.qr(rng.standard_normal((N, N)))[0]


def planted(lam, rng):
    """Q diag(lam) Q' with Q from a QR of a seeded Gaussian, symmetrised."""
    lam = np.asarray(lam, np.float64)
    Q = orthogonal(lam.size, rng)
    return sym((Q * lam) @ Q.T)


SEP_FAMILIES = ["a", "b_out", "b_in", "c_two", "c_one", "d", "e", "f_small", "f_big", "g"]
FEAS_TOL = -1e-6      # OMC.jl:1274-1276
TWO_TOL = -1e-10      # OMC.jl:2471-2473


def sep_spectrum(family, N, rng):
    """Planted eigenvalues of U U' - Y (ascending in their first two places)."""
    rest = max(N - 2, 0)
    if family in ("a", "f_small", "f_big"):
        lam = np.concatenate([[-1.0, -0.7], rng.uniform(-0.4, 0.5, rest)])
    elif family in ("b_out", "b_in"):
        hi = min(1.0, 15.0 / math.sqrt(N))      # keeps ||M||_F <= 10 at every order
        lam = np.concatenate([[-2e-6 if family == "b_out" else -0.5e-6], rng.uniform(-1e-7, hi, N - 1)])
    elif family in ("c_two", "c_one"):
        lam = np.concatenate([[-1e-3, -2e-10 if family == "c_two" else -0.5e-10], rng.uniform(1e-3, 1e-2, rest)])
    elif family == "d":
        lam = np.concatenate([[-1.0, -1.0], rng.uniform(-0.4, 0.5, rest)])
    else:
        raise ValueError(family)
    return lam[:N]


def sep_input(family, N, k, seed):
    """(Y, U) of a separation call at order N, rank k.  Families (a)-(g) of the module's tests; 'b_out' / 'b_in' are the two sides of the
    feasibility threshold, 'c_two' / 'c_one' the two sides of the smallest_2_eigvec switch, 'f_small' / 'f_big' family (a) with M scaled by
    1e-12 / 1e+12 (U by 1e-6 / 1e+6)."""
    rng = np.random.default_rng(seed)
    if family == "e":
        U = np.zeros((N, k)); U[np.arange(k), np.arange(k)] = 1.0
        return U @ U.T, U
    if family == "g":
        B = rng.standard_normal((N, N))
        return B @ B.T / N, 0.2 * rng.standard_normal((N, k))
    M = planted(sep_spectrum(family, N, rng), rng)
    U = 0.5 * np.linalg.qr(rng.standard_normal((N, k)))[0]
    if family in ("f_small", "f_big"):
        s = 1e-12 if family == "f_small" else 1e12
        M = M * s; U = U * math.sqrt(s)
    return U @ U.T - M, U


ROUND_FAMILIES = ["top", "projector", "zero", "top_small", "top_big"]


def round_input(family, N, k, seed):
    """Symmetric PSD Y of a rounding call.  'top': k eigenvalues spread over [0.8, 1] and a decaying tail below 0.3; 'projector': a rank-3
    projector (the top is repeated and the answer at k = 2 is a subspace; rank N where N < 3); 'zero'; 'top_small' / 'top_big': 'top'
    scaled by 1e-12 / 1e+12."""
    rng = np.random.default_rng(seed)
    if family == "zero":
        return np.zeros((N, N))
    if family == "projector":
        r = min(3, N)
        Q = orthogonal(N, rng)[:, :r]
        return sym(Q @ Q.T)
    lam = np.concatenate([np.linspace(1.0, 0.8, k) if k > 1 else [1.0], 0.3 * 0.5 ** np.arange(max(N - k, 0))])[:N]
    Y = planted(lam, rng)
    if family == "top_small":
        Y = Y * 1e-12
    elif family == "top_big":
        Y = Y * 1e12
    elif family != "top":
        raise ValueError(family)
    return Y


SVD_FAMILIES = ["product", "sparse", "zero"]


def svd_input(family, n, m, k, seed):
    """n x m matrix X of a left-singular-vector call, k <= min(n, m).  'product': U V of rank k with singular values 2, 1, 1/2, ..; 'sparse':
    a zero-filled sparse matrix (about 80 % observed) whose dominant part has rank k, re-drawn until sigma_k / sigma_{k+1} >= 2; 'zero'."""
    if family == "zero":
        return np.zeros((n, m))
    for attempt in range(200):
        rng = np.random.default_rng([seed, attempt])
        P = np.linalg.qr(rng.standard_normal((n, k)))[0]; R = np.linalg.qr(rng.standard_normal((m, k)))[0]
        X = (P * (2.0 * 0.5 ** np.arange(k))) @ R.T
        if family == "product":
            return X
        if family != "sparse":
            raise ValueError(family)
        X = np.where(rng.random((n, m)) < 0.8, X, 0.0)
        sv = np.linalg.svd(X, compute_uv=False)
        if sv[k - 1] > 0.0 and (len(sv) == k or sv[k - 1] >= 2.0 * sv[k]):
            return X
    raise RuntimeError("svd_input: no sparse draw with sigma_k / sigma_{k+1} >= 2 at (%d, %d, %d)" % (n, m, k))


def canon(v):
    """Canonical sign: the entry of largest magnitude is positive."""
    i = int(np.argmax(np.abs(v)))
    return v if v[i] >= 0 else -v


def sign_is_decided(v, rel=1e-6):
    """False when the two largest |entries| differ by less than rel (relative): the canonical sign is then a coin toss."""
    a = np.sort(np.abs(v))
    return a.size < 2 or a[-1] - a[-2] >= rel * a[-1]


# ---- the cases of tests/test_plain_ops.py, shared with tools/record_plain_ops_error_units.py ----------------------------------------
# order 514 (one lane per pair in the generic sweep) is left out: a one-matrix separation call takes 2.05 s there on an MI355X, the 20 calls
# of the families under both rules 41 s
SEP_ORDERS = [2, 3, 15, 16, 17, 18, 63, 64, 65, 66, 127, 128, 129, 134, 135, 200, 255, 256, 257, 300]
ROUND_ORDERS = SEP_ORDERS
ROUND_K8_ORDERS = [16, 17, 134, 135]
SVD_SHAPES = ([(n, m) for n in (2, 15, 16, 17, 33) for m in (1, 3, 4, 5, 15, 16, 17, 19, 20, 31, 32, 33)]
              + [(134, 140), (135, 40), (300, 7), (135, 135), (300, 303)])
RECORDED_FROM = 200      # e_ref of orders from here on is read from tests/golden/plain_ops_error_units.json, below it is computed by the test
SEP_K = 2


def sep_cases(N):
    """[(key, family, seed)] of the separation batch at order N."""
    return [("sep/%d/%s" % (N, f), f, 100 * N + i) for i, f in enumerate(SEP_FAMILIES)]


def round_cases(N, k):
    fams = [f for f in ROUND_FAMILIES if f != "projector" or k == 2]
    return [("round/%d/k%d/%s" % (N, k, f), f, 100 * N + 50 + 7 * k + i) for i, f in enumerate(fams)]


def round_ranks(N):
    return [k for k in (1, 2) if k <= N] + ([8] if N in ROUND_K8_ORDERS else [])


def svd_cases(n, m, k):
    return [("svd/%dx%d/k%d/%s" % (n, m, k, f), f, 100000 + 1000 * n + 10 * m + i) for i, f in enumerate(SVD_FAMILIES)]


def svd_shape_accepted(n, m, k):
    """An instance needs n <= m (OMC.jl:249-254) and the planted X rank k."""
    return n <= m and k <= n


def measure_case(M, M_ld):
    """What the golden file records of an input: ||M||_F, e_ref in units of u ||M||_F, the restatement's sweeps."""
    lam, _ = rayleigh_eigvals(M_ld)
    e, _, _, sw = reference_error(M, lam)
    f = fro(M)
    return {"fro": f, "units": (e / (U_RND * f)) if f > 0.0 else 0.0, "sweeps": sw}


# ---- where the cold kernel k_cone holds its matrix, and which sweep its front end takes: csrc/omc_layout.h and eig_frontend mirrored ----
OMC_MAX_DYN_LDS = 144 * 1024
JROWS = 20
LAYOUT_LINES = [      # the definitions mirrored below, as csrc/omc_layout.h and csrc/omc_device.hip state them
    ("omc_layout.h", "#define OMC_MAX_DYN_LDS (144 * 1024)"),
    ("omc_layout.h", "OMC_HD ConeLayout cone_carve(int N, int ld) { const int Np = (N + 1) & ~1; const size_t ev = (size_t)Np * ld; return {Np, ld, ev, ev + Np, ev + 2 * Np}; }"),
    ("omc_layout.h", "OMC_HD ConeLayout cone_layout(int N) { return cone_carve(N, ((N + 1) & ~1) | 1); }"),
    ("omc_layout.h", "OMC_HD size_t cone_bytes(int N) { const ConeLayout L = cone_layout(N); return L.sel * 8 + (size_t)L.Np * 4 + 16; }"),
    ("omc_layout.h", "g.cone = plan_block(cone_bytes(n), cone_bytes(n) <= OMC_MAX_DYN_LDS);"),
    ("omc_device.hip", "#define JROWS 20"),
    ("omc_device.hip", "while (lpp > 1 && lpp * (Np >> 1) > T) lpp >>= 1;"),
    ("omc_device.hip", "} else if (lpp >= 4 && (N + lpp - 1) / lpp <= JROWS) {"),
]


def cone_bytes(N):
    Np = (N + 1) & ~1; ld = Np | 1
    sel = Np * ld + 2 * Np
    return sel * 8 + Np * 4 + 16


def cone_in_lds(N):
    return cone_bytes(N) <= OMC_MAX_DYN_LDS


def dispatch_class(N, T=512):
    """The sweep eig_frontend runs at order N with T threads."""
    Np = (N + 1) & ~1
    lpp = 64
    while lpp > 1 and lpp * (Np >> 1) > T:
        lpp >>= 1
    lpp = min(lpp, 16)
    if Np <= 16:
        return "wave16"
    if lpp >= 4 and (N + lpp - 1) // lpp <= JROWS:
        return "t%d" % lpp
    return "generic%d" % lpp


def layout_lines_missing(csrc_dir):
    """The mirrored definitions that the sources no longer contain verbatim (empty: the mirror is current)."""
    import os
    missing = []
    for name, line in LAYOUT_LINES:
        with open(os.path.join(csrc_dir, name)) as f:
            if line not in f.read():
                missing.append((name, line))
    return missing
