"""References, inputs and bounds for the LOBPCG tests (test infrastructure: numpy/scipy only, no GPU, no oracle).

The m^3 7-point Poisson operator with the generator's scaling and its closed-form spectrum, the start vectors, a float64 numpy
restatement of sgpu_eigs_LOBPCG (saena_amd/csrc/sgpu_eig.hip.inc) with a callable preconditioner, restatements of k_block_mix and
k_eig_residual (saena_amd/csrc/kernels_eig.hip.h), and the bounds tests/test_gpu_eig.py asserts.  tests/test_eig_ref.py shows on
the CPU that a correct implementation stays inside every one of them, and pins the numbers recorded below.
"""
import numpy as np
import scipy.linalg

from tests import gmres_ref as gr, solver_ref as sr

U = sr.U
TOL = 1e-8
# the shapes of the GPU tests: (m, K, nev).  8^3 and 16^3 are the smallest with a two- and a three-level hierarchy (aggregates of
# 2x2x2 down to 64 rows); the spectrum starts with clusters of 1 + 3 + 3 eigenvalues, so nev = 1, 4 and 7 end at a gap
SHAPES = ((8, 4, 4), (16, 4, 4), (16, 8, 7), (16, 2, 1))

# ---- recorded by tests/test_eig_ref.py (which asserts that the reference still gives them) ----
# iterations of the reference to TOL with the V-cycle (Jacobi 3 + 3, direct coarsest solve) and without a preconditioner
ITERS = {(8, 4, 4): 20, (16, 4, 4): 23, (16, 8, 7): 26, (16, 2, 1): 12}
# (the plain counts are sensitive to rounding -- the dense Rayleigh-Ritz solver alone moves them: 85 / 169 / 159 / 95 with LAPACK here,
# 91 / 163 / 161 / 95 with the library's Jacobi solver in the same loop, 177 / 169 / 156 / 95 in the prototype the feature was specified
# from, whose Rayleigh-Ritz step differed -- the preconditioned counts are the same in all three; nothing is asserted on the GPU about
# a plain count beyond the ratio below)
ITERS_PLAIN = {(8, 4, 4): 85, (16, 4, 4): 169, (16, 8, 7): 159, (16, 2, 1): 95}
# max |X^T X - I| of the reference's result
ORTHO = {(8, 4, 4): 6.7e-16, (16, 4, 4): 1.4e-15, (16, 8, 7): 1.3e-15, (16, 2, 1): 2.3e-16}
ORTHO_MARGIN = 16          # the GPU sums in another order
PLAIN_RATIO_MIN = 3        # precond = 0 needs at least this many times the iterations of precond = 1 (the reference: about 7)


def iteration_bound(shape):
    """ceil(1.25 x the reference's count) + 2: a threshold crossed one iteration later by rounding is not a failure"""
    return int(np.ceil(1.25 * ITERS[shape])) + 2


# ---------------------------------------------------------------------------
# the operator
def poisson(m):
    """the interior m^3 system of the generator's laplacian3D on an (m+2)^3 grid: (m+1)^2 times the 7-point stencil (6, -1)"""
    return ((m + 1.0) ** 2 * gr.convdiff(m, 0.0)).tocsr()


def analytic(m, k):
    """the k smallest eigenvalues of poisson(m), ascending: (m+1)^2 sum_d 4 sin^2(pi k_d / (2 (m+1))), k_d = 1 .. m"""
    t = 4.0 * np.sin(np.pi * np.arange(1, m + 1) / (2.0 * (m + 1))) ** 2
    lam = (m + 1.0) ** 2 * (t[:, None, None] + t[None, :, None] + t[None, None, :]).ravel()
    return np.sort(lam)[:k]


def start_vectors(n, K):
    i = np.arange(n, dtype=np.float64)[:, None]
    j = np.arange(K, dtype=np.float64)[None, :]
    return np.sin(0.37 * (j + 1) * i + 0.1 * j) + 0.2 * np.cos(1.3 * i * (j + 2)) + 0.05


_cache = {}


def case(m):
    """-> dict(A, As, Ps, Rs) of poisson(m) with tests/hierarchy.poisson_hierarchy's construction (through gmres_ref), computed once"""
    if m not in _cache:
        A = poisson(m)
        As, Ps, Rs = gr.aggregate_hierarchy(A, m)
        _cache[m] = dict(A=A, As=As, Ps=Ps, Rs=Rs)
    return _cache[m]


def vcycle_block(c):
    """the preconditioner of the reference: gmres_ref.vcycle column by column"""
    return lambda R: np.stack([gr.vcycle(c["As"], c["Ps"], c["Rs"], R[:, j]) for j in range(R.shape[1])], axis=1)


# ---------------------------------------------------------------------------
# the kernels, restated
def block_mix(sources, coefs, add=None):
    """k_block_mix: Out[i, b] = sum_s sum_a S_s[i, a] C_s[a, b] from 0.0, sources in argument order, a ascending, every product
    rounded, then added; add (if given) is added last"""
    out = np.zeros_like(np.asarray(sources[0], np.float64))
    for S, Cm in zip(sources, coefs):
        for a in range(S.shape[1]):
            out = out + S[:, a:a + 1] * np.asarray(Cm, np.float64)[a:a + 1, :]
    if add is not None:
        out = out + add
    return out


def eig_residual(AX, X, lam):
    """k_eig_residual: R = AX - X diag(lam), the product rounded, then subtracted"""
    return AX - X * np.asarray(lam, np.float64)[None, :]


# ---------------------------------------------------------------------------
# the small dense pieces
def chol_rel(G):
    """host/dense_eig.cpp's Cholesky: a pivot must exceed 256 n eps times its diagonal entry.  -> L, or None"""
    G = np.asarray(G, np.float64)
    n = G.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        if not (G[j, j] > 0.0 and np.isfinite(G[j, j])):
            return None
        d = G[j, j] - float(L[j, :j] @ L[j, :j])
        if not d > 256.0 * n * np.finfo(np.float64).eps * G[j, j]:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (G[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    return L


def ortho_factor(G, act, K):
    """T (K x K, zero outside the rows and columns of act) = L^-T of the act x act part of G, or None"""
    T = np.zeros((K, K))
    if not act:
        return T
    S = G[np.ix_(act, act)]
    L = chol_rel(0.5 * (S + S.T))
    if L is None:
        return None
    T[np.ix_(act, act)] = scipy.linalg.solve_triangular(L, np.eye(len(act)), lower=True).T
    return T


class Breakdown(ArithmeticError):
    pass


# ---------------------------------------------------------------------------
# the solver
def lobpcg(A, X0, nev, tol=TOL, max_iter=100, precond=None):
    """sgpu_eigs_LOBPCG in float64 numpy, step for step.  precond: callable R (n, K) -> W (None: W = R).
    -> dict(X, lam, res, iters, hist (iterations + 1, K), converged)"""
    X = np.array(X0, np.float64)
    n, K = X.shape
    every = list(range(K))
    T = ortho_factor(X.T @ X, every, K)
    if T is None:
        raise ValueError("the start vectors are linearly dependent")
    X = block_mix([X], [T])
    AX = A @ X
    H = X.T @ AX
    lam, Q = np.linalg.eigh(0.5 * (H + H.T))
    X, AX = block_mix([X], [Q]), block_mix([AX], [Q])
    P = AP = None
    it, fresh, hist = 0, False, []
    while True:
        R = eig_residual(AX, X, lam)
        rr = np.sum(R * R, axis=0)
        if not fresh:                                          # (a recomputed residual almost always ends the solve: no W for it)
            W = R.copy() if precond is None else precond(R)
            XtW = X.T @ W
        if len(hist) > it:
            hist[it] = np.sqrt(rr)
        else:
            hist.append(np.sqrt(rr))
        act = [j for j in range(K) if not rr[j] < tol * tol * lam[j] * lam[j]]
        conv = not any(j < nev for j in act)
        if conv or it >= max_iter:
            if fresh:
                return dict(X=X, lam=lam, res=np.sqrt(rr), iters=it, hist=np.array(hist), converged=conv)
            AX = A @ X                                         # only recomputed norms declare convergence
            fresh = True
            continue
        if fresh:                                              # the recomputed norms contradict the carried ones: go on from them
            W = R.copy() if precond is None else precond(R)
            XtW = X.T @ W
            fresh = False
        Cw = np.zeros((K, K))
        Cw[:, act] = -XtW[:, act]
        W = block_mix([X], [Cw], add=W)
        Tw = ortho_factor(W.T @ W, act, K)
        if Tw is None:
            raise Breakdown(f"W^T W is not positive definite at iteration {it + 1}")
        Tp = ortho_factor(P.T @ P, act, K) if P is not None else None
        useP = Tp is not None
        W = block_mix([W], [Tw])
        AW = A @ W
        if useP:
            P, AP = block_mix([P], [Tp]), block_mix([AP], [Tp])
        S = [X, W[:, act]] + ([P[:, act]] if useP else [])
        AS = [AX, AW[:, act]] + ([AP[:, act]] if useP else [])
        S, AS = np.hstack(S), np.hstack(AS)
        GS, GA = S.T @ S, S.T @ AS
        theta, V = scipy.linalg.eigh(0.5 * (GA + GA.T), 0.5 * (GS + GS.T))
        if not theta[0] > 0.0:
            raise Breakdown("a Ritz value is not positive")
        na = len(act)
        CX, CW, CP = V[:K, :K], np.zeros((K, K)), np.zeros((K, K))
        CW[act] = V[K:K + na, :K]
        if useP:
            CP[act] = V[K + na:K + 2 * na, :K]
            P, AP = block_mix([W, P], [CW, CP]), block_mix([AW, AP], [CW, CP])
        else:
            P, AP = block_mix([W], [CW]), block_mix([AW], [CW])
        X, AX = block_mix([X], [CX], add=P), block_mix([AX], [CX], add=AP)
        lam = theta[:K].copy()
        it += 1


# ---------------------------------------------------------------------------
# the bounds of the GPU test
def residual_hp(A, x, lam):
    """-> (rho, rounding): rho = ||A x - lam x|| / ||x|| in longdouble with scipy's A, and the rounding term of assertion 1,
    (longest row + 3) u || |A||x| + lam |x| || / ||x||"""
    A = A.tocsr()
    xl = np.asarray(x, np.longdouble)
    prod = A.data.astype(np.longdouble) * xl[A.indices]
    Ax = np.add.reduceat(prod, A.indptr[:-1])
    r = Ax - np.longdouble(lam) * xl
    nx = float(np.sqrt(np.sum(xl * xl)))
    mag = abs(A) @ np.abs(x) + lam * np.abs(x)
    longest = int(np.diff(A.indptr).max())
    return float(np.sqrt(np.sum(r * r))) / nx, (longest + 3) * U * float(np.linalg.norm(mag)) / nx


def check_pairs(A, X, lam, nev, m, tol=TOL, what=""):
    """assertions 1 and 2 of tests/test_gpu_eig.py on the first nev pairs: rho_j <= tol lam_j + rounding, and
    |lam_j - analytic_j| <= rho_j.  -> the rho_j"""
    exact = analytic(m, nev)
    rhos = []
    for j in range(nev):
        rho, rounding = residual_hp(A, X[:, j], lam[j])
        print(f"{what} pair {j}: lambda {lam[j]:.15e} (closed form {exact[j]:.15e}, off by {abs(lam[j] - exact[j]):.2e}), rho {rho:.3e} "
              f"of {tol * lam[j] + rounding:.3e}")
        assert rho <= tol * lam[j] + rounding, (what, j, rho)
        assert abs(lam[j] - exact[j]) <= rho, (what, j, lam[j], exact[j], rho)
        rhos.append(rho)
    return rhos


def ortho_defect(X):
    return float(np.max(np.abs(X.T @ X - np.eye(X.shape[1]))))
