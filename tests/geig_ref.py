"""References, inputs and bounds for the tests of the generalised LOBPCG, A x = lambda B x (test infrastructure: numpy/scipy only, no
GPU, no oracle).

The two mass matrices next to eig_ref.poisson(m) -- the 27-point consistent one with its closed-form generalised spectrum, and a lumped
(diagonal) one with a jump --, a float64 numpy restatement of sgpu_eigs_LOBPCG_gen (lobpcg_run with B, saena_amd/csrc/sgpu_eig.hip.inc) built from
eig_ref's pieces, the restatement of k_geig_residual (saena_amd/csrc/kernels_eig.hip.h), and the bounds tests/test_gpu_geig.py
asserts.  tests/test_geig_ref.py shows on the CPU that a correct implementation stays inside every one of them, and pins the numbers
recorded below: they are this reference's, never the GPU's.
"""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg

from tests import eig_ref as er

U = er.U
TOL = er.TOL
SHAPES = er.SHAPES
MASSES = ("mass27", "lumped")

# ---- recorded by tests/test_geig_ref.py (which asserts that the reference still gives them) ----
# iterations of the reference to TOL with the V-cycle of A (Jacobi 3 + 3, direct coarsest solve) and without a preconditioner
ITERS_GEN = {((8, 4, 4), "mass27"): 20, ((16, 4, 4), "mass27"): 22, ((16, 8, 7), "mass27"): 29, ((16, 2, 1), "mass27"): 12,
             ((8, 4, 4), "lumped"): 34, ((16, 4, 4), "lumped"): 33, ((16, 8, 7), "lumped"): 25, ((16, 2, 1), "lumped"): 13}
# (as in eig_ref, a plain count is sensitive to rounding; nothing is asserted on the GPU about one beyond the 16^3 ratio)
ITERS_GEN_PLAIN = {((8, 4, 4), "mass27"): 82, ((16, 4, 4), "mass27"): 179, ((16, 8, 7), "mass27"): 154, ((16, 2, 1), "mass27"): 94,
                   ((8, 4, 4), "lumped"): 121, ((16, 4, 4), "lumped"): 254, ((16, 8, 7), "lumped"): 148, ((16, 2, 1), "lumped"): 107}
# max |X^T B X - I| of the reference's result
ORTHO_GEN = {((8, 4, 4), "mass27"): 1.4e-15, ((16, 4, 4), "mass27"): 1.8e-15, ((16, 8, 7), "mass27"): 3.4e-15, ((16, 2, 1), "mass27"): 3.4e-15,
             ((8, 4, 4), "lumped"): 1.1e-15, ((16, 4, 4), "lumped"): 3.8e-15, ((16, 8, 7), "lumped"): 2.9e-15, ((16, 2, 1), "lumped"): 3.6e-15}
ORTHO_MARGIN = er.ORTHO_MARGIN
PLAIN_RATIO_MIN = er.PLAIN_RATIO_MIN      # asserted on 16^3 only: 8^3 is too close to it (3.6 with `lumped`)
# a lower bound of lambda_min(B), for the eigenvalue bound |lambda - lambda*| <= ||r|| / sqrt(lambda_min(B)) of a B-normalised x:
# mass27's factors have mu_i = 1 - t_i / 6 > 1/3; lumped's diagonal is at least 1
LAMBDA_MIN_B = {"mass27": 1.0 / 27.0, "lumped": 1.0}


def iteration_bound(shape, mass):
    """ceil(1.25 x the reference's count) + 2, eig_ref's margin"""
    return int(np.ceil(1.25 * ITERS_GEN[(shape, mass)])) + 2


# ---------------------------------------------------------------------------
# the mass matrices
def mass27(m):
    """M1 x M1 x M1 (Kronecker), M1 = tridiag(1/6, 4/6, 1/6) of order m: the consistent mass matrix of trilinear elements on the grid of
    eig_ref.poisson(m), 27 entries per interior row.  M1 = I - T/6 with T the 1-D second difference, so A and every factor of B are
    polynomials in the same matrix and the eigenvectors are shared"""
    M1 = sp.diags([np.full(m - 1, 1.0 / 6.0), np.full(m, 4.0 / 6.0), np.full(m - 1, 1.0 / 6.0)], [-1, 0, 1])
    return sp.kron(sp.kron(M1, M1), M1).tocsr()


def analytic_mass27(m, k):
    """the k smallest eigenvalues of poisson(m) x = lambda mass27(m) x, ascending: (m+1)^2 (t_i + t_j + t_k) / (mu_i mu_j mu_k),
    t_i = 4 sin^2(pi i / (2 (m+1))), mu_i = 1 - t_i / 6"""
    t = 4.0 * np.sin(np.pi * np.arange(1, m + 1) / (2.0 * (m + 1))) ** 2
    mu = 1.0 - t / 6.0
    lam = (m + 1.0) ** 2 * (t[:, None, None] + t[None, :, None] + t[None, None, :]) / (mu[:, None, None] * mu[None, :, None] * mu[None, None, :])
    return np.sort(lam.ravel())[:k]


def lumped(m):
    """a diagonal mass matrix with a density that jumps: 1 + 0.5 sin^2(0.05 i) + 3 [(i mod m) > m // 2], i the row"""
    i = np.arange(m ** 3)
    d = 1.0 + 0.5 * np.sin(0.05 * i) ** 2 + 3.0 * ((i % m) > m // 2)
    return sp.diags(d).tocsr()


_mass = {}
_exact = {}


def mass(name, m):
    if (name, m) not in _mass:
        _mass[(name, m)] = {"mass27": mass27, "lumped": lumped}[name](m)
    return _mass[(name, m)]


def exact(name, m, k):
    """the k smallest generalised eigenvalues: the closed form for mass27; for lumped a dense scipy.linalg.eigh(A, B) on 8^3 and
    eigsh(A, M=B, sigma=0) on 16^3.  Computed once"""
    if name == "mass27":
        return analytic_mass27(m, k)
    if (name, m) not in _exact:
        A, B = er.poisson(m), mass(name, m)
        if m <= 8:
            _exact[(name, m)] = scipy.linalg.eigh(A.toarray(), B.toarray(), eigvals_only=True)[:16]
        else:
            _exact[(name, m)] = np.sort(scipy.sparse.linalg.eigsh(A.tocsc(), k=16, M=B.tocsc(), sigma=0, which="LM", tol=0)[0])
    return _exact[(name, m)][:k]


# ---------------------------------------------------------------------------
# the kernel, restated
def geig_residual(AX, BX, lam):
    """k_geig_residual: R = AX - BX diag(lam), the product rounded, then subtracted (k_eig_residual with BX in X's place)
    -> (R, ||r_j||^2, ||(BX)_j||^2), the norms as plain numpy sums (the kernel's order of summation is the block dot's)"""
    R = er.eig_residual(AX, BX, lam)
    return R, np.sum(R * R, axis=0), np.sum(BX * BX, axis=0)


# ---------------------------------------------------------------------------
# the solver
def lobpcg_gen(A, B, X0, nev, tol=TOL, max_iter=100, precond=None, stop=None):
    """sgpu_eigs_LOBPCG_gen in float64 numpy, step for step: eig_ref.lobpcg with the B-inner product and BX, BW, BP carried.
    precond: callable R (n, K) -> W (None: W = R).  stop: iteration index to return from right after the orthonormalisation step
    (sgpu_debug_eig_stop) -> dict(X, W, BW, P, BP, act, stopped=True).
    -> dict(X, lam, res, bnorm, iters, hist (iterations + 1, K), converged)"""
    X = np.array(X0, np.float64)
    n, K = X.shape
    every = list(range(K))
    BX = B @ X
    T = er.ortho_factor(X.T @ BX, every, K)
    if T is None:
        raise ValueError("X^T B X is not positive definite: the start vectors are linearly dependent, or B is not positive definite")
    X, BX = er.block_mix([X], [T]), er.block_mix([BX], [T])
    AX = A @ X
    H = X.T @ AX
    lam, Q = np.linalg.eigh(0.5 * (H + H.T))
    X, AX, BX = er.block_mix([X], [Q]), er.block_mix([AX], [Q]), er.block_mix([BX], [Q])
    P = AP = BP = None
    it, fresh, hist = 0, False, []
    while True:
        R, rr, bb = geig_residual(AX, BX, lam)
        if not fresh:
            W = R.copy() if precond is None else precond(R)
            XtW = BX.T @ W
        if len(hist) > it:
            hist[it] = np.sqrt(rr)
        else:
            hist.append(np.sqrt(rr))
        act = [j for j in range(K) if not rr[j] < tol * tol * lam[j] * lam[j] * bb[j]]
        conv = not any(j < nev for j in act)
        if conv or it >= max_iter:
            if fresh:
                return dict(X=X, lam=lam, res=np.sqrt(rr), bnorm=np.sqrt(bb), iters=it, hist=np.array(hist), converged=conv)
            AX, BX = A @ X, B @ X                              # only recomputed norms declare convergence
            fresh = True
            continue
        if fresh:
            W = R.copy() if precond is None else precond(R)
            XtW = BX.T @ W
            fresh = False
        Cw = np.zeros((K, K))
        Cw[:, act] = -XtW[:, act]
        W = er.block_mix([X], [Cw], add=W)
        BW = B @ W
        Tw = er.ortho_factor(W.T @ BW, act, K)
        if Tw is None:
            raise er.Breakdown(f"W^T B W is not positive definite at iteration {it + 1}")
        Tp = er.ortho_factor(P.T @ BP, act, K) if P is not None else None
        useP = Tp is not None
        W, BW = er.block_mix([W], [Tw]), er.block_mix([BW], [Tw])
        AW = A @ W
        if useP:
            P, AP, BP = er.block_mix([P], [Tp]), er.block_mix([AP], [Tp]), er.block_mix([BP], [Tp])
        if stop == it:
            return dict(X=X, BX=BX, W=W, BW=BW, AW=AW, P=P if useP else None, BP=BP if useP else None, act=act, Tw=Tw, stopped=True)
        S = np.hstack([X, W[:, act]] + ([P[:, act]] if useP else []))
        AS = np.hstack([AX, AW[:, act]] + ([AP[:, act]] if useP else []))
        BS = np.hstack([BX, BW[:, act]] + ([BP[:, act]] if useP else []))
        GS, GA = S.T @ BS, S.T @ AS
        theta, V = scipy.linalg.eigh(0.5 * (GA + GA.T), 0.5 * (GS + GS.T))
        if not theta[0] > 0.0:
            raise er.Breakdown("a Ritz value is not positive")
        na = len(act)
        CX, CW, CP = V[:K, :K], np.zeros((K, K)), np.zeros((K, K))
        CW[act] = V[K:K + na, :K]
        if useP:
            CP[act] = V[K + na:K + 2 * na, :K]
            P, AP, BP = (er.block_mix([w, p], [CW, CP]) for w, p in ((W, P), (AW, AP), (BW, BP)))
        else:
            P, AP, BP = (er.block_mix([w], [CW]) for w in (W, AW, BW))
        X, AX, BX = er.block_mix([X], [CX], add=P), er.block_mix([AX], [CX], add=AP), er.block_mix([BX], [CX], add=BP)
        lam = theta[:K].copy()
        it += 1


# ---------------------------------------------------------------------------
# the bounds of the GPU test
def _rowsum_hp(M, xl):
    M = M.tocsr()
    prod = M.data.astype(np.longdouble) * xl[M.indices]
    return np.add.reduceat(prod, M.indptr[:-1])


def residual_hp(A, B, x, lam):
    """-> (rho, rounding, ||B x||): rho = ||A x - lam B x|| / ||B x|| in longdouble, and the rounding term of assertion 1,
    (longest row of A + longest row of B + 3) u || |A||x| + lam |B||x| || / ||B x||"""
    A, B = A.tocsr(), B.tocsr()
    xl = np.asarray(x, np.longdouble)
    Bx = _rowsum_hp(B, xl)
    r = _rowsum_hp(A, xl) - np.longdouble(lam) * Bx
    nbx = float(np.sqrt(np.sum(Bx * Bx)))
    mag = abs(A) @ np.abs(x) + lam * (abs(B) @ np.abs(x))
    longest = int(np.diff(A.indptr).max()) + int(np.diff(B.indptr).max())
    return float(np.sqrt(np.sum(r * r))) / nbx, (longest + 3) * U * float(np.linalg.norm(mag)) / nbx, nbx


def check_pairs(A, B, X, lam, nev, want, lambda_min_b, tol=TOL, what=""):
    """assertions 1 and 2 of tests/test_gpu_geig.py on the first nev pairs: rho_j <= tol lam_j + rounding, and
    |lam_j - want_j| <= rho_j ||B x_j|| / sqrt(lambda_min(B)).  -> the rho_j"""
    rhos = []
    for j in range(nev):
        rho, rounding, nbx = residual_hp(A, B, X[:, j], lam[j])
        bound = rho * nbx / np.sqrt(lambda_min_b)
        print(f"{what} pair {j}: lambda {lam[j]:.15e} (want {want[j]:.15e}, off by {abs(lam[j] - want[j]):.2e} of {bound:.2e}), rho {rho:.3e} "
              f"of {tol * lam[j] + rounding:.3e}")
        assert rho <= tol * lam[j] + rounding, (what, j, rho)
        assert abs(lam[j] - want[j]) <= bound, (what, j, lam[j], want[j], bound)
        rhos.append(rho)
    return rhos


# ---------------------------------------------------------------------------
# a solve stopped right after its orthonormalisation step (sgpu_debug_eig_stop), iterations 0 and 1 on SHAPES[0]
STOP_MASSES = MASSES
# recorded by tests/test_geig_ref.py from the reference: (max |W^T B W - I| on the active columns, max |X^T B W|) per (mass, iteration)
STOP_GEN = {("mass27", 0): (4.5e-16, 4.0e-16), ("mass27", 1): (7.8e-16, 1.2e-15), ("lumped", 0): (1.9e-15, 6.6e-16), ("lumped", 1): (2.4e-15, 1.2e-15)}


def stop_start(mass_name, m, K):
    """start vectors of the stopped solves: eig_ref.start_vectors, and for mass27 column 0 replaced by the exact eigenvector of the
    smallest eigenvalue (sin x sin x sin): the Rayleigh-Ritz step of the start reproduces it, so column 0 is converged -- inactive --
    from iteration 0 on, and the step has to zero-fill it.  With lumped every column is active"""
    X0 = er.start_vectors(m ** 3, K)
    if mass_name == "mass27":
        s = np.sin(np.pi * np.arange(1, m + 1) / (m + 1.0))
        X0[:, 0] = np.kron(np.kron(s, s), s)
    return X0


def stop_defects(s, B):
    """-> (max |W^T B W - I| on the active columns, max |X^T B W|) of a stopped solve's dict (the reference's or the GPU's vectors)"""
    act = s["act"]
    BW = B @ s["W"]
    G = s["W"][:, act].T @ BW[:, act]
    return float(np.max(np.abs(G - np.eye(len(act))))), float(np.max(np.abs(s["X"].T @ BW)))


def bw_bound(B, W, Tw, K):
    """entrywise bound of |BW - B W| for the carried BW of a stopped solve.  With W' the projected W before its orthonormalisation,
    the solver forms W = fl(W' T) and BW = fl(fl(B W') T): to first order |W - W' T| <= K u |W'||T| and
    |BW - B W' T| <= (r + K) u |B||W'||T|, r the longest row of B, so |BW - B W| <= (r + 2 K) u |B||W'||T|, and since W' = W T^-1 up to
    rounding, |W'||T| <= |W| M with M = |T^-1||T| on the active columns.  T is the reference's (the GPU's differs from it by rounding),
    and the bound is taken twice for that and for the second-order terms"""
    act = [j for j in range(K) if Tw[j, j] != 0.0]
    M = np.zeros((K, K))
    Ta = Tw[np.ix_(act, act)]
    M[np.ix_(act, act)] = np.abs(np.linalg.inv(Ta)) @ np.abs(Ta)
    r = int(np.diff(B.tocsr().indptr).max())
    return 2.0 * (r + 2 * K) * U * (abs(B) @ (np.abs(W) @ M))


def ortho_defect(X, B):
    return float(np.max(np.abs(X.T @ (B @ X) - np.eye(X.shape[1]))))
