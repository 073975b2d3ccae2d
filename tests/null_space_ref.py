"""Operators with the constant null space, references and numpy restatements for the tests of sgpu_amg_create_null_space
(test infrastructure: numpy/scipy and the host-only setup library, no GPU, no oracle).

  neumann3d, wgrid, path   symmetric operators with A 1 = 0; pinned(A): the same with row 0 pinned (nonsingular)
  center                   k_sum_partial + k_reduce_partials + k_center: x - dot_blocked(x, 1) / n
  pinv                     saena_amd/csrc/coarse_pinv.h: solver_ref.gauss_jordan_inverse on A + (s / n) 1 1^T, s the mean of the
                           diagonal, then every column and then every row has its mean taken off (sequential sums)
  solve_plus               the reference: solver_ref.solve_hp on the bordered system [[A, 1], [1^T, 0]] -> A^+ b, zero mean
  vcycle, pcg, ...         the V-cycle (Jacobi / Chebyshev as jacobi_pp / cheby_pp state them, the coarsest solve restricted to the
                           complement of constants) and the solvers of include/saena_gpu.h on the centred right-hand side

Hierarchies come from the product's own host setup (OPTIONS001, set_remove_boundary(False)); tests/test_null_space_ref.py shows on the
CPU that the restatements stay inside every bound tests/test_gpu_null_space.py asserts.
"""
import numpy as np
import scipy.sparse as sp

from tests import degenerate_ref as dg, solver_ref as sr

U = sr.U
OMEGA = float(np.float32(2.0 / 3.0))     # JACOBI_OMEGA_REF
DEFECT_MAX = 1e-10                       # sgpu_amg_create_null_space's threshold on max|A 1| / max|a_ii|
TOL = 1e-8                               # OPTIONS001's relative_tol
MAX_ITER = 50

# n of the centring kernels' tests: wave and block edges, 1 024 blocks exactly, the second grid-stride trip (262 145)
CENTER_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 100003, 262144, 262145)
PATH_SIZES = (9, 65, 257, 1024)
# name -> (generator, setup option overrides): the hierarchies of the GPU tests
HIERARCHIES = {
    "neumann8": (lambda: neumann3d(8), {}),                                         # 512 rows
    "neumann16": (lambda: neumann3d(16), {}),                                       # 4 096 rows
    "wgrid40": (lambda: wgrid(40, 5), {}),                                          # 1 600 rows
    "neumann16cut": (lambda: neumann3d(16), dict(max_level=1, dynamic_levels=0)),   # coarsest level past 1 024 rows
}
EIG_BOX = (12, 8, 5)                     # the Neumann box of the eigenpair test: lambda_2 and lambda_3 are simple
HIERARCHIES["neumann12x8x5"] = (lambda: neumann3d(*EIG_BOX), {})
SOLVE_HIERARCHIES = ("neumann8", "neumann16", "wgrid40", "neumann16cut")
# sgpu_solve_smoother has no coarse correction: three Jacobi sweeps take a factor of about (1 - omega lambda_2 / a_ii)^3 off the error,
# a few hundred iterations to 1e-8 at 8^3 and tens of thousands on wgrid(40) (lambda_2 = 0.004): it is solved on the first only
SMOOTHER_HIERARCHIES = ("neumann8",)

_cache = {}


# ---------------------------------------------------------------------------
# operators
def _grid_laplacian(shape, weights=None):
    idx = np.arange(int(np.prod(shape))).reshape(shape[::-1])            # x fastest
    a, b = [], []
    for ax in range(len(shape)):
        lo = [slice(None)] * len(shape); hi = [slice(None)] * len(shape)
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        a.append(idx[tuple(lo)].ravel()); b.append(idx[tuple(hi)].ravel())
    a, b = np.concatenate(a), np.concatenate(b)
    w = np.ones(len(a)) if weights is None else weights(len(a))
    n = idx.size
    W = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n)).tocsr()
    A = (sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()
    A.sort_indices()
    return A


def neumann3d(nx, ny=None, nz=None):
    """7-point Laplacian of an nx x ny x nz box with Neumann boundaries (the graph Laplacian of the grid): eigenvalues
    sum over the axes of 2 - 2 cos(k pi / n)"""
    ny = nx if ny is None else ny
    nz = nx if nz is None else nz
    return _grid_laplacian((nx, ny, nz))


def wgrid(m, seed):
    """graph Laplacian of the m x m grid with seeded edge weights 0.5 + U[0, 1)"""
    rng = np.random.default_rng(seed)
    return _grid_laplacian((m, m), lambda k: 0.5 + rng.random(k))


def path(n):
    """diagonal 1, 2, ..., 2, 1, off-diagonals -1: every entry exact, an exact zero pivot for the plain elimination"""
    return _grid_laplacian((n,))


def pinned(A):
    """row and column 0 cleared, a_00 = 1: the usual way to make such a system nonsingular.  max|A 1| / max|a_ii| is 1 / max a_ii"""
    D = A.tolil(copy=True)
    D[0, :] = 0.0
    D[:, 0] = 0.0
    D[0, 0] = 1.0
    D = D.tocsr()
    D.eliminate_zeros()
    D.sort_indices()
    return D


def defect(A):
    """max_i |(A 1)_i| / max_i |a_ii|"""
    return float(np.max(np.abs(A @ np.ones(A.shape[1]))) / np.max(np.abs(A.diagonal())))


def rhs_for(n):
    """solver_ref.rhs_for: smooth, sign-changing, mean about -0.3 -- not consistent with a singular system as it stands"""
    return sr.rhs_for(n)


# ---------------------------------------------------------------------------
# the kernels and the host header, restated
def center(x):
    """sgpu_vec_center: x - S / n, S in sgpu_dot's order of summation -> (y, mean)"""
    x = np.asarray(x, np.float64)
    mean = np.float64(sr.dot_blocked(x, np.ones(len(x)))) / np.float64(len(x))
    return x - mean, float(mean)


def shifted(D):
    """-> (A + (s / n) 1 1^T, s), s the mean of the diagonal summed in index order"""
    D = np.asarray(D, np.float64)
    n = D.shape[0]
    tr = np.float64(0.0)
    for i in range(n):
        tr = tr + D[i, i]
    s = tr / np.float64(n)
    return D + s / np.float64(n), float(s)


def pinv(D):
    """coarse_pinv::pseudo_inverse, rounding for rounding"""
    S, _ = shifted(D)
    M, _ = sr.gauss_jordan_inverse(S)
    n = M.shape[0]
    col = np.zeros(n)
    for i in range(n):
        col = col + M[i]
    M = M - (col / np.float64(n))[None, :]
    row = np.zeros(n)
    for j in range(n):
        row = row + M[:, j]
    return M - (row / np.float64(n))[:, None]


def solve_plus(A, b):
    """A^+ b by solver_ref.solve_hp on [[A, 1], [1^T, 0]] -> (x of zero mean, the bordered system's relative residual)"""
    D = A.toarray() if sp.issparse(A) else np.asarray(A, np.float64)
    n = D.shape[0]
    K = np.zeros((n + 1, n + 1))
    K[:n, :n] = D
    K[:n, n] = 1.0
    K[n, :n] = 1.0
    x, resid = sr.solve_hp(K, np.concatenate([np.asarray(b, np.float64), [0.0]]))
    return x[:n], resid


def pinv_bound(n, cond_shifted):
    """||u - x+|| / ||x+|| of u = pinv(A) rhs: solver_ref.direct_bound with the shifted matrix's condition number, plus the centrings'
    rounding -- two sequential sums of n terms and two subtractions on entries of size ||(A + s z z^T)^-1|| <= cond / s, applied to a
    right-hand side: 4 (n + 2) u cond"""
    return sr.direct_bound(n, cond_shifted) + 4 * (n + 2) * U * cond_shifted


def spectrum(A):
    """-> (lambda_2, lambda_max) of a connected graph Laplacian (lambda_1 = 0), by numpy"""
    import hashlib
    A = A.tocsr()
    key = ("spec", A.shape, hashlib.sha256(A.indptr.tobytes() + A.indices.tobytes() + A.data.tobytes()).hexdigest())
    if key not in _cache:
        if A.shape[0] <= 2048:
            lam = np.linalg.eigvalsh(A.toarray())
            _cache[key] = (float(lam[1]), float(lam[-1]))
        else:
            import scipy.sparse.linalg as sla
            top = sla.eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-10)
            low = sla.eigsh(A + 1e-2 * sp.identity(A.shape[0]), k=2, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-10)
            _cache[key] = (float(np.sort(low)[1] - 1e-2), float(top[0]))
    return _cache[key]


def error_bound(A, tol=TOL):
    """||u - x+|| / ||x+|| <= 1.01 tol lambda_max / lambda_2: ||e|| <= ||r|| / lambda_2 and ||x+|| >= ||b~|| / lambda_max"""
    l2, lmax = spectrum(A)
    return 1.01 * tol * lmax / l2


# ---------------------------------------------------------------------------
# hierarchies of the product's host setup
def _csr(d, ncols):
    ptr = np.concatenate([[0], np.cumsum(d["nnzPerRow_local"], dtype=np.int64)])
    return sp.csr_matrix((d["val_local"].astype(np.float64), d["col_local"].astype(np.int32), ptr), shape=(int(d["M"]), int(ncols)))


def hierarchy(name):
    """-> dict(A, P, R: scipy CSR per level, from the setup's own arrays; eig: the setup's eig_max per level; A0: the generator's
    matrix).  Built once with Chebyshev options so that eig_max exists; the operators do not depend on the smoother.  Treat as
    read-only"""
    if ("hier", name) not in _cache:
        from saena_amd import host
        gen, over = HIERARCHIES[name]
        A0 = gen()
        L = host.load("host")
        M = host.Matrix(host.Comm("host", "self"))
        M.set_remove_boundary(False)
        coo = A0.tocoo()
        M.set_many(coo.row.astype(np.int32), coo.col.astype(np.int32), coo.data)
        M.assemble()
        S = host.AmgSolver(M, host.options(L, **dict(host.OPTIONS001, smoother="chebyshev", **over)))
        nl = S.num_levels
        H = dict(A=[], P=[], R=[], eig=[], A0=A0, name=name)
        for l in range(nl):
            d = S.level_layout(l, 0)
            H["A"].append(_csr(d, d["M"])); H["eig"].append(S.level_info(l)["eig_max"])
        for l in range(nl - 1):
            dp, dr = S.level_layout(l, 1), S.level_layout(l, 2)
            H["P"].append(_csr(dp, H["A"][l + 1].shape[0]))
            H["R"].append(_csr(dr, H["A"][l].shape[0]))
        _cache[("hier", name)] = H
    return _cache[("hier", name)]


def one_level(A):
    """the one-level hierarchy ([A], [], []) in hierarchy()'s form"""
    return dict(A=[A.tocsr()], P=[], R=[], eig=[0.0], A0=A, name="one_level")


def coarse_pinv(H):
    """pinv of the coarsest operator of H, computed once"""
    key = ("pinv", id(H))
    if key not in _cache:
        _cache[key] = (H, pinv(H["A"][-1].toarray()))
    return _cache[key][1]


# ---------------------------------------------------------------------------
# the V-cycle and the solvers, restated (the residual is A u - rhs and corrections are subtracted, as in the library)
def coarsest(H, rhs, coarse, u0=None):
    """-> (u, iterations): "direct" up to 1 024 rows: pinv(A_c) rhs (the iterate is overwritten); otherwise ("cg", "device_cg", the
    fallback of "direct") solver_ref.coarsest_cg from u0 on the centred right-hand side"""
    Ac = H["A"][-1]
    if coarse == "direct" and Ac.shape[0] <= sr.CG_MAXN:
        return coarse_pinv(H) @ rhs, 0
    return sr.coarsest_cg(Ac, center(rhs)[0], u0=u0)


def smooth(H, l, sweeps, u, rhs, smoother):
    A, inv = H["A"][l], 1.0 / H["A"][l].diagonal()
    if smoother == "jacobi":
        for _ in range(sweeps):
            u = u - (A @ u - rhs) * (inv * OMEGA)
        return u
    eig = H["eig"][l]
    alpha, beta = 0.13 * eig, eig
    delta, theta = (beta - alpha) / 2.0, (beta + alpha) / 2.0
    s1 = theta / delta
    rhok = 1.0 / s1
    d = None
    for i in range(sweeps):
        if i == 0:
            d = ((1.0 / theta) * inv) * (rhs - A @ u)
        else:
            rhokp1 = 1.0 / (2.0 * s1 - rhok)
            d = (rhokp1 * rhok) * d + ((2.0 * rhokp1 / delta) * inv) * (rhs - A @ u)
            rhok = rhokp1
        u = u + d
    return u


def vcycle(H, rhs, smoother="jacobi", coarse="direct", u=None, pre=3, post=3):
    def level(l, u, b):
        if l == len(H["A"]) - 1:
            return coarsest(H, b, coarse, u0=u)[0]
        u = smooth(H, l, pre, u, b, smoother)
        e = level(l + 1, np.zeros(H["A"][l + 1].shape[0]), H["R"][l] @ (H["A"][l] @ u - b))
        u = u - H["P"][l] @ e
        return smooth(H, l, post, u, b, smoother)
    rhs = np.asarray(rhs, np.float64)
    return level(0, np.zeros(len(rhs)) if u is None else u, rhs)


def _finish(u, hist, conv):
    return dict(u=center(u)[0], iters=len(hist) - 1, hist=np.array(hist), converged=conv, stopped=None)


def _nonfinite(u, hist):
    """rule 3 of include/saena_gpu.h's "Degenerate right-hand sides": stopped where the dot is not finite, u as it is (not centred)"""
    return dict(u=u, iters=len(hist) - 1, hist=np.array(hist), converged=False, stopped="nonfinite")


def pcg(H, rhs, smoother="jacobi", coarse="direct", tol=TOL, max_iter=MAX_ITER, precond=True):
    """sgpu_solve_pCG (precond) / sgpu_solve_CG under null_space 1: r_0 centred, nothing centred per iteration, u centred at the end"""
    A = H["A"][0]
    M = (lambda r: vcycle(H, r, smoother, coarse)) if precond else (lambda r: r)
    u = np.zeros(A.shape[0])
    r, mean = center(-np.asarray(rhs, np.float64))
    init = float(r @ r)
    kind = dg.at_start(init, len(r), mean, null_space=True)          # rules 1 to 3 at iteration 0
    if kind:
        return dg.start_result(kind, len(r), init)
    hist, thr = [np.sqrt(init)], init * tol * tol
    rho = M(r)
    p = rho.copy()
    rr = float(r @ rho)
    conv = False
    for _ in range(max_iter):
        hh = A @ p
        alpha = rr / float(p @ hh)
        u = u - alpha * p
        r = r - alpha * hh
        cur = float(r @ r)
        hist.append(np.sqrt(cur))
        if cur < thr:
            conv = True
            break
        if not np.isfinite(cur):
            return _nonfinite(u, hist)
        rho = M(r)
        rr_new = float(r @ rho)
        p = rho + (rr_new / rr) * p
        rr = rr_new
    return _finish(u, hist, conv)


def stationary(H, rhs, smoother="jacobi", coarse="direct", tol=TOL, max_iter=MAX_ITER, with_coarse=True, pre=3):
    """sgpu_solve (V-cycles) / sgpu_solve_smoother (pre sweeps of the smoother) under null_space 1: the right-hand side is centred once"""
    A = H["A"][0]
    b, mean = center(np.asarray(rhs, np.float64))
    u = np.zeros(A.shape[0])
    r = A @ u - b
    init = float(r @ r)
    kind = dg.at_start(init, len(b), mean, null_space=True)
    if kind:
        return dg.start_result(kind, len(b), init)
    hist, thr = [np.sqrt(init)], init * tol * tol
    conv = False
    for _ in range(max_iter):
        u = vcycle(H, b, smoother, coarse, u=u) if with_coarse else smooth(H, 0, pre, u, b, smoother)
        r = A @ u - b
        cur = float(r @ r)
        hist.append(np.sqrt(cur))
        if cur < thr:
            conv = True
            break
        if not np.isfinite(cur):
            return _nonfinite(u, hist)
    return _finish(u, hist, conv)


def lobpcg_constant_locked(H, K, nev, smoother="jacobi", coarse="direct"):
    """eig_lock_ref.lobpcg_locked on level 0 of H with the normalised constant vector as its one locked column, the generated start
    block and this module's V-cycle as the preconditioner: the smallest nonzero eigenpairs"""
    from tests import eig_lock_ref as lr
    A = H["A"][0]
    n = A.shape[0]
    q = np.full((n, 1), 1.0 / np.sqrt(n))
    M = lambda R: np.stack([vcycle(H, R[:, j], smoother, coarse) for j in range(R.shape[1])], axis=1)      # noqa: E731
    return lr.lobpcg_locked(A, None, lr.start_block(n, K)[0], nev, q, q, precond=M)
