"""References and inputs for the FGMRES tests (test infrastructure: numpy/scipy only, no GPU, no oracle).

The nonsymmetric operator convdiff(n, pe), its scipy hierarchy (the construction of tests/hierarchy.py) with a numpy V-cycle, a
float64 numpy restarted flexible GMRES with the structure of sgpu_solve_FGMRES (the preconditioner a callable, the dot product
pluggable), and float64 numpy restatements of the two Gram-Schmidt kernels of saena_amd/csrc/kernels_gmres.hip.h: the dots'
summation order with its error bound, and the update.  tests/test_gmres_ref.py shows on the CPU that a correct implementation
stays inside every bound tests/test_gpu_gmres.py asserts.
"""
import numpy as np
import scipy.sparse as sp

from tests import solver_ref as sr

U = sr.U
BLOCK = sr.BLOCK
GS_C = 8                              # columns per pass of the Gram-Schmidt kernels
GS_MAXBLK = 1024                      # most blocks of a pass
GS_WRAP = 2 * BLOCK * GS_MAXBLK       # first row of the second grid-stride trip (rows are walked in pairs)
TOL_HIST = 1e-10                      # of ||r_0||; and 1e-6 of the entry's own size (the block pCG contract's bound)


# ---------------------------------------------------------------------------
# inputs
def convdiff(n, pe):
    """n^3 rows: the 7-point Laplacian plus pe times an upwinded convection (1, 0.5, 0.25 along x, y, z)"""
    I = sp.identity(n, format="csr")
    D = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1], format="csr")
    Cm = sp.diags([np.full(n - 1, -1.0), np.full(n, 1.0)], [-1, 0], format="csr")
    k3 = lambda a, b, c: sp.kron(sp.kron(a, b), c)      # noqa: E731
    A = k3(I, I, D) + k3(I, D, I) + k3(D, I, I) + pe * (k3(I, I, Cm) + 0.5 * k3(I, Cm, I) + 0.25 * k3(Cm, I, I))
    A = A.tocsr()
    A.sort_indices()
    return A


def rhs_for(n):
    i = np.arange(n, dtype=np.float64)
    return np.sin(0.37 * i) + 0.2 * np.cos(1.3 * i) + 0.05


def aggregate_hierarchy(A0, n, omega=2.0 / 3, coarsest=64):
    """tests/hierarchy.poisson_hierarchy's construction on any operator of an n^3 grid: 2x2x2 aggregates, one damped-Jacobi step on
    P, R = P^T, Ac = R A P, until a level has at most `coarsest` rows.  -> As, Ps, Rs (scipy CSR)"""
    As, Ps, Rs = [A0], [], []
    dims = (n, n, n)
    while As[-1].shape[0] > coarsest:
        A = As[-1]
        nx, ny, nz = dims
        cx, cy, cz = (nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        agg = ((k // 2) * cy + (j // 2)) * cx + (i // 2)
        T = sp.csr_matrix((np.ones(A.shape[0]), (np.arange(A.shape[0]), agg.ravel())), shape=(A.shape[0], cx * cy * cz))
        P = (T - omega * (sp.diags(1.0 / A.diagonal()) @ A @ T)).tocsr()
        P.eliminate_zeros()
        R = P.T.tocsr()
        Ac = (R @ A @ P).tocsr()
        Ac.eliminate_zeros()
        for M in (P, R, Ac):
            M.sort_indices()
        Ps.append(P); Rs.append(R); As.append(Ac)
        dims = (cx, cy, cz)
    return As, Ps, Rs


_cache = {}


def case(n, pe):
    """-> dict(A, As, Ps, Rs, rhs) of convdiff(n, pe), computed once and shared: treat as read-only"""
    if (n, pe) not in _cache:
        A = convdiff(n, pe)
        As, Ps, Rs = aggregate_hierarchy(A, n)
        b = rhs_for(A.shape[0])
        b.setflags(write=False)
        _cache[(n, pe)] = dict(A=A, As=As, Ps=Ps, Rs=Rs, rhs=b)
    return _cache[(n, pe)]


def vcycle(As, Ps, Rs, rhs, pre=3, post=3, omega=2.0 / 3):
    """one V-cycle from a zero iterate: damped Jacobi (pre, post), dense solve on the coarsest level"""
    def level(l, b):
        A = As[l]
        if l == len(As) - 1:
            return np.linalg.solve(A.toarray(), b)
        w = omega / A.diagonal()
        u = np.zeros_like(b)
        for _ in range(pre):
            u = u - w * (A @ u - b)
        u = u + Ps[l] @ level(l + 1, Rs[l] @ (b - A @ u))
        for _ in range(post):
            u = u - w * (A @ u - b)
        return u
    return level(0, np.asarray(rhs, np.float64))


def pcg(A, b, precond, tol=1e-8, max_iter=100):
    """sgpu_solve_pCG's recurrence in numpy -> (iterations, converged, smallest ||r|| / ||r_0|| seen)"""
    u = np.zeros_like(b)
    r = A @ u - b
    init = float(r @ r)
    thr = init * tol * tol
    rho = precond(r)
    p = rho.copy()
    rr = float(r @ rho)
    best = 1.0
    for i in range(max_iter):
        hh = A @ p
        alpha = rr / float(p @ hh)
        u -= alpha * p
        r -= alpha * hh
        cur = float(r @ r)
        best = min(best, np.sqrt(cur / init))
        if cur < thr:
            return i + 1, True, best
        rho = precond(r)
        rr_new = float(r @ rho)
        p = rho + (rr_new / rr) * p
        rr = rr_new
    return max_iter, False, best


# ---------------------------------------------------------------------------
# the Gram-Schmidt kernels, restated
def gs_blocks(n):
    return min(GS_MAXBLK, max(1, -(-(n // 2) // BLOCK)))


def gs_dot_blocked(x, y):
    """k_gs_dots_partial + k_gs_reduce on one column, in float64 numpy: nb blocks of 256 threads; thread (b, t) owns the row pairs
    b*256 + t + k*256*nb in order of k and adds a pair's two products one after the other; thread 0 of block 0 then adds the last
    row of an odd n; block_sum; one block adds the nb partials the way sgpu_dot's second kernel does"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = len(x)
    n2 = n // 2
    nb = gs_blocks(n)
    trips = max(1, -(-n2 // (BLOCK * nb)))
    prod = np.zeros((2, trips * nb * BLOCK))
    prod[0, :n2] = x[0:2 * n2:2] * y[0:2 * n2:2]
    prod[1, :n2] = x[1:2 * n2:2] * y[1:2 * n2:2]
    prod = prod.reshape(2, trips, nb, BLOCK)
    s = np.zeros((nb, BLOCK))
    for k in range(trips):
        s = s + prod[0, k]
        s = s + prod[1, k]
    if n & 1:
        s[0, 0] = s[0, 0] + x[n - 1] * y[n - 1]
    partial = sr._block_sums(s)
    trips2 = -(-nb // BLOCK)
    p = np.zeros(trips2 * BLOCK)
    p[:nb] = partial
    p = p.reshape(trips2, BLOCK)
    s2 = np.zeros((1, BLOCK))
    for k in range(trips2):
        s2 = s2 + p[k]
    return float(sr._block_sums(s2)[0])


def gs_roundings(n):
    """Roundings on the longest path from an input element to a coefficient, plus one for rounding the reference to float64: a
    thread's two adds per trip, the last row of an odd n, the product, the 64-lane butterfly (6), the 4 wave sums, then in the
    second kernel a thread's adds of the partials, the butterfly, the 4 wave sums"""
    nb = gs_blocks(n)
    trips = max(1, -(-(n // 2) // (BLOCK * nb)))
    return 2 * trips + 1 + 1 + 6 + 4 + -(-nb // BLOCK) + 6 + 4 + 1


def gs_dot_bound(x, y):
    """|got - ref| <= k u sum|x_i y_i| / (1 - k u), k = gs_roundings(n)"""
    k = gs_roundings(len(x))
    s = float(np.sum(np.abs(np.asarray(x, np.longdouble) * np.asarray(y, np.longdouble))))
    return k * U * s / (1 - k * U)


def gs_update(V, h, w):
    """k_gs_update: w - sum_c h[c] V[:, c] in ascending c, each product rounded, then subtracted (whatever the chunking)"""
    w = np.array(w, np.float64)
    for c in range(len(h)):
        w = w - np.float64(h[c]) * V[:, c]
    return w


def dot64(x, y):
    return float(np.dot(x, y))


def dot_ld(x, y):
    return float(sr.dot_hp(x, y))


# ---------------------------------------------------------------------------
# the solver
def fgmres(A, b, restart, tol=1e-8, max_iter=100, precond=None, dot=dot64):
    """sgpu_solve_FGMRES in float64 numpy.  precond: callable r -> z (None: the identity), dot: callable (x, y) -> float.
    -> dict(u, iters, hist, true_res, converged, restarts).  hist[0] = ||r_0||, hist[k] = |g_{j+1}| after inner iteration k; per inner
    iteration classical Gram-Schmidt twice, the Hessenberg column h1 + h2, Givens rotations; the estimate is tested before v_{j+1} is
    formed; at the end of a cycle u += Z y, r = b - A u recomputed, and only that recomputed dot declares convergence."""
    b = np.asarray(b, np.float64)
    n, m = len(b), int(restart)
    u = np.zeros(n)
    r = b - A @ u
    init = dot(r, r)
    hist = [np.sqrt(init)]
    out = dict(u=u, iters=0, hist=np.array(hist), true_res=np.sqrt(init), converged=True, restarts=0)
    if init == 0.0:
        return out
    thr = init * tol * tol
    cur, k, conv, cycles = init, 0, False, 0
    while k < max_iter:
        cycles += 1
        V = np.zeros((n, m + 1))
        Z = np.zeros((n, m))
        H = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        V[:, 0] = r / np.sqrt(cur)
        g[0] = np.sqrt(cur)
        jj = 0
        for j in range(m):
            if k >= max_iter:
                break
            z = V[:, j] if precond is None else precond(V[:, j])
            Z[:, j] = z
            w = A @ z
            nc = j + 1
            h1 = np.array([dot(V[:, c], w) for c in range(nc)])
            w = gs_update(V, h1, w)
            h2 = np.array([dot(V[:, c], w) for c in range(nc)])
            w = gs_update(V, h2, w)
            nrm2 = dot(w, w)
            hc = np.zeros(m + 1)
            hc[:nc] = h1 + h2
            hc[nc] = np.sqrt(nrm2)
            for i in range(j):
                t = cs[i] * hc[i] + sn[i] * hc[i + 1]
                hc[i + 1] = cs[i] * hc[i + 1] - sn[i] * hc[i]
                hc[i] = t
            d = np.sqrt(hc[j] * hc[j] + hc[j + 1] * hc[j + 1])
            if not d > 0.0:
                raise ArithmeticError("breakdown")
            cs[j], sn[j] = hc[j] / d, hc[j + 1] / d
            hc[j], hc[j + 1] = d, 0.0
            g[j + 1] = -(sn[j] * g[j])
            g[j] = cs[j] * g[j]
            H[:, j] = hc
            k += 1
            jj = j + 1
            hist.append(abs(g[j + 1]))
            if g[j + 1] * g[j + 1] < thr or j + 1 == m or k == max_iter:
                break
            if not nrm2 > 0.0:
                raise ArithmeticError("zero norm without convergence")
            V[:, j + 1] = w / np.sqrt(nrm2)
        y = np.zeros(jj)
        for i in range(jj - 1, -1, -1):
            s = g[i]
            for c in range(i + 1, jj):
                s -= H[i, c] * y[c]
            y[i] = s / H[i, i]
        u = gs_update(Z[:, :jj], -y, u)
        r = b - A @ u
        cur = dot(r, r)
        if cur < thr:
            conv = True
            break
    return dict(u=u, iters=k, hist=np.array(hist), true_res=float(np.sqrt(cur)), converged=conv, restarts=cycles - 1)


def monotone_within_cycles(hist, restart, slack=1e-12):
    """a minimal-residual method: within a cycle (entries k*restart .. (k+1)*restart) no estimate exceeds the one before it by
    more than slack ||r_0||.  The first entry of a later cycle is an estimate (the cycle itself starts from the recomputed residual)
    and is compared within its own cycle only"""
    hist = np.asarray(hist)
    for a in range(0, len(hist) - 1, restart):
        seg = hist[a if a == 0 else a + 1:a + restart + 1]
        if len(seg) > 1 and np.any(np.diff(seg) > slack * hist[0]):
            return False
    return True


def hist_within(got, ref):
    """the bound of the GPU test: every entry within TOL_HIST ||r_0|| of the reference's, and within 1e-6 of its own size"""
    got, ref = np.asarray(got), np.asarray(ref)
    n = min(len(got), len(ref))
    d = np.abs(got[:n] - ref[:n])
    return bool(np.all(d <= TOL_HIST * ref[0]) and np.all(d <= 1e-6 * ref[:n]))
