"""References, inputs and bounds for the tests of LOBPCG with hard locking (test infrastructure: numpy/scipy only, no GPU, no oracle).

A float64 numpy restatement of sgpu_eigs_LOBPCG_locked and of the driver sgpu_eigs_LOBPCG_many (saena_amd/csrc/sgpu_eig_lock.hip.inc),
step for step, from eig_ref's and geig_ref's pieces; the restatements of k_lock_gram_partial, k_lock_project and the refill generator
(saena_amd/csrc/kernels_eig_lock.hip.h); the sweep bookkeeping of saena_amd/csrc/eig_lock_plan.h; and the bounds
tests/test_gpu_eig_lock.py asserts.  tests/test_eig_lock_ref.py shows on the CPU that a correct implementation stays inside every one
of them, and pins the numbers recorded below: they are this reference's, never the GPU's.
"""
import numpy as np
import scipy.linalg

from tests import eig_ref as er, geig_ref as gr, solver_ref as sr

TOL = er.TOL
MAX_LOCKED = 64
LOCK_C = 8
# the shapes of the GPU tests: ((m, K, nev, sweep_nev), mass or None).  8^3 is the smallest with a two-level hierarchy; nev = 20 at
# sweep_nev = 4 forces five sweeps and cuts clusters of the spectrum (1 + 3 + 3 + 1 + 6 + 3 + 3 ...)
SHAPES = (((8, 8, 20, 4), None), ((8, 4, 12, 2), None), ((16, 8, 24, 4), None), ((8, 8, 20, 4), "mass27"), ((8, 4, 12, 2), "lumped"))
MAX_ITER = 400

# ---- recorded by tests/test_eig_lock_ref.py (which asserts that the reference still gives them) ----
# total iterations over all sweeps, and the number of sweeps, of the reference to TOL with the V-cycle (Jacobi 3 + 3, direct coarsest)
ITERS = {SHAPES[0]: 65, SHAPES[1]: 67, SHAPES[2]: 90, SHAPES[3]: 64, SHAPES[4]: 106}
SWEEPS = {SHAPES[0]: 5, SHAPES[1]: 6, SHAPES[2]: 6, SHAPES[3]: 5, SHAPES[4]: 6}
# (per sweep: 13 + 8 + 14 + 7 + 23; 15 + 4 + 17 + 6 + 16 + 9; 16 + 10 + 16 + 10 + 26 + 12; 13 + 8 + 13 + 7 + 23; 17 + 13 + 14 + 22 + 21 + 19)
# max |Q^T B Q - I| of the reference's result
ORTHO = {SHAPES[0]: 2.0e-15, SHAPES[1]: 2.3e-15, SHAPES[2]: 1.8e-15, SHAPES[3]: 2.5e-15, SHAPES[4]: 1.4e-15}
ORTHO_MARGIN = er.ORTHO_MARGIN


def iteration_bound(shape):
    """ceil(1.25 x the reference's total) + 2 x the reference's sweeps: eig_ref.iteration_bound's rule applied per sweep"""
    return int(np.ceil(1.25 * ITERS[shape])) + 2 * SWEEPS[shape]


# ---------------------------------------------------------------------------
# the kernels, restated
def lock_gram(Z, Y):
    """k_lock_gram_partial + k_gram_reduce: C[l, b] = sum_i Z[i, l] Y[i, b] in sgpu_dot's order of summation (solver_ref.dot_blocked):
    an entry depends on its two columns alone"""
    return np.array([[sr.dot_blocked(Z[:, l], Y[:, b]) for b in range(Y.shape[1])] for l in range(Z.shape[1])]).reshape(Z.shape[1], Y.shape[1])


def lock_project(Q, C, W):
    """k_lock_project: W[i, b] <- (sum_l Q[i, l] (-C[l, b]) from 0.0, l ascending, every product rounded, then added) + W[i, b], W last"""
    out = np.zeros_like(np.asarray(W, np.float64))
    Cm = np.asarray(C, np.float64)
    for l in range(Q.shape[1]):
        out = out + Q[:, l:l + 1] * (-Cm[l:l + 1, :])
    return out + W


def refill(n, counter):
    """k_block_refill: lock_hash(row, counter) for the rows 0 .. n-1, exact in [-1, 1)"""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((int(counter) + 1) * 0xD1B54A32D192ED03 % 2 ** 64)
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


# ---------------------------------------------------------------------------
# the sweep bookkeeping (eig_lock_plan.h)
def default_sweep_nev(K):
    return max(1, K // 2)


def sweep_want(nev, nlocked, sweep_nev):
    return max(0, min(sweep_nev, nev - nlocked))


def sweep_take(K, nev, nlocked, leading):
    return max(0, min(leading, K, nev - nlocked))


def refill_plan(take, counter):
    """-> ([(column, counter value)], the advanced counter)"""
    return [(j, counter + j) for j in range(take)], counter + max(0, take)


def final_order(lam):
    """perm[k] = the locked column that goes to position k: ascending, stable"""
    return [int(i) for i in np.argsort(np.asarray(lam, np.float64), kind="stable")]


# ---------------------------------------------------------------------------
# the constrained solve
def lobpcg_locked(A, B, X0, nev, Q=None, BQ=None, tol=TOL, max_iter=100, precond=None):
    """sgpu_eigs_LOBPCG_locked in float64 numpy, step for step: eig_ref.lobpcg (B None) or geig_ref.lobpcg_gen with X projected twice
    against the locked set before the start orthonormalisation and W once right after W = M R.  Q (n, L) or None; BQ = B Q.
    -> dict(X, BX, lam, res, iters, hist, converged, leading)"""
    gen = B is not None
    L = 0 if Q is None else Q.shape[1]
    Z = BQ if gen else Q

    def project(V):
        return lock_project(Q, Z.T @ V, V) if L else V

    def mul_B(V):
        return B @ V if gen else V                             # (the standard problem: BV IS V, the same array)

    def mix_B(BV, V_new, T):
        return er.block_mix([BV], [T]) if gen else V_new

    X = np.array(X0, np.float64)
    n, K = X.shape
    every = list(range(K))
    X = project(project(X))
    BX = mul_B(X)
    T = er.ortho_factor(X.T @ BX, every, K)
    if T is None:
        raise ValueError("X^T B X is not positive definite")
    Xn = er.block_mix([X], [T])
    X, BX = Xn, mix_B(BX, Xn, T)
    AX = A @ X
    H = X.T @ AX
    lam, Qr = np.linalg.eigh(0.5 * (H + H.T))
    Xn = er.block_mix([X], [Qr])
    if gen:
        X, AX, BX = Xn, er.block_mix([AX], [Qr]), er.block_mix([BX], [Qr])
    else:
        X, AX = Xn, er.block_mix([AX], [Qr])
        BX = X
    P = AP = BP = None
    it, fresh, hist = 0, False, []

    def precondition(R):
        W = R.copy() if precond is None else precond(R)
        W = project(W)
        return W, BX.T @ W

    while True:
        if gen:
            R, rr, bb = gr.geig_residual(AX, BX, lam)
        else:
            R = er.eig_residual(AX, X, lam)
            rr, bb = np.sum(R * R, axis=0), None
        if not fresh:
            W, XtW = precondition(R)
        if len(hist) > it:
            hist[it] = np.sqrt(rr)
        else:
            hist.append(np.sqrt(rr))
        if gen:
            act = [j for j in range(K) if not rr[j] < tol * tol * lam[j] * lam[j] * bb[j]]
        else:
            act = [j for j in range(K) if not rr[j] < tol * tol * lam[j] * lam[j]]
        conv = not any(j < nev for j in act)
        if conv or it >= max_iter:
            if fresh:
                return dict(X=X, BX=BX, lam=lam, res=np.sqrt(rr), iters=it, hist=np.array(hist), converged=conv,
                            leading=act[0] if act else K)
            AX = A @ X
            BX = mul_B(X)
            fresh = True
            continue
        if fresh:
            W, XtW = precondition(R)
            fresh = False
        Cw = np.zeros((K, K))
        Cw[:, act] = -XtW[:, act]
        W = er.block_mix([X], [Cw], add=W)
        BW = mul_B(W)
        Tw = er.ortho_factor(W.T @ BW, act, K)
        if Tw is None:
            raise er.Breakdown(f"W^T B W is not positive definite at iteration {it + 1}")
        Tp = er.ortho_factor(P.T @ BP, act, K) if P is not None else None
        useP = Tp is not None
        Wn = er.block_mix([W], [Tw])
        W, BW = Wn, mix_B(BW, Wn, Tw)
        AW = A @ W
        if useP:
            Pn = er.block_mix([P], [Tp])
            P, AP, BP = Pn, er.block_mix([AP], [Tp]), mix_B(BP, Pn, Tp)
        S = np.hstack([X, W[:, act]] + ([P[:, act]] if useP else []))
        AS = np.hstack([AX, AW[:, act]] + ([AP[:, act]] if useP else []))
        BS = np.hstack([BX, BW[:, act]] + ([BP[:, act]] if useP else [])) if gen else S
        GS, GA = S.T @ BS, S.T @ AS
        theta, V = scipy.linalg.eigh(0.5 * (GA + GA.T), 0.5 * (GS + GS.T))
        if not theta[0] > 0.0:
            raise er.Breakdown("a Ritz value is not positive")
        na = len(act)
        CX, CW, CP = V[:K, :K], np.zeros((K, K)), np.zeros((K, K))
        CW[act] = V[K:K + na, :K]
        if useP:
            CP[act] = V[K + na:K + 2 * na, :K]
            Pn, APn = er.block_mix([W, P], [CW, CP]), er.block_mix([AW, AP], [CW, CP])
            BP = er.block_mix([BW, BP], [CW, CP]) if gen else Pn
            P, AP = Pn, APn
        else:
            P, AP = er.block_mix([W], [CW]), er.block_mix([AW], [CW])
            BP = er.block_mix([BW], [CW]) if gen else P
        Xn, AX = er.block_mix([X], [CX], add=P), er.block_mix([AX], [CX], add=AP)
        BX = er.block_mix([BX], [CX], add=BP) if gen else Xn
        X = Xn
        lam = theta[:K].copy()
        it += 1


# ---------------------------------------------------------------------------
# the driver
def start_block(n, K):
    """the generated start block of a call without start vectors: counters 0 .. K-1 -> (X, the advanced counter)"""
    return np.stack([refill(n, c) for c in range(K)], axis=1), K


def many(A, B, nev, K, sweep_nev=0, X0=None, tol=TOL, max_iter=MAX_ITER, precond=None):
    """sgpu_eigs_LOBPCG_many, step for step.  -> dict(Q (n, nlocked), lam, res, iters, sweeps, per_sweep, nlocked, converged)"""
    n = A.shape[0]
    gen = B is not None
    sweep_nev = sweep_nev or default_sweep_nev(K)
    counter = 0
    if X0 is None:
        X, counter = start_block(n, K)
    else:
        X = np.array(X0, np.float64)
    Q, BQ = np.zeros((n, 0)), np.zeros((n, 0))
    lam, res, per_sweep = [], [], []
    total, converged = 0, True
    while Q.shape[1] < nev:
        Lc = Q.shape[1]
        want = sweep_want(nev, Lc, sweep_nev)
        try:
            s = lobpcg_locked(A, B, X, want, Q if Lc else None, BQ if Lc else None, tol=tol, max_iter=max_iter - total, precond=precond)
        except er.Breakdown:
            converged = False
            break
        total += s["iters"]
        per_sweep.append(s["iters"])
        take = sweep_take(K, nev, Lc, s["leading"])
        X = s["X"].copy()
        Q = np.hstack([Q, X[:, :take]])
        if gen:
            BQ = np.hstack([BQ, s["BX"][:, :take]])
        lam += list(s["lam"][:take])
        res += list(s["res"][:take])
        if not s["converged"] or not take:
            converged = False
            break
        if Q.shape[1] < nev:
            plan, counter = refill_plan(take, counter)
            for col, c in plan:
                X[:, col] = refill(n, c)
    perm = final_order(lam)
    return dict(Q=Q[:, perm], lam=np.array(lam)[perm], res=np.array(res)[perm], iters=total, sweeps=len(per_sweep), per_sweep=per_sweep,
                nlocked=Q.shape[1], converged=converged)


# ---------------------------------------------------------------------------
# the bounds of the GPU test
def operators(shape):
    """-> (A, B or None) of a SHAPES entry"""
    (m, K, nev, sweep_nev), mass = shape
    return er.poisson(m), (gr.mass(mass, m) if mass else None)


def exact(shape):
    (m, K, nev, sweep_nev), mass = shape
    return gr.exact(mass, m, nev) if mass else er.analytic(m, nev)


def check_pairs(shape, Q, lam, nev=None, A=None, what=""):
    """both assertions of eig_ref.check_pairs / geig_ref.check_pairs on the first nev pairs (default: all of the shape's)"""
    (m, K, nev_all, sweep_nev), mass = shape
    nev = nev_all if nev is None else nev
    A0, B = operators(shape)
    A = A0 if A is None else A
    if mass:
        return gr.check_pairs(A, B, Q, lam, nev, exact(shape), gr.LAMBDA_MIN_B[mass], what=what or str(shape))
    return er.check_pairs(A, Q, lam, nev, m, what=what or str(shape))


def ortho_defect(shape, Q):
    _, B = operators(shape)
    return gr.ortho_defect(Q, B) if B is not None else er.ortho_defect(Q)
