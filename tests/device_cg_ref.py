"""The device-resident coarsest CG (coarse_solver = 2, saena_amd/csrc/kernels_coarse_cg.hip.h) restated in float64 numpy, and the
cases tests/test_gpu_device_cg.py runs (test infrastructure: numpy/scipy only, no GPU, no oracle).

The restatement follows the kernels launch by launch -- the two scalar slots of `dot` by iteration parity, the two stop words, the
iteration count written by the direction kernel -- with every dot in solver_ref.dot_blocked's order (k_dot_partial's element-to-thread
assignment, k_reduce_partials' order over the partial sums).  The product is scipy's: a row's entries in stored order, where the kernel
gives a row 1, 4, 16 or 64 lanes; tests/test_device_cg_ref.py holds the restatement to the four bounds the GPU test asserts, which is
the evidence that those bounds leave room for a summation order.
"""
import numpy as np

from tests import solver_ref as sr

# the four bounds of the coarsest-CG contract (tests/test_gpu_solver_layer.py, check_cg_contracts), restated
IT_SLACK = 1                 # |it - it_oracle| <= 1
REL_ORACLE = 1e-11           # rel(u, u_oracle)
REL_HP_FACTOR = 2.0          # rel(u, x_hp) <= 2 cond tol
RESID_FACTOR = 2.0           # residual_hp <= 2 tol ||rhs||

# one-level hierarchies: the first size on the new path (3, 17 and 1 025 entries in a row; a last workgroup that is not full), a wave per row
CONTRACT_CASES = (("tri", 1025), ("band17", 1025), ("arrow", 1025), ("dense_spd", 1100))
BIG_TRI = 262401             # the partial sums take a second grid-stride trip (256 * 1024 < n); too large for solver_ref.case
EARLY_OUT_CASES = (("tri", 1025),)
CAPPED_CASES = (("tri", 1300), ("band17", 1300))         # CG_coarsest_max_iter = 6
CAP = 6
# the smallest caps: 1 is k_dcg_setup's own branch (count 0, 2 launches, no iteration), 2 is k_dcg_dir's `it + 1 == max_iter` rule at its
# first iteration, 3 and 7 are odd (the last iteration reads the dot's slot 0 / writes slot 1, the reverse of cap 6)
CAPS = (1, 2, 3, 7)
CAPS_CASES = (("tri", 1300), ("band17", 1300))
CAPS_COUNT = {1: 0, 2: 1, 3: 2, 7: 6}                    # solve_coarsest_CG's `i--`: cap - 1 updates, reported as cap - 1
SMALL_SIZES = (257, 1024)    # at most CG_MAXN rows: value 2 runs k_coarse_cg, value 0's bits
SET_OPERATOR = (("tri", 1300), ("band17", 1300))
TWO_LEVEL = (2600, 2)        # solver_ref.tri_two_level: 1 300 coarse rows


def band49(n, seed):
    """solver_ref.band17 with offsets 1..24: up to 49 entries per row, which is what gives a row 16 lanes (no case of solver_ref does)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    Up = sp.csr_matrix((n, n))
    for d in range(1, 25):
        Up = Up + sp.diags([-(0.5 + rng.random(n - d)) / (1 + d)], [d], shape=(n, n))
    off = (Up + Up.T).tocsr()
    diag = np.asarray(abs(off).sum(axis=1)).ravel() + 1.0
    A = (off + sp.diags([diag], [0], shape=(n, n))).tocsr()
    A.sort_indices()
    return A


EXTRA_CASES = (("band49", 1025),)
_cache = {}


def case(family, n):
    """solver_ref.case, plus the families of this module; computed once and shared: treat as read-only"""
    if family != "band49":
        return sr.case(family, n)
    if (family, n) not in _cache:
        A = band49(n, 49 + n)
        D, b = A.toarray(), sr.rhs_for(n)
        x, resid = sr.solve_hp(D, b)
        for a in (D, b, x):
            a.setflags(write=False)
        _cache[(family, n)] = dict(A=A, dense=D, rhs=b, x=x, resid=resid, cond=float(np.linalg.cond(D)))
    return _cache[(family, n)]


def sparse_case(A, rhs):
    """a case dict for check_contracts of a symmetric scipy matrix too large for solver_ref.case's dense algebra (a coarsest level
    of thousands of rows): x by a sparse LU and three rounds of refinement on a longdouble residual -- solve_hp's scheme --, cond as
    max |lambda| / min |lambda|, which is the 2-norm condition number np.linalg.cond gives for a symmetric matrix, definite or not.
    The asymmetry rounding leaves in a Galerkin product is checked to be far below min |lambda|.  eig_ends: the smallest
    eigenvalue, the one nearest zero, the largest."""
    import scipy.sparse.linalg as sla
    A = A.tocsr()
    rhs = np.asarray(rhs, np.float64)
    lu = sla.splu(A.tocsc())
    x = lu.solve(rhs).astype(np.longdouble)
    Al, idx, bl = A.data.astype(np.longdouble), A.indices, rhs.astype(np.longdouble)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))

    def resid(x):
        Ax = np.zeros(A.shape[0], np.longdouble)
        np.add.at(Ax, rows, Al * x[idx])
        return bl - Ax
    for _ in range(3):
        x = x + lu.solve(resid(x).astype(np.float64)).astype(np.longdouble)
    r = resid(x)
    Asym = ((A + A.T) * 0.5).tocsc()
    asym = float(abs(A - A.T).sum(axis=1).max())                                  # the infinity norm bounds the 2-norm
    ends = [float(sla.eigsh(Asym, k=1, which=w, return_eigenvectors=False, tol=1e-10)[0]) for w in ("LA", "SA")]
    near0 = float(sla.eigsh(Asym, k=1, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-10)[0])
    lmax, lmin = max(abs(e) for e in ends), abs(near0)
    assert lmin > 0.0 and asym <= 1e-10 * lmin, (lmin, asym)
    return dict(A=A, rhs=rhs, x=x.astype(np.float64), resid=float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(bl * bl))), cond=lmax / lmin,
                eig_ends=(ends[1], near0, ends[0]))


def check_contracts(c, u, it, u_o, it_o):
    """the four bounds, each figure printed before it is asserted; c: a case dict"""
    nrm = np.linalg.norm(c["rhs"])
    print(f"it {it} (oracle {it_o}), rel oracle {sr.rel(u, u_o):.2e}, rel hp {sr.rel(u, c['x']):.2e} of {REL_HP_FACTOR * c['cond'] * sr.CG_TOL:.2e}, "
          f"residual {sr.residual_hp(c['A'], u, c['rhs']) / nrm:.2e}")
    assert abs(it - it_o) <= IT_SLACK, (it, it_o)
    assert sr.rel(u, u_o) <= REL_ORACLE
    assert sr.rel(u, c["x"]) <= REL_HP_FACTOR * c["cond"] * sr.CG_TOL
    assert sr.residual_hp(c["A"], u, c["rhs"]) <= RESID_FACTOR * sr.CG_TOL * nrm


def lanes_per_row(A):
    """block_auto_lanes: 1, 4, 16 or 64 lanes from the mean row length (8 entries per lane)"""
    mean = A.nnz / A.shape[0] if A.shape[0] else 0.0
    for G in (1, 4, 16):
        if G * 8.0 >= mean:
            return G
    return 64


def launches(max_iter):
    """the fixed length of the sequence"""
    return 2 + 3 * (max(max_iter, 1) - 1)


def device_cg(A, rhs, u0=None, tol=sr.CG_TOL, max_iter=sr.CG_MAX_ITER):
    """-> (u, reported iterations, launches that did work).  Every launch of the fixed sequence is walked; one that finds its stop
    word set does nothing."""
    rhs = np.asarray(rhs, np.float64)
    u = np.zeros(len(rhs)) if u0 is None else np.array(u0, np.float64)
    # k_dcg_start, k_dcg_setup
    res, dirv = rhs.copy(), rhs.copy()
    dot0 = sr.dot_blocked(res, res)
    thres = dot0 * tol * tol
    slot = [0.0, dot0]                                   # iteration `it` reads slot[it & 1]
    stop = stop_dir = dot0 < tol * tol
    iters = 0 if (not stop and max_iter == 1) else 1
    worked = 2
    for it in range(1, max_iter):
        # k_dcg_matvec
        if stop:
            stop_dir = True
        else:
            mt = A @ dirv
            worked += 1
        # k_dcg_update
        if not stop:
            factor = slot[it & 1] / sr.dot_blocked(dirv, mt)
            u += factor * dirv
            res -= factor * mt
            worked += 1
        # k_dcg_dir
        if not stop_dir:
            dot = sr.dot_blocked(res, res)
            worked += 1
            if dot < thres:
                stop = True
                continue
            factor = dot / slot[it & 1]
            slot[(it + 1) & 1] = dot
            iters = it if it + 1 == max_iter else it + 1
            dirv = res + factor * dirv
    return u, iters, worked
