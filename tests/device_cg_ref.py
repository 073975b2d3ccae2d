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
