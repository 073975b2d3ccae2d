"""The Chebyshev eigenvalue estimate (amg_hierarchy::find_eig, sgpu_op_eig_max) restated in numpy, with the two things the host loop
and the device kernels do differently left open: how a dot is summed, and where isd enters the product.

  start        find_eig's LCG sequence over the row index in (-1, 1), normalised;
  estimate     m = min(steps, n) steps of  w = isd .* (A (isd .* v)),  a = w.v,  w -= a v + b vprev,  b = ||w||,  stop at b < 1e-300,
               vprev = v, v = w / b;  1.0001 x the largest eigenvalue of the tridiagonal matrix, by numpy.linalg.eigvalsh (the library
               bisects a Sturm count to 1e-14: tests/test_lanczos_ref.py anchors this file to it);
  DOTS         the orders a dot can be summed in: one element after the other (the host loop), a binary tree, math.fsum (the exactly
               rounded sum of the rounded products), k_dot_partial + k_reduce_partials (tests/solver_ref.dot_blocked);
  APPLIES      "val*isd*x": the host's row sum of (val isd_j) x_j;  "val*(isd*x)": the device's, t = isd .* x first, then the
               operator's own product.  Rows are summed in column order in both.

Also here: the operators of tests/test_lanczos_ref.py and tests/test_gpu_lanczos.py, as (Csr, inv_diag).  No GPU import."""
import math
import os

import numpy as np
import scipy.sparse as sp

from tests import solver_ref
from tests.spgemm_ref import Csr

FACTOR = 1.0001
PLAT362 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrices", "plat362.mtx")


def start(n):
    x, out = 88172645463325252, np.empty(n)
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[i] = ((x >> 11) * (1.0 / 9007199254740992.0)) * 2.0 - 1.0
    nrm = 0.0
    for s in (out * out).tolist():             # the norm in row order, as the library sums it
        nrm += s
    return out / math.sqrt(nrm)


# ---- dots ---------------------------------------------------------------------------------------------------------------
def dot_sequential(x, y):
    return float(np.cumsum(x * y)[-1])         # cumsum adds one element after the other


def dot_pairwise(x, y):
    p = x * y
    size = 1
    while size < len(p):
        size *= 2
    p = np.concatenate([p, np.zeros(size - len(p))])
    while len(p) > 1:
        h = len(p) // 2
        p = p[:h] + p[h:]
    return float(p[0])


def dot_fsum(x, y):
    return math.fsum((x * y).tolist())


def dot_blocked(x, y):
    return solver_ref.dot_blocked(x, y)


def dot_numpy(x, y):
    return float(np.sum(x * y))                # what the GPU tests use on the large operators: fast, pairwise in blocks


DOTS = {"sequential": dot_sequential, "pairwise": dot_pairwise, "fsum": dot_fsum, "k_dot_partial": dot_blocked}
APPLIES = ("val*isd*x", "val*(isd*x)")


# ---- the recurrence -----------------------------------------------------------------------------------------------------
def tridiagonal(A, inv_diag, steps=20, dot=dot_sequential, apply="val*isd*x"):
    """-> (alpha, beta) of the recurrence"""
    n = A.nrows
    c = A.col.astype(np.int64)
    isd = np.sqrt(np.abs(np.asarray(inv_diag, np.float64)))
    assert apply in APPLIES
    # (scipy's CSR product: every row's products are added one after the other in stored order, as the library's row loops add them)
    plain = sp.csr_matrix((A.val, A.col, A.ptr), shape=(n, n))
    scaled = sp.csr_matrix((A.val * isd[c], A.col, A.ptr), shape=(n, n))

    def matvec(x):
        y = scaled @ x if apply == "val*isd*x" else plain @ (isd * x)
        return y * isd

    v, vprev, b = start(n), np.zeros(n), 0.0
    m = min(int(steps), n)
    alpha, beta = [], []
    for k in range(m):
        w = matvec(v)
        a = dot(w, v)
        alpha.append(a)
        w = w - (a * v + b * vprev)
        b = math.sqrt(dot(w, w))
        if k + 1 < m:
            beta.append(b)
        if b < 1e-300:
            break
        vprev, v = v, w / b
    return alpha, beta


def ritz_max(alpha, beta):
    kd = len(alpha)
    T = np.diag(alpha) + np.diag(beta[:kd - 1], 1) + np.diag(beta[:kd - 1], -1)
    return float(np.linalg.eigvalsh(T)[-1])


def estimate(A, inv_diag, steps=20, dot=dot_sequential, apply="val*isd*x"):
    return FACTOR * ritz_max(*tridiagonal(A, inv_diag, steps, dot, apply))


# ---- operators ----------------------------------------------------------------------------------------------------------
def from_coo(n, rows, cols, vals):
    order = np.lexsort((cols, rows))
    rows, cols, vals = np.asarray(rows)[order], np.asarray(cols)[order], np.asarray(vals, np.float64)[order]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return Csr(ptr, cols.astype(np.int32), vals, int(n), int(n))


def diagonal(A):
    r = np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(A.ptr))
    d = np.full(A.nrows, np.nan)
    on = r == A.col
    d[r[on]] = A.val[on]
    return d


def poisson(m):
    """the 7-point Laplacian on an m^3 grid, every grid point a row (6 on the diagonal, -1 to each neighbour inside the grid)"""
    n = m ** 3
    idx = np.arange(n, dtype=np.int64)
    x, y, z = idx % m, (idx // m) % m, idx // (m * m)
    rows, cols, vals = [idx], [idx], [np.full(n, 6.0)]
    for coord, step in ((x, 1), (y, m), (z, m * m)):
        for sign in (-1, 1):
            ok = (coord + sign >= 0) & (coord + sign < m)
            rows.append(idx[ok]); cols.append(idx[ok] + sign * step); vals.append(np.full(int(ok.sum()), -1.0))
    return from_coo(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def scaled(A, log_range=3.0):
    """D A D with d_i = exp(log_range sin(0.37 i)): symmetric, the same spectrum of D^-1 A up to the scaling, entries over e^(+-2 log_range)"""
    d = np.exp(log_range * np.sin(0.37 * np.arange(A.nrows)))
    r = np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(A.ptr))
    return Csr(A.ptr.copy(), A.col.copy(), d[r] * A.val * d[A.col.astype(np.int64)], A.nrows, A.ncols)


def diagonal_operator(n=9):
    """diag(3, 4, ...): D^-1/2 A D^-1/2 is the identity, w - a v is rounding noise after the first step"""
    return from_coo(n, np.arange(n), np.arange(n), 3.0 + np.arange(n))


def plat362():
    """tests/golden/matrices/plat362.mtx as the host library assembles it -> (Csr, inv_diag)"""
    from saena_amd import host
    from tests import setup_ref
    A = host.Matrix(host.Comm("host", "self")).read_file(PLAT362).assemble()
    d = A.layout()
    return setup_ref.from_layout(d), d["inv_diag"].copy()


def operator(name):
    """-> (Csr, inv_diag)"""
    if name == "plat362":
        return plat362()
    if name.startswith("poisson"):
        A = poisson(int(name[len("poisson"):]))
    elif name.startswith("scaled"):
        A = scaled(poisson(int(name[len("scaled"):])))
    elif name == "diagonal9":
        A = diagonal_operator(9)
    elif name == "one_row":
        A = from_coo(1, [0], [0], [4.0])
    else:
        raise ValueError(name)
    return A, 1.0 / diagonal(A)


def descriptor(A, inv_diag):
    """capi.Operator's keywords for a one-rank operator"""
    return dict(M=A.nrows, N_local=A.ncols, col_offset=0, nnzPerRow_local=np.diff(A.ptr).astype(np.int32), col_local=A.col, val_local=A.val,
                inv_diag=inv_diag)
