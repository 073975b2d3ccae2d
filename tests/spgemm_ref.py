"""Two references for the sparse product C = A B of the AMG setup that share no code with the host kernel
(saena_amd/csrc/host/amg_setup.cpp, spgemm_host) or with the device kernels (saena_amd/csrc/sgpu_spgemm.hip).

The contract of both kernels, for A (m x k), B (k x n) in CSR and `row_offset` (the global id of row 0 of A):
  * every entry c_ij starts at 0.0 and adds the products a_il * b_lj -- each rounded once, no FMA -- in the order of the
    entries of row i of A (a row of A may name a row of B twice: two products, in sequence);
  * the entry is kept iff |c_ij| > 1e-14 or i + row_offset == j (a NaN off the diagonal is dropped: the test is
    "not (|c| > t)");
  * the rows of C ascend by column.

`sequential` computes exactly that, vectorised; `sequential_loop` is the same contract as a plain double loop and pins the
vectorised form (tests/test_spgemm_conformance.py::test_the_vectorised_reference_is_the_plain_loop).  `exact` sums the same
rounded-once products without rounding (math.fsum) and gives S_ij = sum |a_il b_lj|: whatever order a correct kernel adds n
products in, its sum differs from the exact one by at most gamma_(n) S <= n eps S / (1 - n eps) (Higham, Accuracy and
Stability of Numerical Algorithms, 4.2, with the first addition to 0.0 exact); `bound` is that figure.  It catches a
sequential reference that is wrong the same way the kernels are.
"""
import math
from collections import namedtuple

import numpy as np

DROP = 1e-14                     # SAENA_ALMOST_ZERO
EPS = 2.0 ** -53                 # unit roundoff of binary64

Csr = namedtuple("Csr", "ptr col val nrows ncols")
Expanded = namedtuple("Expanded", "row col prod start length n_products")


def csr(rows, ncols):
    """rows: one (columns, values) pair per row, as given (no sorting, no merging) -> Csr"""
    ptr = np.zeros(len(rows) + 1, np.int64)
    for i, (c, _) in enumerate(rows):
        ptr[i + 1] = ptr[i] + len(c)
    col = np.concatenate([np.asarray(c, np.int32) for c, _ in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    val = np.concatenate([np.asarray(v, np.float64) for _, v in rows] + [np.zeros(0, np.float64)]).astype(np.float64)
    return Csr(ptr, col, val, len(rows), int(ncols))


def from_scipy(M):
    M = M.tocsr().copy()
    M.sum_duplicates()
    M.sort_indices()
    return Csr(M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.astype(np.float64), M.shape[0], M.shape[1])


def check_operands(A, B):
    """the kernels' preconditions: ids in range, the columns of every row of B distinct and ascending"""
    assert A.ncols == B.nrows and len(A.col) == A.ptr[-1] and len(B.col) == B.ptr[-1]
    assert len(A.col) == 0 or (A.col.min() >= 0 and A.col.max() < B.nrows)
    assert len(B.col) == 0 or (B.col.min() >= 0 and B.col.max() < B.ncols)
    inner = np.ones(len(B.col), bool)
    inner[B.ptr[:-1][B.ptr[:-1] < len(B.col)]] = False          # first entry of every non-empty row
    assert np.all(np.diff(B.col.astype(np.int64))[inner[1:]] > 0), "a row of B is not ascending and distinct"


def expand(A, B):
    """every product a_il * b_lj in generation order (row of A, then entry of that row, then entry of B's row), grouped by
    output entry with a STABLE sort: inside a group the products keep the order in which a kernel has to add them"""
    a_row = np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(A.ptr))
    b_len = (B.ptr[1:] - B.ptr[:-1])[A.col]
    n_products = np.zeros(A.nrows, np.int64)
    np.add.at(n_products, a_row, b_len)
    total = int(b_len.sum())
    src_a = np.repeat(np.arange(len(A.col), dtype=np.int64), b_len)
    first = np.cumsum(b_len) - b_len
    src_b = B.ptr[:-1][A.col][src_a] + (np.arange(total, dtype=np.int64) - first[src_a])
    row, colj = a_row[src_a], B.col[src_b].astype(np.int64)
    with np.errstate(all="ignore"):
        prod = A.val[src_a] * B.val[src_b]                                   # one rounding per product
    order = np.argsort(row * max(B.ncols, 1) + colj, kind="stable")
    row, colj, prod = row[order], colj[order], prod[order]
    new = np.ones(total, bool)
    new[1:] = (row[1:] != row[:-1]) | (colj[1:] != colj[:-1])
    start = np.flatnonzero(new)
    length = np.diff(np.append(start, total))
    return Expanded(row[start], colj[start], prod, start, length, n_products)


def _assemble(E, value, row_offset, nrows):
    with np.errstate(invalid="ignore"):
        keep = (np.abs(value) > DROP) | (E.row + row_offset == E.col)
    ptr = np.zeros(nrows + 1, np.int64)
    np.add.at(ptr, E.row[keep] + 1, 1)
    return np.cumsum(ptr), E.col[keep].astype(np.int32), value[keep], keep


def sequential(A, B, row_offset=0, expanded=None):
    """-> (c_ptr, c_col, c_val, info): the contract, entry by entry; info has the expansion, every entry's value before
    the drop rule and the kept mask (for the bound and for the expected path of every row)"""
    E = expanded or expand(A, B)
    by_len = np.argsort(-E.length, kind="stable")
    acc = np.zeros(len(E.start))
    with np.errstate(all="ignore"):
        for t in range(int(E.length.max()) if len(E.length) else 0):
            live = by_len[:np.searchsorted(-E.length[by_len], -t, side="left")]      # the entries with more than t products
            acc[live] = acc[live] + E.prod[E.start[live] + t]
    ptr, col, val, keep = _assemble(E, acc, row_offset, A.nrows)
    return ptr, col, val, dict(E=E, value=acc, keep=keep)


def sequential_loop(A, B, row_offset=0):
    """the same contract as the plain double loop it is stated as (small operands only)"""
    ptr, col, val = [0], [], []
    for i in range(A.nrows):
        acc = {}
        for ka in range(A.ptr[i], A.ptr[i + 1]):
            l, a = int(A.col[ka]), A.val[ka]
            for kb in range(B.ptr[l], B.ptr[l + 1]):
                j = int(B.col[kb])
                with np.errstate(all="ignore"):
                    acc[j] = acc.get(j, np.float64(0.0)) + a * B.val[kb]
        for j in sorted(acc):
            if abs(acc[j]) > DROP or i + row_offset == j:
                col.append(j); val.append(acc[j])
        ptr.append(len(col))
    return np.array(ptr, np.int64), np.array(col, np.int32), np.array(val, np.float64)


def exact(E):
    """per output entry: the correctly rounded sum of its (rounded-once) products, and S = sum of their magnitudes.
    Entries with a non-finite product get NaN / Inf: no bound applies to them."""
    p = E.prod.tolist()
    finite = np.isfinite(np.add.reduceat(np.abs(E.prod), E.start)) if len(E.start) else np.zeros(0, bool)
    ex = np.full(len(E.start), np.nan)
    for g in np.flatnonzero(finite):
        s = E.start[g]
        ex[g] = math.fsum(p[s:s + E.length[g]])
    S = np.full(len(E.start), np.inf)
    for g in np.flatnonzero(finite):
        s = E.start[g]
        S[g] = math.fsum(abs(x) for x in p[s:s + E.length[g]])
    return ex, S


def bound(E, S):
    """gamma_n S with n the number of products of the entry; plus half an ulp of S for the rounding of `exact` itself"""
    n = E.length.astype(np.float64)
    return n * EPS / (1.0 - n * EPS) * S + EPS * S


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same_values(got, want, what):
    """bit for bit; a NaN only has to be a NaN where the reference has one (its payload and sign are not part of the contract)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN entries")
    bad = np.flatnonzero(bits(got)[~nan] != bits(want)[~nan])
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} values differ in their bits, first at kept entry {np.flatnonzero(~nan)[bad[0]]}: " \
                          f"{got[~nan][bad[0]]!r} != {want[~nan][bad[0]]!r}"
