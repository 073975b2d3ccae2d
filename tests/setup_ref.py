"""The smoothed-aggregation setup restated the plain way (numpy only).  It shares no code with
saena_amd/csrc/host/amg_setup.cpp; every function is the rule itself, vectorised only where that leaves the order of
the additions alone.  tests/test_setup_ref.py anchors it -- aggregates and P against the compiled reference's fixtures,
the Galerkin product and the filter against plain double loops -- before tests/test_setup_contract.py holds the
product to it.

  strength      mx_i = max over the off-diagonal k of -a_ik, started at -DBL_MAX (a row without off-diagonals keeps it; a row
                of positive off-diagonals has a negative mx_i).  An entry is strong iff it is the diagonal, or
                -a_ij / mx_i > conn, or -a_ij / mx_j > conn; conn is the float32 option promoted to double.
  plain_rounds  synchronous rounds; every undecided row scans ALL its strong neighbours in EVERY round for the smallest id
                among those that are undecided or roots; itself -> a root, a root -> it joins.  Roots are numbered in
                ascending order of their fine index.
  smoothed_P    row i, in the order of its stored columns: the term ((-w inv_diag_i) a_ik), the diagonal's + 1 after the
                product; w = float32(2/3) as a double, inv_diag_i = 1 / a_ii.  Terms of equal coarse id are added one after
                the other in that stored order; a sum stays iff |v| > 1e-14; columns ascend.
  transpose     rows ascend by fine row id.
  galerkin      (R A) P, each product by the contract of tests/spgemm_ref.py (drop rule included).
  filter        off-diagonal entries with |v| <= thre leave; their values are added to one another in row order and the sum
                is added to the diagonal once; a diagonal that ends with |d| < 1e-14 becomes 1.0; a row without a
                diagonal gets one of value 1.0 at its place in column order.
  hierarchy     the level loop: the filter from the filter_start-th coarsening step on, its threshold capped at filter_max
                before use and multiplied by 10^filter_rate after; with dynamic_levels a step whose aggregates number
                <= 100 or > 0.90 of the rows is the last; max_level caps the steps.
  lanczos_eig   at most 20 Lanczos steps on D^-1/2 A D^-1/2 from an LCG start vector, largest eigenvalue of the
                tridiagonal matrix (np.linalg.eigvalsh) times 1.0001; in float64, or with the dots and updates in
                np.longdouble.
"""
from collections import namedtuple

import numpy as np

from tests import spgemm_ref
from tests.spgemm_ref import Csr

DROP = 1e-14
DBL_MAX = np.finfo(np.float64).max
OMEGA = float(np.float32(2.0 / 3.0))

# agg, nagg, P, R are None on the coarsest level; dropped: the entries the filter took out of the Galerkin product that became A
Level = namedtuple("Level", "A agg nagg P R dropped")


def from_layout(d, ncols=None):
    """a one-rank layout of host.AmgSolver.level_layout / host.Matrix.layout -> Csr"""
    ptr = np.concatenate([[0], np.cumsum(d["nnzPerRow_local"], dtype=np.int64)]).astype(np.int64)
    return Csr(ptr, d["col_local"].astype(np.int32), d["val_local"].astype(np.float64), int(d["M"]), int(ncols if ncols is not None else d["N_local"]))


def from_coo(n, rows, cols, vals):
    """distinct entries in any order -> Csr, columns ascending"""
    order = np.lexsort((cols, rows))
    rows, cols, vals = np.asarray(rows)[order], np.asarray(cols)[order], np.asarray(vals, np.float64)[order]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return Csr(ptr, cols.astype(np.int32), vals, int(n), int(n))


def rows_of(A):
    return np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(A.ptr))


def diagonal(A):
    r = rows_of(A)
    d = np.full(A.nrows, np.nan)
    on = r == A.col
    d[r[on]] = A.val[on]
    return d


# ---------------------------------------------------------------------------------------------------------------------
def strength(A, conn):
    """-> one bool per stored entry of A: the entry is a strong connection"""
    conn = float(np.float32(conn))
    r, c = rows_of(A), A.col.astype(np.int64)
    off = r != c
    mx = np.full(A.nrows, -DBL_MAX)
    np.maximum.at(mx, r[off], -A.val[off])
    with np.errstate(all="ignore"):
        return ~off | (-A.val / mx[r] > conn) | (-A.val / mx[c] > conn)


def plain_rounds(A, strong):
    """-> (coarse id of every row, number of aggregates)"""
    n = A.nrows
    ptr, col = A.ptr.tolist(), A.col.tolist()
    keep = strong.tolist()
    nei = [[col[k] for k in range(ptr[i], ptr[i + 1]) if keep[k]] for i in range(n)]
    agg, decided, root = list(range(n)), [False] * n, [False] * n
    undecided = list(range(n))
    while undecided:
        verdict = []
        for i in undecided:
            best, dec, rn = agg[i], True, False
            for c in nei[i]:
                if agg[c] < best and (not decided[c] or root[c]):
                    best, dec, rn = agg[c], decided[c], root[c]
            verdict.append((best, dec, rn))
        still = []
        for i, (best, dec, rn) in zip(undecided, verdict):
            if not dec:
                still.append(i)
                continue
            decided[i] = True
            if agg[i] == best:
                root[i] = True
            elif rn:
                agg[i] = best
        undecided = still
    ids = np.flatnonzero(np.array(root, bool))
    return np.searchsorted(ids, np.array(agg, np.int64)).astype(np.int32), len(ids)


def smoothed_P(A, agg, nagg):
    r, c = rows_of(A), A.col.astype(np.int64)
    inv_diag = 1.0 / diagonal(A)
    term = (-OMEGA * inv_diag[r]) * A.val
    on = r == c
    term[on] = term[on] + 1.0
    key = r * nagg + agg[c]
    uk, group = np.unique(key, return_inverse=True)
    value = np.zeros(len(uk))
    np.add.at(value, group, term)                   # unbuffered: one addition per term, in the order of the stored entries
    keep = np.abs(value) > DROP
    uk, value = uk[keep], value[keep]
    ptr = np.zeros(A.nrows + 1, np.int64)
    np.add.at(ptr, uk // nagg + 1, 1)
    return Csr(np.cumsum(ptr), (uk % nagg).astype(np.int32), value, A.nrows, int(nagg))


def smoothed_P_loop(A, agg, nagg):
    """smoothed_P as the loop it is stated as (small operands: pins the vectorised form)"""
    ptr, col, val = [0], [], []
    d = diagonal(A)
    for i in range(A.nrows):
        acc, scale = {}, -OMEGA * (1.0 / d[i])
        for k in range(A.ptr[i], A.ptr[i + 1]):
            t = scale * A.val[k]
            if A.col[k] == i:
                t = t + 1.0
            j = int(agg[A.col[k]])
            acc[j] = acc[j] + t if j in acc else t
        for j in sorted(acc):
            if abs(acc[j]) > DROP:
                col.append(j); val.append(acc[j])
        ptr.append(len(col))
    return Csr(np.array(ptr, np.int64), np.array(col, np.int32), np.array(val, np.float64), A.nrows, int(nagg))


def transpose(P):
    r = rows_of(P)
    order = np.argsort(P.col, kind="stable")        # equal coarse ids keep the order of their fine rows: ascending
    ptr = np.zeros(P.ncols + 1, np.int64)
    np.add.at(ptr, P.col.astype(np.int64) + 1, 1)
    return Csr(np.cumsum(ptr), r[order].astype(np.int32), P.val[order], P.ncols, P.nrows)


def n_products(A, B):
    """how many products spgemm_ref.expand materialises for A B"""
    return int((B.ptr[1:] - B.ptr[:-1])[A.col].sum())


CHUNK = 10 ** 6                 # products spgemm_ref.expand materialises at a time (rows of C are independent of one another)


def product(A, B, chunk=CHUNK, row_offset=0):
    """C = A B by spgemm_ref.sequential, a block of A's rows at a time: no expansion holds more than `chunk` products
    (a single row that has more is refused).  row_offset: the id of A's row 0 in the level (the drop rule's diagonal)"""
    per_row = np.zeros(A.nrows + 1, np.int64)
    np.add.at(per_row, rows_of(A) + 1, (B.ptr[1:] - B.ptr[:-1])[A.col])
    cum = np.cumsum(per_row)
    assert A.nrows == 0 or np.diff(cum).max() <= chunk, "one row of the product exceeds the chunk"
    ptrs, cols, vals, lo = [np.zeros(1, np.int64)], [], [], 0
    while lo < A.nrows:
        hi = max(lo + 1, int(np.searchsorted(cum, cum[lo] + chunk, side="right")) - 1)
        blk = Csr(A.ptr[lo:hi + 1] - A.ptr[lo], A.col[A.ptr[lo]:A.ptr[hi]], A.val[A.ptr[lo]:A.ptr[hi]], hi - lo, A.ncols)
        p, c, v, _ = spgemm_ref.sequential(blk, B, row_offset=row_offset + lo)
        ptrs.append(p[1:] + ptrs[-1][-1]); cols.append(c); vals.append(v)
        lo = hi
    return Csr(np.concatenate(ptrs), np.concatenate(cols + [np.zeros(0, np.int32)]).astype(np.int32),
               np.concatenate(vals + [np.zeros(0)]), A.nrows, B.ncols)


def galerkin(R, A, P, chunk=CHUNK):
    return product(product(R, A, chunk), P, chunk)


def galerkin_loop(R, A, P):
    p, c, v = spgemm_ref.sequential_loop(R, A)
    p, c, v = spgemm_ref.sequential_loop(Csr(p, c, v, R.nrows, A.ncols), P)
    return Csr(p, c, v, R.nrows, P.ncols)


def filter(C, thre, row_offset=0):      # noqa: A001 -- the setup's name for it
    """C holds rows [row_offset, row_offset + C.nrows) of a level, its columns are global ids"""
    r, c = rows_of(C), C.col.astype(np.int64)
    on = c == r + row_offset
    with np.errstate(invalid="ignore"):
        stay = on | (np.abs(C.val) > thre)
    lump = np.zeros(C.nrows)
    np.add.at(lump, r[~stay], C.val[~stay])         # in row order, from 0.0
    val = C.val.copy()
    val[on] = val[on] + lump[r[on]]                 # once
    tiny = on & (np.abs(val) < DROP)
    val[tiny] = 1.0
    has = np.zeros(C.nrows, bool)
    has[r[on]] = True
    new = np.flatnonzero(~has)
    rr = np.concatenate([r[stay], new])
    cc = np.concatenate([c[stay], new + row_offset])
    vv = np.concatenate([val[stay], np.ones(len(new))])
    order = np.lexsort((cc, rr))
    ptr = np.zeros(C.nrows + 1, np.int64)
    np.add.at(ptr, rr + 1, 1)
    return Csr(np.cumsum(ptr), cc[order].astype(np.int32), vv[order], C.nrows, C.ncols)


def filter_loop(C, thre, row_offset=0):
    """filter as the loop it is stated as (small operands: pins the vectorised form)"""
    ptr, col, val = [0], [], []
    for i in range(C.nrows):
        g, row, lump, at = i + row_offset, [], np.float64(0.0), None
        for k in range(C.ptr[i], C.ptr[i + 1]):
            j, v = int(C.col[k]), C.val[k]
            if j == g:
                at = len(row)
                row.append([j, v])
            elif abs(v) > thre:
                row.append([j, v])
            else:
                lump = lump + v
        if at is None:
            row.append([g, np.float64(1.0)])
            row.sort(key=lambda e: e[0])
        else:
            row[at][1] = row[at][1] + lump
            if abs(row[at][1]) < DROP:
                row[at][1] = np.float64(1.0)
        col += [e[0] for e in row]; val += [e[1] for e in row]
        ptr.append(len(col))
    return Csr(np.array(ptr, np.int64), np.array(col, np.int32), np.array(val, np.float64), C.nrows, C.ncols)


# ---------------------------------------------------------------------------------------------------------------------
def filter_thresholds(options, steps):
    """the filter's threshold at every coarsening step (None: the step is not filtered)"""
    thre, out = float(options["filter_thre"]), []
    for step in range(1, steps + 1):
        out.append(None)
        if step >= int(options["filter_start"]):
            thre = min(thre, float(options["filter_max"]))
            out[-1] = thre
            thre *= 10.0 ** int(options["filter_rate"])
    return out


def hierarchy(A, options, max_products=None, chunk=CHUNK):
    """-> [Level]; options: the dict host.options takes (connStrength, dynamic_levels, max_level, filter_*).
    max_products: refuse (AssertionError) a product of more products than that, before anything of it is expanded"""
    thre = filter_thresholds(options, int(options["max_level"]))
    levels, dropped = [], 0
    for step in range(int(options["max_level"])):
        agg, nagg = plain_rounds(A, strength(A, options["connStrength"]))
        last = bool(options["dynamic_levels"]) and (nagg <= 100 or float(np.float32(nagg) / np.float32(A.nrows)) > 0.90)
        P = smoothed_P(A, agg, nagg)
        R = transpose(P)
        if max_products is not None:
            assert n_products(R, A) <= max_products, f"R A of {A.nrows} rows: {n_products(R, A)} products"
        RA = product(R, A, chunk)
        if max_products is not None:
            assert n_products(RA, P) <= max_products, f"(R A) P of {A.nrows} rows: {n_products(RA, P)} products"
        Ac = product(RA, P, chunk)
        before = len(Ac.col)
        if thre[step] is not None:
            Ac = filter(Ac, thre[step])
        levels.append(Level(A, agg, nagg, P, R, dropped))
        A, dropped = Ac, before - len(Ac.col)
        if last:
            break
    levels.append(Level(A, None, None, None, None, dropped))
    return levels


# ---------------------------------------------------------------------------------------------------------------------
def lcg_start(n):
    x, out = 88172645463325252, np.empty(n)
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[i] = ((x >> 11) * (1.0 / 9007199254740992.0)) * 2.0 - 1.0
    return out


def lanczos_eig(A, dtype=np.float64, factor=1.0001):
    """the estimate of lambda_max(D^-1 A); dtype: the format of the vectors, the matvec's sums, the dots and the updates"""
    n = A.nrows
    r, c = rows_of(A), A.col.astype(np.int64)
    isd = np.sqrt(np.abs(1.0 / diagonal(A))).astype(dtype)
    scaled = A.val.astype(dtype) * isd[c]

    def matvec(x):
        y = np.zeros(n, dtype)
        np.add.at(y, r, scaled * x[c])
        return y * isd

    v = lcg_start(n).astype(dtype)
    v = v / np.sqrt(np.sum(v * v))
    vprev, b = np.zeros(n, dtype), dtype(0)
    m = min(20, n)
    alpha, beta = [], []
    for k in range(m):
        w = matvec(v)
        a = np.sum(w * v)
        alpha.append(float(a))
        w = w - (a * v + b * vprev)
        b = np.sqrt(np.sum(w * w))
        if k + 1 < m:
            beta.append(float(b))
        if b < 1e-300:
            break
        vprev, v = v, w / b
    kd = len(alpha)
    T = np.diag(alpha) + np.diag(beta[:kd - 1], 1) + np.diag(beta[:kd - 1], -1)
    return factor * float(np.linalg.eigvalsh(T)[-1])
