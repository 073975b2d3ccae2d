"""References and inputs for the solver-layer tests (test infrastructure: numpy/scipy only, no GPU, no oracle).

Coarsest-level systems (scipy CSR, float64, seeded), a high-precision reference solution, a high-precision dot and
the dot's error bound, plus float64 numpy restatements of the three algorithms the GPU kernels implement -- the
coarsest CG, the Gauss-Jordan inverse, the dot's blocked summation order -- so that tests/test_solver_ref.py can show
on the CPU that a correct implementation stays inside every bound tests/test_gpu_solver_layer.py asserts.
"""
import numpy as np
import scipy.sparse as sp

# the residuals of solve_hp and the products of dot_hp need more than float64: x87 extended (64-bit significand) or better
assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 on this platform"

U = 2.0 ** -53                       # unit roundoff of float64

# the library's constants (saena_amd/csrc/kernels.hip.h, sgpu_runtime.hip)
BLOCK = 256                          # threads of a streaming / dot block, and of the coarsest solvers' one workgroup
N_PARTIALS = 1024                    # most blocks a dot launches
CG_MAXN = 1024                       # most rows the LDS-resident coarsest solvers hold


# ---------------------------------------------------------------------------
# matrices
def tri(n):
    """diagonal 2.5, off-diagonals -1 (eigenvalues in (0.5, 4.5))"""
    return sp.diags([np.full(max(n - 1, 0), -1.0), np.full(n, 2.5), np.full(max(n - 1, 0), -1.0)], [-1, 0, 1], shape=(n, n), format="csr")


def band17(n, seed):
    """symmetric, offsets 1..8 (up to 17 entries per row: more than the 8 lanes the LDS matvec gives a row), off-diagonal
    -(0.5 + U[0,1)) / (1 + d) at offset d, diagonal = row sum of |off-diagonals| + 1"""
    rng = np.random.default_rng(seed)
    Up = sp.csr_matrix((n, n))
    for d in range(1, min(8, n - 1) + 1):
        Up = Up + sp.diags([-(0.5 + rng.random(n - d)) / (1 + d)], [d], shape=(n, n))
    off = (Up + Up.T).tocsr()
    diag = np.asarray(abs(off).sum(axis=1)).ravel() + 1.0
    A = (off + sp.diags([diag], [0], shape=(n, n))).tocsr()
    A.sort_indices()
    return A


def arrow(n):
    """diagonal 3 + (i mod 5); first row and first column -1/n: one row of n entries, the others 2"""
    A = sp.lil_matrix((n, n))
    A[0, :] = -1.0 / n
    A[:, 0] = -1.0 / n
    A.setdiag(3.0 + (np.arange(n) % 5))
    A = A.tocsr()
    A.sort_indices()
    return A


def dense_spd(n, seed):
    """B B^T / n + I, B standard normal: every row has n entries"""
    B = np.random.default_rng(seed).standard_normal((n, n))
    S = B @ B.T / n
    return sp.csr_matrix((S + S.T) / 2 + np.eye(n))


def shifted(n, seed):
    """For the direct solver only: tri(n) plus a seeded strictly-upper band (offsets 1..2, values 0.3 U[0,1)), then the
    rows rolled down by one.  The 2.5 of every row then sits one place BELOW the diagonal and what is left on the
    diagonal is the smaller -1 + 0.3 U, so every column needs the pivot search and a row swap.  The roll also brings the
    old last row, which has nothing in column 0, to the top: entry (0, 0) is an exact zero, and an elimination that
    keeps the diagonal as its pivot stops there (tests/test_solver_ref.py asserts both)."""
    rng = np.random.default_rng(seed)
    A = tri(n)
    for d in (1, 2):
        if n - d > 0:
            A = A + sp.diags([0.3 * rng.random(n - d)], [d], shape=(n, n))
    A = sp.csr_matrix(np.roll(A.toarray(), 1, axis=0))
    A.sort_indices()
    return A


def singular(n):
    """tri(n) with its last row a copy of the first: exactly singular, and the elimination meets an exact zero column"""
    D = tri(n).toarray()
    D[n - 1, :] = D[0, :]
    return sp.csr_matrix(D)


# ---------------------------------------------------------------------------
# the cases of the GPU module (tests/test_solver_ref.py proves each of them fair)
TRI_SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 600, 1023, 1024)
FAMILY_SIZES = (9, 65, 257, 1024)
CG_TOL, CG_MAX_ITER = 1e-12, 150

_BUILD = {"tri": lambda n: tri(n), "band17": lambda n: band17(n, 17 + n), "arrow": lambda n: arrow(n),
          "dense_spd": lambda n: dense_spd(n, 5 + n), "shifted": lambda n: shifted(n, 29 + n)}

CG_CASES = ([("tri", n) for n in TRI_SIZES] + [(f, n) for f in ("band17", "arrow") for n in FAMILY_SIZES] + [("dense_spd", 200)])
DIRECT_CASES = CG_CASES + [("shifted", n) for n in FAMILY_SIZES]
CAPPED_CASES = (("tri", 300), ("band17", 300))                       # CG_coarsest_max_iter = 6
EARLY_OUT_CASES = (("tri", 257), ("tri", 1025))                      # rhs = 0 and ||rhs|| = 1e-13
FALLBACK_CASES = (("tri", 1025), ("band17", 1025), ("arrow", 1025))  # more rows than the LDS solvers hold
KRYLOV_SIZES = (262401, 524545)                                      # solve_CG on tri(n): past 256 * 1024 rows (the dot's grid, which the fused
#                                                                      update runs on) and past 256 * 2048 (the direction update's grid)
# the block path (tests/test_gpu_block_solver_layer.py).  k_dense_solve_block<C> holds C = min(K, pow2floor(4096 / n)) columns of
# the right-hand side in LDS per pass: 512 rows at K = 8 fill it with C = 8, 513 to 1024 rows at K = 8 take two passes of C = 4,
# 1024 rows at K = 4 fill it with C = 4
BLOCK_DIRECT_CASES = ([("tri", n) for n in (1, 9, 64, 65, 511, 512, 513, 729, 1023, 1024)]
                      + [(f, n) for f in ("band17", "arrow", "shifted") for n in (257, 1024)] + [("dense_spd", 200)])
BLOCK_CG_CASES = [c for c in CG_CASES if c[1] in FAMILY_SIZES] + [("tri", 1023)]
BLOCK_NEW_CASES = sorted(set(BLOCK_DIRECT_CASES) - set(DIRECT_CASES))  # tri 511, 512, 513, 729: in no scalar list
TWO_LEVEL = ((262401, 257), (524545, 513))                           # tri_two_level: 1022 and 1023 coarse rows; the fine level is past
#                                                                      the grid of the block dot / update, the second past the direction's too
# every size at which a block vector kernel takes another path: wave and block edges, the second grid-stride trip of the dot and
# the fused update (n > 256 * 1024) and of direction / pack / unpack (n > 256 * 2048)
BLOCK_VEC_SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 100003, 262144, 262145, 262401, 524288, 524289, 1048577)
ALL_CASES = sorted(set(DIRECT_CASES) | set(CAPPED_CASES) | set(EARLY_OUT_CASES) | set(FALLBACK_CASES) | set(BLOCK_DIRECT_CASES))

_cache = {}


def rhs_for(n):
    """smooth, sign-changing, no zero entry; the same closed form as tests/inputs.rhs2"""
    return np.cos(0.05 * np.arange(n, dtype=np.float64)) - 0.3


def case(family, n):
    """-> dict(A (scipy CSR), dense, rhs, x (solve_hp), resid, cond), computed once and shared: treat as read-only"""
    key = (family, n)
    if key not in _cache:
        A = _BUILD[family](n)
        D = A.toarray()
        b = rhs_for(n)
        x, resid = solve_hp(D, b)
        for a in (D, b, x):
            a.setflags(write=False)
        _cache[key] = dict(A=A, dense=D, rhs=b, x=x, resid=resid, cond=float(np.linalg.cond(D)))
    return _cache[key]


_COL_SCALE = (1.0, 0.0, -2.5, 0.75, 4.0, 1.5, -1.0, 3.0)


def coarse_columns(family, n, K):
    """-> (RHS (n, K), X (n, K)): column j is case(family, n)["rhs"] times _COL_SCALE[j] plus 0.1 j, column 1 all zero; X its
    solve_hp solutions.  A column does not depend on K.  Computed once and shared: treat as read-only"""
    c = case(family, n)
    for j in range(K):
        if (family, n, j) not in _cache:
            b = _COL_SCALE[j] * c["rhs"] + (0.1 * j if j != 1 else 0.0)
            x = solve_hp(c["dense"], b)[0] if j != 1 else np.zeros(n)
            b.setflags(write=False); x.setflags(write=False)
            _cache[(family, n, j)] = (b, x)
    cols = [_cache[(family, n, j)] for j in range(K)]
    return np.stack([b for b, _ in cols], axis=1), np.stack([x for _, x in cols], axis=1)


def tri_two_level(n, agg):
    """-> ([A, Ac], [P], [R]): A = tri(n), P piecewise constant (ones) over aggregates of `agg` consecutive rows, R = P^T,
    Ac = R A P with sorted indices (tridiagonal, ceil(n / agg) rows)"""
    A = tri(n)
    nc = -(-n // agg)
    P = sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) // agg)), shape=(n, nc))
    R = P.T.tocsr()
    Ac = (R @ A @ P).tocsr()
    Ac.sort_indices()
    R.sort_indices()
    return [A, Ac], [P], [R]


def block_columns(n, K):
    """-> K distinct right-hand sides of n rows (a list).  Smooth ones (1 and 7) that the coarse level takes most of, rough ones
    that the smoother takes, a single spike, a seeded random one: they reach a tolerance at different iterations"""
    i = np.arange(n, dtype=np.float64)
    spike = np.zeros(n)
    spike[n // 2] = 1.0
    cols = [rhs_for(n), np.sin(0.001 * i), np.random.default_rng(7 + n).standard_normal(n), spike,
            1.0 + 0.5 * np.sin(0.2 * i), (1.0 - 2.0 * (np.arange(n) % 2)) * (1.0 + 0.1 * np.cos(0.01 * i)), i / n - 0.5, np.cos(0.0003 * i)]
    return cols[:K]


# ---------------------------------------------------------------------------
# references
def residual_hp(A, x, b):
    """||b - A x||_2 with the products and sums in np.longdouble; A dense or scipy sparse"""
    x = np.asarray(x, np.longdouble)
    b = np.asarray(b, np.longdouble)
    if sp.issparse(A):
        A = A.tocsr()
        prod = A.data.astype(np.longdouble) * x[A.indices]
        if A.shape[0] and np.diff(A.indptr).min() > 0:          # no empty row: a row's products added in stored order, quickly
            Ax = np.add.reduceat(prod, A.indptr[:-1])
        else:
            Ax = np.zeros(A.shape[0], np.longdouble)
            np.add.at(Ax, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), prod)
    else:
        Ax = np.asarray(A, np.longdouble) @ x
    r = b - Ax
    return float(np.sqrt(np.sum(r * r)))


def solve_hp(A, b):
    """float64 LU followed by three rounds of iterative refinement whose residuals b - A x are formed in np.longdouble.
    -> (x rounded to float64, ||b - A x|| / ||b|| of the unrounded x)"""
    D = A.toarray() if sp.issparse(A) else np.asarray(A, np.float64)
    Dl = D.astype(np.longdouble)
    bl = np.asarray(b, np.longdouble)
    x = np.linalg.solve(D, np.asarray(b, np.float64)).astype(np.longdouble)
    for _ in range(3):
        r = bl - Dl @ x
        x = x + np.linalg.solve(D, r.astype(np.float64)).astype(np.longdouble)
    r = bl - Dl @ x
    nb = float(np.sqrt(np.sum(bl * bl)))
    return x.astype(np.float64), float(np.sqrt(np.sum(r * r))) / max(nb, 1e-300)


def dot_hp(x, y):
    """sum of np.longdouble products, as np.longdouble"""
    return np.sum(np.asarray(x, np.longdouble) * np.asarray(y, np.longdouble))


def dot_blocks(n):
    return min(N_PARTIALS, max(1, -(-n // BLOCK)))


def dot_roundings(n):
    """Roundings on the longest path from an input element to sgpu_dot's result (k_dot_partial + k_reduce_partials), plus
    one for rounding the reference to float64: a thread's sequential adds over its grid-stride trips, the product, the
    64-lane butterfly (6), the 4 wave sums, then in the second kernel a thread's adds of the partials, the butterfly, the
    4 wave sums."""
    nb = dot_blocks(n)
    return -(-n // (BLOCK * nb)) + 1 + 6 + 4 + -(-nb // BLOCK) + 6 + 4 + 1


def dot_bound(x, y):
    """|got - ref| <= k u sum|x_i y_i| / (1 - k u), k = dot_roundings(n)"""
    k = dot_roundings(len(x))
    s = float(np.sum(np.abs(np.asarray(x, np.longdouble) * np.asarray(y, np.longdouble))))
    return k * U * s / (1 - k * U)


def dot_inputs(n, kind, seed=0):
    """-> (x, y) float64.  normal: mixed signs; positive: no cancellation at all; cancelling: the second half-block undoes
    the first (y[h:2h] = -y[:h], x[h:2h] = x[:h]), so the exact result is small against sum|x y|.  seed: another pair of the
    same kind (the columns of a block)"""
    rng = np.random.default_rng(1000 + n + 7919 * 1000 * seed)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    if kind == "positive":
        x, y = np.abs(x) + 0.5, np.abs(y) + 0.5
    elif kind == "cancelling":
        h = n // 2
        x[h:2 * h] = x[:h]
        y[h:2 * h] = -y[:h]
    else:
        assert kind == "normal"
    return x, y


# ---------------------------------------------------------------------------
# float64 restatements of what the kernels compute
def _butterfly64(v):
    """group_sum<64> on the last axis (64 lanes): v += v[lane ^ off], off = 32 .. 1; lane 0 holds the result"""
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    return v[..., 0]


def _block_sums(v):
    """v: (blocks, 256) per-thread values -> per-block sums the way block_sum forms them"""
    w = _butterfly64(v.reshape(v.shape[0], BLOCK // 64, 64))          # (blocks, 4 waves)
    t = np.zeros(v.shape[0])
    for k in range(BLOCK // 64):
        t = t + w[:, k]
    return t


def dot_blocked(x, y):
    """sgpu_dot's summation order in float64 numpy: nb blocks of 256 threads, thread (b, t) adds the products of elements
    b*256 + t + k*256*nb in order of k; block_sum; one block adds the nb partials the same way"""
    n = len(x)
    nb = dot_blocks(n)
    trips = max(1, -(-n // (BLOCK * nb)))
    prod = np.zeros(trips * nb * BLOCK)
    prod[:n] = np.asarray(x, np.float64) * np.asarray(y, np.float64)
    prod = prod.reshape(trips, nb, BLOCK)
    s = np.zeros((nb, BLOCK))
    for k in range(trips):
        s = s + prod[k]
    partial = _block_sums(s)
    trips2 = -(-nb // BLOCK)
    p = np.zeros(trips2 * BLOCK)
    p[:nb] = partial
    p = p.reshape(trips2, BLOCK)
    s2 = np.zeros((1, BLOCK))
    for k in range(trips2):
        s2 = s2 + p[k]
    return float(_block_sums(s2)[0])


def pcg_update(num, den, p, h, u, r):
    """k_pcg_update_block on one column, a rounding per operation: alpha = num / den; -> (u - alpha p, r - alpha h)"""
    alpha = np.float64(num) / np.float64(den)
    return u - alpha * p, r - alpha * h


def pcg_direction(num, den, z, p):
    """k_pcg_direction_block on one column: beta = num / den; -> 1 z + beta p"""
    beta = np.float64(num) / np.float64(den)
    return 1.0 * z + beta * p


def coarsest_cg(A, rhs, u0=None, tol=CG_TOL, max_iter=CG_MAX_ITER):
    """solve_coarsest_CG as the oracle states it (oracle/saena_oracle.c, orc_solve_coarsest_CG), float64 numpy.
    -> (u, reported iterations)"""
    rhs = np.asarray(rhs, np.float64)
    u = np.zeros(len(rhs)) if u0 is None else np.array(u0, np.float64)
    res, dirv = rhs.copy(), rhs.copy()
    initial_dot = float(res @ res)
    thres = initial_dot * tol * tol
    dot = initial_dot
    if dot < tol * tol:
        max_iter = 0
    i = 1
    while i < max_iter:
        mt = A @ dirv
        factor = dot / float(dirv @ mt)
        u += factor * dirv
        res -= factor * mt
        dot_prev = dot
        dot = float(res @ res)
        if dot < thres:
            break
        dirv = res + (dot / dot_prev) * dirv
        i += 1
    if i == max_iter and max_iter != 0:
        i -= 1
    return u, i


class Singular(ArithmeticError):
    pass


def gauss_jordan_inverse(D, pivot=True):
    """The dense inverse as sgpu_amg_create forms it on the host: Gauss-Jordan on [A | I], partial pivoting (first
    largest |a| at or below the diagonal), the pivot row scaled by 1/pivot, an exact-zero pivot refused.
    -> (inverse, number of row swaps).  pivot=False keeps the diagonal: what a missing pivot search would compute.
    The arithmetic is the library's, rounding for rounding: every row but the pivot's has f times the pivot row taken
    off it, a product and then a difference (singular(65) ends in the exact zero the library refuses).  The library
    skips the rows whose f is zero; here they have zeros taken off them, which changes no value."""
    a = np.array(D, np.float64)
    n = a.shape[0]
    inv = np.eye(n)
    t = np.empty((n, n))
    swaps = 0
    for c in range(n):
        piv = c + int(np.argmax(np.abs(a[c:, c]))) if pivot else c
        if a[piv, c] == 0.0:
            raise Singular("coarsest operator is singular")
        if piv != c:
            a[[piv, c]] = a[[c, piv]]
            inv[[piv, c]] = inv[[c, piv]]
            swaps += 1
        d = 1.0 / a[c, c]
        a[c] *= d
        inv[c] *= d
        f = a[:, c].copy()
        f[c] = 0.0
        for m in (a, inv):
            np.multiply.outer(f, m[c], out=t)
            m -= t
    return inv, swaps


def inverse(family, n):
    """gauss_jordan_inverse of case(family, n), computed once (seconds at 1024 rows) and shared: treat as read-only"""
    if ("inv", family, n) not in _cache:
        _cache[("inv", family, n)] = gauss_jordan_inverse(case(family, n)["dense"])
        _cache[("inv", family, n)][0].setflags(write=False)
    return _cache[("inv", family, n)]


def direct_bound(n, cond):
    """||u - x|| / ||x|| of u = inverse(A) rhs: 4 (n + 4) u cond_2(A)"""
    return 4 * (n + 4) * U * cond


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def vec_sizes():
    """every size at which a vector kernel takes another path: the double2 body against the scalar tail (1, 2, 3), wave and
    block edges, the first grid-stride trip of the dot (n > 256 * 1024) and of fill/axpby (n > 2 * 256 * 2048)"""
    return (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 100003, 262144, 262145, 262401, 1048576, 1048577, 2097155)

