"""Operands for tests/test_spgemm_conformance.py, one builder per case, and the check every product goes through.

Every operand is generated here from seeded generators (or read from tests/golden/matrices); the rows of B are distinct
and ascending, always: the kernels' precondition (sgpu_spgemm.hip, gpu_spgemm) is honoured, never probed.

The dispatch of the two kernels is restated below from their documentation, NOT read from them, so that a product's
statistics (host.spgemm_stats) can be compared with what the operands call for, row by row:
  device (sgpu_spgemm.hip)  upper bound ub = min(products of the row, columns of B); ub = 0: nothing runs; ub <= 256
      light; ub <= 2048 medium; else the 4096-slot table is tried and the row abandoned iff it touches more than 3072
      distinct columns; abandoned rows go to the LDS accumulator (windows of 20 224 columns) when B has at most 16
      windows and SAENA_SPGEMM_NO_LDS is unset, else to the HBM accumulator; consecutive rows form a chunk until the
      next row's ub would lift the chunk's sum over the chunk size (SAENA_SPGEMM_CHUNK_ENTRIES, default 384 Mi); a row
      whose ub alone exceeds it makes the device decline;
  host (amg_setup.cpp)      products > columns of B / 8: dense accumulator, else the hash accumulator.
"""
import os
from collections import namedtuple

import numpy as np

from saena_amd import host
from saena_amd.capi import SgpuError
from tests import spgemm_ref as R

LIGHT_UB, MEDIUM_UB, TABLE_FILL, TABLE_SLOTS, WINDOW, MAX_WINDOWS = 256, 2048, 3072, 4096, 20224, 16
DEFAULT_CHUNK = 384 << 20

# must: the counters that have to be positive for the case to deserve its name (device leg / host leg)
Product = namedtuple("Product", "name A B row_offset split_row must must_host env")


def product(name, A, B, row_offset=0, split_row=None, must=(), must_host=(), env=None):
    return Product(name, A, B, row_offset, split_row, tuple(must), tuple(must_host), dict(env or {}))


def values(rng, n):
    """magnitudes over 16 binades, both signs: sums round, and round differently in another order"""
    return rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-8, 9, n)


def brow(rng, pool, count):
    """`count` distinct columns of `pool`, ascending, with values"""
    c = np.sort(rng.choice(pool, int(count), replace=False))
    return c, values(rng, len(c))


def arow(rng, cols):
    cols = np.asarray(cols, np.int64)
    return cols, values(rng, len(cols))


# ---- expectations ---------------------------------------------------------------------------------------------------
def chunk_starts(ub, chunk):
    starts, s, start = [0], 0, 0
    for i, u in enumerate(ub):
        if i > start and s + u > chunk:
            starts.append(i); start = i; s = 0
        s += int(u)
    return starts


def expected_stats(A, B, info, which, env):
    E = info["E"]
    products = E.n_products
    touched = np.bincount(E.row, minlength=A.nrows)
    out = {k: 0 for k in host.SPGEMM_STATS}
    if which == "host":
        dense = products > B.ncols // 8
        out.update(host_dense=int(dense.sum()), host_hash=int((~dense).sum()))
        return out
    ub = np.minimum(products, B.ncols)
    chunk = min(DEFAULT_CHUNK, max(1, int(env.get("SAENA_SPGEMM_CHUNK_ENTRIES", DEFAULT_CHUNK))))
    heavy = ub > MEDIUM_UB
    abandoned = heavy & (touched > TABLE_FILL)
    windows = -(-B.ncols // WINDOW)
    lds = windows <= MAX_WINDOWS and "SAENA_SPGEMM_NO_LDS" not in env
    out.update(light=int(((ub > 0) & (ub <= LIGHT_UB)).sum()), medium=int(((ub > LIGHT_UB) & (ub <= MEDIUM_UB)).sum()),
               try_kept=int((heavy & ~abandoned).sum()), try_abandoned=int(abandoned.sum()),
               lds=int(abandoned.sum()) if lds else 0, hbm=0 if lds else int(abandoned.sum()),
               chunks=len(chunk_starts(ub, chunk)), windows=windows if lds and abandoned.any() else 0, on_device=1)
    return out


class _Env:
    """the driver reads its switches per call: set for one product, restored after it"""

    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check(L, which, p, log=None):
    """one product against both references and its expected paths; `which`: "host" or "device".  Returns the statistics."""
    A, B = p.A, p.B
    R.check_operands(A, B)
    env = dict(p.env)
    for k in ("SAENA_SPGEMM_NO_LDS", "SAENA_SPGEMM_CHUNK_ENTRIES"):       # what the process was started with counts as well
        if k in os.environ:
            env.setdefault(k, os.environ[k])
    ptr, col, val, info = R.sequential(A, B, p.row_offset)
    with _Env(p.env):
        got_ptr, got_col, got_val = host.spgemm(L, A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.ncols, p.row_offset, mode=which, split_row=p.split_row)
    stats = host.spgemm_stats(L)
    line = f"{p.name} [{which}] {A.nrows}x{A.ncols}x{B.ncols} -> {len(col)} entries: " + " ".join(f"{k}={v}" for k, v in stats.items() if v)
    print(line)
    if log is not None:
        log.append(line)
    # 1. the pattern, exactly
    np.testing.assert_array_equal(got_ptr, ptr, err_msg=f"{p.name}: row pointers")
    np.testing.assert_array_equal(got_col, col, err_msg=f"{p.name}: columns")
    # 2. the values, bit for bit
    R.assert_same_values(got_val, val, p.name)
    # 3. within the exact sum's bound (finite entries); the sequential reference is held to it as well
    E, keep = info["E"], info["keep"]
    ex, S = R.exact(E)
    lim = R.bound(E, S)
    fin = np.isfinite(S[keep])
    assert np.all(np.abs(val[fin] - ex[keep][fin]) <= lim[keep][fin]), f"{p.name}: the sequential reference leaves the exact sum's bound"
    over = np.flatnonzero(~(np.abs(got_val[fin] - ex[keep][fin]) <= lim[keep][fin]))
    assert len(over) == 0, f"{p.name}: {len(over)} values outside n eps S of the exact sum"
    dropped = ~keep & np.isfinite(S)                                        # what was dropped is ~0 by the same measure
    assert np.all(np.abs(ex[dropped]) <= R.DROP + lim[dropped]), f"{p.name}: an entry far from zero was dropped"
    # 4. the path every row took
    want = expected_stats(A, B, info, which, env)
    rehash = stats.pop("host_rehash")
    want.pop("host_rehash")
    assert stats == want, f"{p.name}: rows per path {stats}, the operands call for {want}"
    stats["host_rehash"] = rehash
    for k in (p.must_host if which == "host" else p.must):
        assert stats[k] > 0, f"{p.name}: no row on '{k}', the path this case is named after ({stats})"
    return stats


# ---- the cases ------------------------------------------------------------------------------------------------------
def case_light():
    rng = np.random.default_rng(101)
    k, n, m = 300, 3000, 210
    allc = np.arange(n)
    Brows = [(np.zeros(0, np.int64), np.zeros(0)) if r % 9 == 4 else brow(rng, allc, rng.integers(1, 41)) for r in range(k)]
    Brows[0], Brows[1], Brows[2] = brow(rng, allc, 128), brow(rng, allc, 128), brow(rng, allc, 129)
    Arows = [(np.zeros(0, np.int64), np.zeros(0)) if i % 7 == 3 else arow(rng, rng.choice(k, rng.integers(1, 41), replace=False)) for i in range(m)]
    Arows[0] = arow(rng, [0, 1])                     # 256 products: the last light row
    Arows[1] = arow(rng, [2, 0])                     # 257: the first medium row
    Arows[2] = arow(rng, [4, 13, 22])                # every row of B it names is empty: upper bound 0
    Arows[4] = arow(rng, [4, 5, 13, 6])              # empty rows of B among others
    out = [product("light", R.csr(Arows, k), R.csr(Brows, n), must=["light", "medium"], must_host=["host_hash"])]
    for ncols in (256, 257):                         # the same boundary through ub = min(products, columns of B)
        rng = np.random.default_rng(102)
        Brows = [brow(rng, np.arange(ncols), rng.integers(100, 201)) for _ in range(40)]
        Brows[39] = brow(rng, np.arange(ncols), 20)
        Arows = [arow(rng, rng.choice(39, rng.integers(3, 7), replace=False)) for _ in range(30)]
        Arows[7] = arow(rng, [39])
        out.append(product(f"light.cols{ncols}", R.csr(Arows, 40), R.csr(Brows, ncols), must=["light"] if ncols == 256 else ["light", "medium"],
                           must_host=["host_dense"]))
    return out


def case_medium():
    rng = np.random.default_rng(201)
    k, n = 80, 6000
    allc = np.arange(n)
    Brows = [brow(rng, allc, rng.integers(100, 501)) for _ in range(k)]
    for r in (0, 1, 2, 4):
        Brows[r] = brow(rng, allc, 512)
    Brows[3] = brow(rng, allc, 513)
    Arows = [arow(rng, rng.choice(np.arange(5, k), rng.integers(2, 7), replace=False)) for _ in range(60)]
    Arows[0] = arow(rng, [0, 1, 2, 4])               # upper bound 2048: the last medium row
    Arows[1] = arow(rng, [0, 1, 2, 3])               # 2049: the first row that tries the table
    Arows[2] = arow(rng, [7, 9, 7, 11, 9])           # a row of A may name a row of B twice: two products, in sequence
    Arows[3] = arow(rng, [20, 20, 20, 20])
    return [product("medium", R.csr(Arows, k), R.csr(Brows, n), must=["medium", "try_kept"], must_host=["host_dense", "host_hash"])]


def case_try():
    rng = np.random.default_rng(301)
    n = 5000
    perm = rng.permutation(n)
    p3000, p3072, p3073 = np.sort(perm[:3000]), np.sort(perm[1000:4072]), np.sort(perm[1500:4573])
    Brows = [brow(rng, p3000, 500) for _ in range(30)]                                   # 0..29
    Brows += [(c, values(rng, len(c))) for c in np.array_split(p3072, 6)]                # 30..35: together exactly 3072 columns
    Brows += [brow(rng, p3072, 500) for _ in range(24)]                                  # 36..59
    Brows += [(c, values(rng, len(c))) for c in np.array_split(p3073, 7)]                # 60..66: together 3073
    Brows += [brow(rng, p3073, 500) for _ in range(23)]                                  # 67..89
    Brows += [brow(rng, np.arange(n), 4500)]                                             # 90: longer than the 4096-slot table
    Brows += [brow(rng, np.arange(n), 300) for _ in range(5)]                            # 91..95
    Arows = [arow(rng, rng.choice(30, 24, replace=False)),          # 12 000 products on <= 3000 columns: kept by the table
             arow(rng, rng.permutation(np.arange(30, 60))),         # 15 072 products on exactly 3072: kept
             arow(rng, rng.permutation(np.arange(60, 90))),         # on 3073: abandoned
             arow(rng, [90, 91, 92]),                               # the table fills inside the first step
             arow(rng, [91, 90, 93]),                               # ... inside the second
             arow(rng, np.concatenate([rng.choice(30, 20, replace=False), [95, 94]])),
             arow(rng, [91]), arow(rng, [])]
    A, B = R.csr(Arows, len(Brows)), R.csr(Brows, n)
    touched = np.bincount(R.expand(A, B).row, minlength=A.nrows)
    assert touched[1] == TABLE_FILL and touched[2] == TABLE_FILL + 1 and touched[0] <= 3000 and touched[3] > TABLE_SLOTS
    return [product("try", A, B, must=["try_kept", "try_abandoned", "lds"], must_host=["host_dense"])]


def wide_operands(ncols, seed):
    """rows that overflow the table on a B of `ncols` columns, with entries at the window edges and at the last column"""
    rng = np.random.default_rng(seed)
    allc = np.arange(ncols)
    windows = -(-ncols // WINDOW)
    Brows = [brow(rng, allc, 600) for _ in range(50)]
    edge = np.unique([c for c in (0, WINDOW - 1, WINDOW, 2 * WINDOW - 1, 2 * WINDOW, ncols - 2, ncols - 1) if 0 <= c < ncols])
    for r in (0, 1):
        c = np.union1d(Brows[r][0], edge)
        Brows[r] = (c, values(rng, len(c)))
    Arows = [arow(rng, np.concatenate([[0], rng.choice(np.arange(2, 50), 8, replace=False), [1]])),
             arow(rng, rng.choice(50, 9, replace=False)),
             arow(rng, [1, 0]), arow(rng, []), arow(rng, [3])]
    late = []                                                    # rows whose columns all lie in ONE window that is not the first
    for w in sorted({windows - 1, windows // 2}):
        lo, hi = w * WINDOW, min((w + 1) * WINDOW, ncols)
        if w == 0 or hi - lo < 8000:
            continue
        first = len(Brows)
        Brows += [brow(rng, np.arange(lo, hi), 600) for _ in range(10)]
        Arows.append(arow(rng, np.arange(first, first + 10)))
        late.append(len(Arows) - 1)
    A, B = R.csr(Arows, len(Brows)), R.csr(Brows, ncols)
    touched = np.bincount(R.expand(A, B).row, minlength=A.nrows)
    assert touched[0] > TABLE_FILL and touched[1] > TABLE_FILL and all(touched[i] > TABLE_FILL for i in late)
    return A, B


LDS_COLS = [WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW - 1, 2 * WINDOW, 2 * WINDOW + 1, MAX_WINDOWS * WINDOW]


def case_lds(max_cols=None):
    return [product(f"lds.cols{n}", *wide_operands(n, 400 + i), must=["try_abandoned", "lds"], must_host=["host_hash"])
            for i, n in enumerate(LDS_COLS) if max_cols is None or n <= max_cols]


def case_hbm():
    """one column more than 16 windows: no LDS form"""
    return [product("hbm.cols%d" % (MAX_WINDOWS * WINDOW + 1), *wide_operands(MAX_WINDOWS * WINDOW + 1, 450), must=["try_abandoned", "hbm"])]


def case_hbm_no_lds():
    """the `lds` operands of up to two windows and a column (512 accumulators of 12 B x 40 449 columns = 0.25 GB) for a process
    started with SAENA_SPGEMM_NO_LDS=1"""
    return [p._replace(name=p.name.replace("lds", "hbm.nolds"), must=("try_abandoned", "hbm")) for p in case_lds(2 * WINDOW + 1)]


CHUNK = 50000


def chunk_operands():
    rng = np.random.default_rng(501)
    n, k, m = 6000, 3000, 3000
    allc = np.arange(n)
    Brows = [brow(rng, allc, 100) for _ in range(2989)] + [brow(rng, allc, 2000)] + [brow(rng, allc, 500) for _ in range(10)]
    Arows = [arow(rng, []) if i % 11 == 5 else arow(rng, rng.choice(2989, rng.integers(1, 4), replace=False)) for i in range(m)]
    for i in range(m - 4, m):                                        # rows that overflow the table, in the last chunk
        Arows[i] = arow(rng, rng.permutation(np.arange(2990, 3000)))
    ub = np.array([100 * len(c) for c, _ in Arows])
    ub[m - 4:] = 5000
    b = chunk_starts(ub, CHUNK)[1]
    Arows[b - 1] = arow(rng, [])                                     # a chunk boundary directly after an empty row ...
    Arows[b] = arow(rng, [2989])                                     # ... (the row behind it is large enough to keep the boundary there)
    A, B = R.csr(Arows, k), R.csr(Brows, n)
    E = R.expand(A, B)
    ub = np.minimum(E.n_products, n)
    starts = chunk_starts(ub, CHUNK)
    touched = np.bincount(E.row, minlength=m)
    assert len(starts) >= 3 and b in starts and ub[b - 1] == 0 and starts[-1] > 0 and np.all(touched[m - 4:] > TABLE_FILL)
    assert len(A.col) + len(B.col) >= 200000                          # "auto" asks the device
    return A, B, int(ub.max())


def case_chunks():
    A, B, _ = chunk_operands()
    return [product("chunks", A, B, must=["light", "medium", "try_abandoned"], env={"SAENA_SPGEMM_CHUNK_ENTRIES": str(CHUNK)})]


def case_offsets():
    """n = 400: the host's dense accumulator serves the crafted rows, n = 4000: its hash accumulator"""
    return offsets_products(400, "host_dense") + offsets_products(4000, "host_hash")


def offsets_products(n, host_path):
    rng = np.random.default_rng(601)
    m, k, off = 150, 200, 37
    targets = (5, 41, 77)
    reserved = sorted({t for t in targets} | {t + off for t in targets} | {300})
    pool = np.setdiff1d(np.arange(n), reserved)
    Brows = [brow(rng, pool, rng.integers(5, 31)) for _ in range(k - 2)]
    twin = (np.array(reserved), values(rng, len(reserved)))
    Brows += [twin, (twin[0].copy(), twin[1].copy())]                 # rows 198 and 199: the same entries
    Arows = [arow(rng, rng.choice(k - 2, rng.integers(3, 13), replace=False)) for _ in range(m)]
    for t in targets:                                                # 2.5 x ... - 2.5 x: exact zeros at (t, t), (t, t + 37) and (t, 300)
        c, v = Arows[t]
        Arows[t] = (np.concatenate([[198], c, [199]]), np.concatenate([[2.5], v, [-2.5]]))
    A, B = R.csr(Arows, k), R.csr(Brows, n)
    out = []
    for ro in (0, off):
        ptr, col, val, _ = R.sequential(A, B, ro)
        for t in targets:                                            # the zero on the GLOBAL diagonal stays, the others go
            rowc = col[ptr[t]:ptr[t + 1]]
            assert (t + ro in rowc) and val[ptr[t]:ptr[t + 1]][list(rowc).index(t + ro)] == 0.0
            assert (t + off - ro) not in rowc and 300 not in rowc
        out.append(product(f"offsets.cols{n}.ro{ro}", A, B, row_offset=ro, must=["light"], must_host=[host_path]))
        out.append(product(f"offsets.cols{n}.ro{ro}.split", A, B, row_offset=ro, split_row=120, must=["light"], must_host=[host_path]))
    return out


NEXT = float(np.nextafter(1e-14, 1.0))


def case_threshold():
    """sums on the drop threshold and order-visible cancellation in a light, a medium and a table-overflowing row (the last
    one lands on the LDS accumulator, or on the HBM accumulator in a process started with SAENA_SPGEMM_NO_LDS=1); once with
    row_offset = 0 and once with 50, where the kept zero is the one at (i, i + 50)"""
    rng = np.random.default_rng(701)
    n, x = 30000, 0.7310585786300049
    c = dict(plus=100, minus=101, next=102, zero=103, lost=104, kept=105, twice=106)
    diagonals = (0, 1, 2, 50, 51, 52)
    pool = np.arange(200, n)
    Brows = [brow(rng, pool, 500) for _ in range(40)] + [brow(rng, pool, 30) for _ in range(5)]
    s0 = {c["plus"]: 1e-14, c["minus"]: -1e-14, c["next"]: NEXT, c["zero"]: x, c["lost"]: 1e16, c["kept"]: 1e16, c["twice"]: 0.5e-14}
    s1 = {c["zero"]: -x, c["lost"]: 1.0, c["kept"]: -1e16, c["twice"]: 0.5e-14}
    s2 = {c["lost"]: -1e16, c["kept"]: 1.0}
    s0.update({d: x for d in diagonals})
    s1.update({d: -x for d in diagonals})
    for s in (s0, s1, s2):
        Brows.append((np.array(sorted(s)), np.array([s[j] for j in sorted(s)])))
    k = len(Brows)
    S0, S1, S2 = k - 3, k - 2, k - 1
    one = lambda cols: (np.asarray(cols, np.int64), np.ones(len(cols)))
    Arows = [one([S0, 40, S1, 41, S2]),                                            # light
             one([S0, 3, S1, 5, S2]),                                               # medium
             one([S0, S1] + list(rng.choice(40, 10, replace=False)) + [S2]),        # overflows the table
             one([S2, S1, S0])]                                                     # the other order: neither survives
    A, B = R.csr(Arows, k), R.csr(Brows, n)
    out = []
    for ro in (0, 50):
        ptr, col, val, _ = R.sequential(A, B, ro)
        for i in (0, 1, 2):              # what the contract says about the crafted entries, checked on the reference itself
            row = dict(zip(col[ptr[i]:ptr[i + 1]].tolist(), val[ptr[i]:ptr[i + 1]].tolist()))
            assert row[c["next"]] == NEXT and row[c["kept"]] == 1.0 and row[i + ro] == 0.0
            assert not any(c[q] in row for q in ("plus", "minus", "zero", "lost", "twice")) and not any(d in row for d in diagonals if d != i + ro)
        row = dict(zip(col[ptr[3]:ptr[4]].tolist(), val[ptr[3]:ptr[4]].tolist()))
        assert c["lost"] not in row and c["kept"] not in row    # -1e16 + 1 + 1e16 = 0 and 1 + -1e16 + 1e16 = 0 in that order
        out.append(product(f"threshold.ro{ro}", A, B, row_offset=ro, must=["light", "medium", "try_abandoned"], must_host=["host_hash", "host_dense"]))
    return out


def case_specials():
    rng = np.random.default_rng(801)
    n, k = 3000, 60
    pool = np.arange(10, n)
    Brows = [brow(rng, pool, 100) for _ in range(k)]
    Brows[59] = (np.array([0, 1, 2]), np.array([-1e-200, -1e-200, -0.0]))           # products -0.0 on the diagonals of rows 0, 1, 2
    c, v = Brows[12]
    Brows[12] = (np.concatenate([[7], c]), np.concatenate([[np.nan], v]))            # a NaN that lands on the diagonal of row 7
    Brows[10][1][5], Brows[11][1][50], Brows[13][1][0] = -np.inf, np.nan, np.inf
    Arows = [arow(rng, [1, 2]) for _ in range(12)]
    Arows[0] = (np.array([59, 20, 21]), np.array([1e-200, 1.5, -2.0]))               # light; its diagonal entry has the one product -0.0
    Arows[1] = (np.concatenate([[59], np.arange(20, 28)]), np.concatenate([[1e-200], values(rng, 8)]))      # medium
    Arows[2] = (np.concatenate([[59], np.arange(20, 50)]), np.concatenate([[1.0], values(rng, 30)]))        # tries the table, kept
    Arows[3] = arow(rng, [10, 30]); Arows[4] = arow(rng, [30, 11, 31]); Arows[5] = arow(rng, [13, 10, 32])
    Arows[6] = (np.array([33, 34]), np.array([np.inf, 1.0]))
    Arows[7] = arow(rng, [12, 35])
    Arows[8] = (np.array([36, 37, 36]), np.array([np.nan, 2.0, 1.0]))
    Arows[9] = (np.array([38, 38]), np.array([np.inf, -np.inf]))                     # Inf - Inf: NaN, dropped off the diagonal
    A, B = R.csr(Arows, k), R.csr(Brows, n)
    ptr, col, val, info = R.sequential(A, B)
    for i in (0, 1, 2):
        assert col[ptr[i]] == i and R.bits(val[ptr[i]:ptr[i] + 1])[0] == 0, "0.0 + -0.0 is +0.0"
    assert col[ptr[7]] == 7 and np.isnan(val[ptr[7]]) and ptr[10] == ptr[9]          # NaN kept on the diagonal only
    E = info["E"]
    tainted = ~np.isfinite(np.add.reduceat(np.abs(E.prod), E.start))
    assert not np.any(~np.isfinite(info["value"]) & ~tainted), "only entries that take a non-finite product are non-finite"
    return [product("specials", A, B, must=["light", "medium", "try_kept"], must_host=["host_dense", "host_hash"])]


def case_rehash():
    """the host's hash accumulator starts at 256 slots for a short row of A and doubles at load 1/2: 3000 columns from one
    entry of A are five grow-and-rehash steps"""
    rng = np.random.default_rng(901)
    n = 40000
    Brows = [brow(rng, np.arange(n), 3000) for _ in range(10)] + [brow(rng, np.arange(n), 150) for _ in range(4)]
    Arows = [arow(rng, [r]) for r in range(10)] + [arow(rng, [10, 11, 12, 13]), arow(rng, [0, 1]), arow(rng, [10, 3])]
    return [product("rehash", R.csr(Arows, len(Brows)), R.csr(Brows, n), must=["try_kept"], must_host=["host_rehash", "host_hash", "host_dense"])]


def case_real():
    import scipy.sparse as sp

    from tests import hierarchy, matrices
    out = []
    for name in ("plat362", "fxm3_6", "SiH4"):
        e, M = matrices.entries(name)
        A = R.from_scipy(sp.csr_matrix((e["val"], (e["row"], e["col"])), shape=(M, M)))
        out.append(product(f"real.{name}^2", A, A))
    As, Ps, Rs = hierarchy.poisson_hierarchy(22, 4)
    for l in range(3):
        Rm, Am, Pm = R.from_scipy(Rs[l]), R.from_scipy(As[l]), R.from_scipy(Ps[l])
        RA = R.sequential(Rm, Am)
        RAm = R.Csr(RA[0], RA[1], RA[2], Rm.nrows, Am.ncols)
        out.append(product(f"real.RA.l{l}", Rm, Am))
        out.append(product(f"real.(RA)P.l{l}", RAm, Pm))
    return out


CASES = dict(light=case_light, medium=case_medium, **{"try": case_try}, lds=case_lds, hbm=case_hbm, chunks=case_chunks, offsets=case_offsets,
             threshold=case_threshold, specials=case_specials, rehash=case_rehash, real=case_real, hbm_no_lds=case_hbm_no_lds)


def run_case(L, which, name, log=None):
    return [check(L, which, p, log) for p in CASES[name]()]


def decline_legs(L, log=None):
    """a row whose upper bound alone exceeds the chunk: "device" reports that the kernel declined, "auto" asks it (the
    operands hold 200 000 stored entries), is declined and returns the host's product"""
    A, B, ub_max = chunk_operands()
    small = {"SAENA_SPGEMM_CHUNK_ENTRIES": str(ub_max - 1)}
    ptr, col, val, _ = R.sequential(A, B)
    args = (L, A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.ncols, 0)
    with _Env(small):
        try:
            host.spgemm(*args, mode="device")
            raise AssertionError("the device kernel multiplied a row larger than its chunk")
        except SgpuError as e:
            assert "declined" in str(e), e
        st = host.spgemm_stats(L)
        assert st["declined"] == 1 and st["on_device"] == 0 and st["host_hash"] + st["host_dense"] == 0, st
        got = host.spgemm(*args, mode="auto")
        st = host.spgemm_stats(L)
    line = "chunks.decline [auto] " + " ".join(f"{k}={v}" for k, v in st.items() if v)
    print(line)
    if log is not None:
        log.append(line)
    assert st["declined"] == 1 and st["on_device"] == 0 and st["host_hash"] + st["host_dense"] == A.nrows, st
    np.testing.assert_array_equal(got[0], ptr)
    np.testing.assert_array_equal(got[1], col)
    R.assert_same_values(got[2], val, "chunks.decline")
