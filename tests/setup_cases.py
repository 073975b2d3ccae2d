"""The operators the smoothed-aggregation setup is held to its restatement on (tests/setup_ref.py), named once.

  wgrid16   weighted 7-point grid graph, 16^3, weights over four decades, 15 % of the edges deleted: irregular degrees, a
            strength relation in which either of its two tests fires, a filter that drops entries from level 2 on
  wgrid36   the same at 36^3, cut at two coarsening steps: level 0 is above the 32 768 rows from which the aggregation
            deals its rounds to threads
  fxm3_6    a pattern matrix: every off-diagonal is +1, so the row maximum of -a_ik is negative in every row
  SiH4      mixed signs, 34 entries per row on average, rows of up to 205 entries (level 1 is nearly full)
  plat362   as the fixtures have it

`options(name)` are the setup's options of the case, `assemble(name, tmpdir)` is the assembled operator; what it looks
like after assemble() -- boundary rows removed -- is read back through level_layout(0, 0), never assumed."""
import numpy as np

from saena_amd import host
from tests import matrices

# SiH4: level 1 has 2 151 rows that are nearly full (2.1 M entries).  The first coarsening step multiplies 7.7e6 products for
# R A and 4.3e7 for (R A) P; the second would multiply 5.3e8 and 1.9e8.  max_level = 1 it is: the restatement then never
# holds more than setup_ref.CHUNK = 1e6 products at a time (it expands a product a block of rows at a time), and
# tests/test_setup_contract.py checks every product's count against MAX_PRODUCTS before any of it is expanded.
# wgrid36 is cut at two steps for the product (its second step: 2.8e7 and 7.9e7 products); the restatement's
# Galerkin product of that second step is taken on a sample of the coarse rows (tests/test_setup_contract.py).
MAX_PRODUCTS = 5 * 10 ** 7
MAX_LEVEL = {"wgrid36": 2, "SiH4": 1}
NAMES = ("wgrid16", "wgrid36", "fxm3_6", "SiH4", "plat362")
SYMMETRIC = ("wgrid16", "plat362", "fxm3_6")        # the inputs whose eigenvalue estimate is held against eigsh


def wgrid(m, seed, drop=0.15):
    """-> (rows, cols, vals) of a weighted 7-point grid graph on m^3 vertices: edge weights 10^U(-2, 2), a share `drop` of
    the edges deleted, off-diagonals -w, diagonal = sum of the row's weights + 1.  A vertex that loses all its edges is a
    row with nothing but its diagonal: assemble() removes it."""
    rng = np.random.default_rng(seed)
    idx = np.arange(m ** 3).reshape(m, m, m)
    a = np.concatenate([idx[:-1, :, :].ravel(), idx[:, :-1, :].ravel(), idx[:, :, :-1].ravel()])
    b = np.concatenate([idx[1:, :, :].ravel(), idx[:, 1:, :].ravel(), idx[:, :, 1:].ravel()])
    w = 10.0 ** rng.uniform(-2, 2, size=len(a))
    keep = rng.random(len(a)) >= drop
    a, b, w = a[keep], b[keep], w[keep]
    rows, cols, vals = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([-w, -w])
    diag = np.zeros(m ** 3)
    np.add.at(diag, rows, -vals)
    n = m ** 3
    return (np.concatenate([rows, np.arange(n)]).astype(np.int32), np.concatenate([cols, np.arange(n)]).astype(np.int32),
            np.concatenate([vals, diag + 1.0]))


WGRIDS = {"wgrid16": (16, 5), "wgrid36": (36, 3)}


def tiny_operators():
    """-> [(name, A, P, thre)]: three hand-made operators (tests/spgemm_ref.Csr) for the Galerkin product R A P, R = P^T, and
    for the filter at threshold thre, small enough for the plain double loops that pin the vectorised restatement"""
    from tests.spgemm_ref import csr
    u = 2.0 ** -53
    # 1: sums whose result depends on the order and on HOW OFTEN the diagonal is rounded: row 0 lumps 1e16, 1, -1e16 (in
    #    that order 0.0, in another 1.0), row 1 lumps u + u onto a diagonal of 1.0 (added once: 1 + 2u; entry by entry: 1.0)
    A1 = csr([([0, 1, 2, 3], [4.0, 1e16, 1.0, -1e16]), ([0, 1, 2], [u, 1.0, u]), ([0, 1, 2, 4], [-1.0, 1e-3, 5.0, -2.0]),
              ([0, 3, 5], [-0.5, 3.0, 1e-9]), ([2, 4, 5], [-2.0, 6.0, -1e-20]), ([3, 4, 5], [2e-9, -1e-20, 7.0])], 6)
    P1 = csr([([0], [1.0]), ([0, 1], [0.5, 0.25]), ([1], [1.0]), ([1, 2], [-0.125, 0.75]), ([2], [1.0]), ([0, 2], [1e-3, 0.3])], 3)
    # 2: rows without a diagonal entry -- its place is the front (row 0), the middle (row 2), the end (row 4) -- one of
    #    them (row 2) with small entries whose lump is then thrown away, and an empty row (row 5)
    A2 = csr([([1, 3], [-1.0, 1e-7]), ([0, 1], [-1.0, 2.0]), ([0, 1, 3, 4], [1e-7, -3.0, 2e-7, 4.0]), ([2, 3], [-1.0, 5.0]),
              ([0, 1, 2], [0.25, 1e-8, -0.5]), ([], [])], 6)
    P2 = csr([([0], [1.0]), ([0], [0.5]), ([1], [1.0]), ([0, 1], [0.25, 0.5]), ([1], [2.0]), ([1], [1.0])], 2)
    # 3: diagonals that lump to less than 1e-14 -- to exactly 0.0 (row 0), to 1e-19 (row 1), to -5e-15 (row 2) -- or to just
    #    above it (row 3: stays), a NaN off the diagonal (row 4: it fails "|v| > thre" and is lumped)
    A3 = csr([([0, 1, 2], [1e-3, -5e-4, -5e-4]), ([0, 1, 3], [-6e-4, 1e-3, -4e-4]), ([1, 2, 4], [-5e-4, 1e-3, -5.00000000005e-4]),
              ([0, 3, 4], [-1e-3, 1.00000000002e-3, 2.0]), ([0, 4], [np.nan, 1.0])], 5)
    P3 = csr([([0], [1.0]), ([0, 1], [0.5, 0.5]), ([1], [1.0]), ([1], [0.75]), ([0], [-0.5])], 2)
    return [("order", A1, P1, 1e17), ("no_diagonal", A2, P2, 1e-6), ("lumped_to_zero", A3, P3, 1e-3)]


def options(name, **kw):
    o = dict(host.OPTIONS001)
    if name in MAX_LEVEL:
        o["max_level"] = MAX_LEVEL[name]
    o.update(kw)
    return o


def assemble(name, tmpdir=None, which="host", kind="self"):
    """the case's operator, assembled at one rank (which / kind: the library and communicator, as host.Comm takes them)"""
    A = host.Matrix(host.Comm(which, kind))
    if name in WGRIDS:
        A.set_many(*wgrid(*WGRIDS[name]))
    else:
        A.read_file(matrices.path(name, tmpdir))
    return A.assemble()


def hashes(S):
    """sha256 of every array of every level's A, P and R and of the aggregates: what two builds must have in common"""
    import hashlib
    out = {"levels": S.num_levels}
    for l in range(S.num_levels):
        for which in (0, 1, 2) if l < S.num_levels - 1 else (0,):
            d = S.level_layout(l, which)
            for k in ("nnzPerRow_local", "col_local", "val_local"):
                out[f"{l}.{'APR'[which]}.{k}"] = hashlib.sha256(np.ascontiguousarray(d[k]).tobytes()).hexdigest()
        if l < S.num_levels - 1:
            out[f"{l}.agg"] = hashlib.sha256(np.ascontiguousarray(S.level_aggregates(l)[0]).tobytes()).hexdigest()
    return out


def solver(name, tmpdir=None, which="host", kind="self", **kw):
    """-> (A, AmgSolver) under options(name, **kw)"""
    A = assemble(name, tmpdir, which, kind)
    return A, host.AmgSolver(A, host.options(host.load(which), **options(name, **kw)))
