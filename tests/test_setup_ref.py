"""tests/setup_ref.py -- the smoothed-aggregation setup restated the plain way -- is anchored before it judges the product
(tests/test_setup_contract.py).  It never judges itself:

  * strength + plain_rounds and smoothed_P against what the compiled reference computed (tests/golden/refsa_*: the coarse
    id of every fine row and P entry by entry, on every level of five hierarchies; the bound on P's values is the one
    tests/test_sa_pins.py holds the product to);
  * smoothed_P, galerkin and filter against the plain loops they are stated as, on three hand-made operators
    (tests/setup_cases.tiny_operators: sums that depend on their order, rows without a diagonal, diagonals that lump to ~0);
  * lanczos_eig in float64 against the same recurrence with its dots and updates in np.longdouble: what the order and the
    rounding of those sums can move the estimate by.  Measured on every level of every input: at most 8.8e-16 relative
    (plat362, level 2), far below the quarter of the contract's 1e-12 that is asserted."""
import glob
import os

import numpy as np
import pytest

from tests import setup_cases, setup_ref, spgemm_ref
from tests.spgemm_ref import Csr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = sorted(os.path.basename(f)[len("refsa_"):-len(".hier.npz")] for f in glob.glob(os.path.join(GOLDEN, "refsa_*.hier.npz")))
EIG_BOUND = 1e-12           # tests/test_setup_contract.py: product against lanczos_eig


def assert_same_csr(got, want, what, values=True):
    np.testing.assert_array_equal(got.ptr, want.ptr, err_msg=f"{what}: row pointers")
    np.testing.assert_array_equal(got.col, want.col, err_msg=f"{what}: columns")
    if values:
        spgemm_ref.assert_same_values(got.val, want.val, what)


def test_every_fixture_hierarchy_is_used():
    assert TAGS == ["plat362", "poisson12", "poisson16", "poisson24", "poisson8"]


@pytest.mark.parametrize("tag", TAGS)
def test_aggregates_and_P_are_the_compiled_reference_s(tag):
    H = np.load(os.path.join(GOLDEN, f"refsa_{tag}.hier.npz"))
    ranks = sorted(glob.glob(os.path.join(GOLDEN, f"refsa_{tag}.np[0-9].npz")))
    assert ranks
    nl = int(H["nlevels"])
    for l in range(nl - 1):
        npr = H[f"A{l}_npr"]
        ptr = np.concatenate([[0], np.cumsum(npr, dtype=np.int64)]).astype(np.int64)
        A = Csr(ptr, H[f"A{l}_col"].astype(np.int32), H[f"A{l}_val"].astype(np.float64), len(npr), len(npr))
        agg, nagg = setup_ref.plain_rounds(A, setup_ref.strength(A, 0.2))
        P = setup_ref.smoothed_P(A, agg, nagg)
        for f in ranks:
            G = np.load(f)
            what = f"{os.path.basename(f)} level {l}"
            assert nagg == int(G[f"Pshape{l}"][1]), what
            np.testing.assert_array_equal(agg, G[f"agg{l}"], err_msg=f"{what}: aggregates")
            np.testing.assert_array_equal(setup_ref.rows_of(P), G[f"Prow{l}"], err_msg=f"{what}: P's rows")
            np.testing.assert_array_equal(P.col, G[f"Pcol{l}"], err_msg=f"{what}: P's columns")
            ref_v = G[f"Pval{l}"]
            scale = np.repeat(np.maximum.reduceat(np.abs(ref_v), P.ptr[:-1]), np.diff(P.ptr))      # every row of P has an entry
            diff = np.abs(P.val - ref_v)
            assert np.all(diff <= 1e-14 * scale), f"{what}: max diff / row scale {np.max(diff / scale)}"
            assert np.mean(diff == 0) >= 0.5, f"{what}: only {np.mean(diff == 0):.2%} of P's values are bit-identical"


TINY = setup_cases.tiny_operators()


@pytest.mark.parametrize("name,A,P,thre", TINY, ids=[t[0] for t in TINY])
def test_the_vectorised_restatement_is_the_plain_loop(name, A, P, thre):
    R = setup_ref.transpose(P)
    # transpose, by hand: entry (i, j) of P is entry (j, i) of R, R's rows ascend
    dense = np.zeros((P.nrows, P.ncols)); dense[setup_ref.rows_of(P), P.col] = P.val
    back = np.zeros((P.ncols, P.nrows)); back[setup_ref.rows_of(R), R.col] = R.val
    np.testing.assert_array_equal(back, dense.T)
    assert all(np.all(np.diff(R.col[R.ptr[i]:R.ptr[i + 1]]) > 0) for i in range(R.nrows))
    assert_same_csr(setup_ref.galerkin(R, A, P), setup_ref.galerkin_loop(R, A, P), f"{name}: R A P")
    for t in (thre, 1e-8, 0.0):
        for block, ofs in ((A, 0), (Csr(A.ptr[2:] - A.ptr[2], A.col[A.ptr[2]:], A.val[A.ptr[2]:], A.nrows - 2, A.ncols), 2)):
            assert_same_csr(setup_ref.filter(block, t, ofs), setup_ref.filter_loop(block, t, ofs), f"{name}: filter at {t}, rows from {ofs}")


def test_the_filter_s_rules_on_the_hand_made_rows():
    """what the three operators are there for, stated as numbers (so that two restatements wrong in the same way fail)"""
    (_, A1, _, t1), (_, A2, _, t2), (_, A3, _, t3) = TINY
    F = setup_ref.filter(A1, t1)
    np.testing.assert_array_equal(F.col, np.arange(6))                       # everything is lumped
    assert F.val[0] == 4.0 and F.val[1] == 1.0 + 2.0 ** -52                   # (1e16 + 1) - 1e16 = 0; u + u added ONCE
    F = setup_ref.filter(A2, t2)
    np.testing.assert_array_equal(np.diff(F.ptr), [2, 2, 3, 2, 3, 1])
    rows = [list(zip(F.col[F.ptr[i]:F.ptr[i + 1]].tolist(), F.val[F.ptr[i]:F.ptr[i + 1]].tolist())) for i in range(6)]
    assert rows[0] == [(0, 1.0), (1, -1.0)] and rows[2] == [(1, -3.0), (2, 1.0), (4, 4.0)] and rows[4] == [(0, 0.25), (2, -0.5), (4, 1.0)]
    assert rows[5] == [(5, 1.0)] and rows[1] == [(0, -1.0), (1, 2.0)]
    F = setup_ref.filter(A3, t3)
    d = setup_ref.diagonal(F)
    assert d[0] == 1.0 and d[1] == 1.0 and d[2] == 1.0 and 1e-14 < d[3] < 3e-14 and np.isnan(d[4])
    np.testing.assert_array_equal(np.diff(F.ptr), [1, 1, 1, 2, 1])


def test_smoothed_P_is_its_plain_loop():
    _, A1, _, _ = TINY[0]
    agg = np.array([0, 0, 1, 1, 2, 2], np.int32)
    assert_same_csr(setup_ref.smoothed_P(A1, agg, 3), setup_ref.smoothed_P_loop(A1, agg, 3), "smoothed P")
    # a poisson-like row, by hand: row (-1, 2, -1) around a diagonal of 2, columns in aggregates (0, 0, 1)
    A = spgemm_ref.csr([([0, 1], [2.0, -1.0]), ([0, 1, 2], [-1.0, 2.0, -1.0]), ([1, 2], [-1.0, 2.0])], 3)
    P = setup_ref.smoothed_P(A, np.array([0, 0, 1], np.int32), 2)
    w = setup_ref.OMEGA
    assert w == float(np.float32(2.0 / 3.0)) and w != 2.0 / 3.0
    np.testing.assert_array_equal(P.ptr, [0, 1, 3, 5])
    np.testing.assert_array_equal(P.col, [0, 0, 1, 0, 1])
    s = -w * 0.5
    d, o = s * 2.0 + 1.0, s * -1.0                                          # the diagonal's term (+ 1 AFTER the product), a neighbour's
    spgemm_ref.assert_same_values(P.val, [d + o, o + d, o, o, d], "P of the 1-D row")


@pytest.fixture(scope="module")
def operators(tmp_path_factory):
    """every level of every input's hierarchy (built by the product: here they are inputs, nothing more)"""
    tmp = tmp_path_factory.mktemp("mtx")
    out = {}
    for name in setup_cases.NAMES:
        _, S = setup_cases.solver(name, tmp)
        out[name] = [setup_ref.from_layout(S.level_layout(l, 0)) for l in range(S.num_levels)]
    return out


@pytest.mark.parametrize("name", setup_cases.NAMES)
def test_lanczos_in_float64_against_long_double(name, operators):
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is no wider than float64 here"
    for l, A in enumerate(operators[name]):
        e64, eld = setup_ref.lanczos_eig(A), setup_ref.lanczos_eig(A, np.longdouble)
        rel = abs(e64 - eld) / abs(eld)
        print(f"{name} level {l} ({A.nrows} rows): float64 {e64!r}, long double {eld!r}, relative difference {rel:.2e}")
        assert rel < EIG_BOUND / 4, (name, l, rel)


def test_lanczos_on_a_matrix_whose_spectrum_is_known():
    """diagonal scaling D^-1/2 A D^-1/2 and the factor: A = diag(d) has D^-1 A = I, so the estimate is 1.0001 after one step
    (beta = 0 ends the recurrence); the 1-D Laplacian's 20-step Ritz value lies below lambda_max = 1 + cos(pi / (n + 1))"""
    n = 50
    A = spgemm_ref.csr([([i], [3.0 + i]) for i in range(n)], n)
    assert abs(setup_ref.lanczos_eig(A) - 1.0001) <= 1e-14           # sqrt(1/d) d sqrt(1/d) is 1 to a handful of roundings (2.2e-16 each)
    T = spgemm_ref.csr([([j for j in (i - 1, i, i + 1) if 0 <= j < n], [(-1.0 if j != i else 2.0) for j in (i - 1, i, i + 1) if 0 <= j < n]) for i in range(n)], n)
    lam = 1.0 + np.cos(np.pi / (n + 1))
    e = setup_ref.lanczos_eig(T, factor=1.0)
    assert 0.9 * lam < e <= lam * (1 + 1e-14)
    assert setup_ref.lanczos_eig(T) == 1.0001 * e
    # a matrix of at most 20 rows: the Krylov space is the whole space, the Ritz value is lambda_max itself
    n = 12
    T = spgemm_ref.csr([([j for j in (i - 1, i, i + 1) if 0 <= j < n], [(-1.0 if j != i else 2.0) for j in (i - 1, i, i + 1) if 0 <= j < n]) for i in range(n)], n)
    assert abs(setup_ref.lanczos_eig(T, factor=1.0) - (1.0 + np.cos(np.pi / (n + 1)))) <= 1e-13
