"""The host's smoothed-aggregation setup (saena_amd/csrc/host/amg_setup.cpp: strength graph, aggregation, smoothed P,
R = P^T, Galerkin product, filter, level-stop rule, eigenvalue estimate) against its restatement (tests/setup_ref.py, anchored
by tests/test_setup_ref.py) on irregular operators (tests/setup_cases.py).

The contract: for every input and every level the aggregates and their count, the pattern of P, R and A_(l+1) and the number
of levels are the restatement's exactly, and every VALUE of P, R and A_(l+1) is the restatement's bit for bit -- each sum is
restated in the product's order (P's duplicates in stored order, the products of tests/spgemm_ref.py's contract, the
filter's lump in row order, added to the diagonal once).  The eigenvalue estimate of the Chebyshev smoother is
lanczos_eig's within 1e-12 relative (the bound tests/test_amg_setup.py holds the distributed estimate to, for the same
cause: the order of the sums in the Lanczos dots; the restatement in long double moves it by 8.8e-16 at most).

What each input costs the restatement is in tests/setup_cases.py: SiH4 is cut at one coarsening step (max_level = 1), and
of wgrid36's second step the Galerkin product is restated on four blocks of coarse rows, a sixteenth of them in all.
Measured: estimate / lambda_max(D^-1 A) = 0.9948 on level 0 of wgrid16 (4 095 rows) and 1.0001 on its levels 1-4 and on every
level of plat362 and fxm3_6: twenty Lanczos steps UNDER-estimate on a large level, the factor 1.0001 does not make the
estimate an upper bound.  The product's estimate differs from the restated one by 4.5e-15 relative at most."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from saena_amd import host
from tests import setup_cases, setup_ref, spgemm_ref
from tests.spgemm_ref import Csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG_BOUND = 1e-12


def assert_same_csr(got, want, what):
    assert (got.nrows, got.ncols) == (want.nrows, want.ncols), what
    np.testing.assert_array_equal(got.ptr, want.ptr, err_msg=f"{what}: row pointers")
    np.testing.assert_array_equal(got.col, want.col, err_msg=f"{what}: columns")
    spgemm_ref.assert_same_values(got.val, want.val, what)


def assert_level_equals(S, l, want, what):
    """level l of the product against a setup_ref.Level"""
    assert_same_csr(setup_ref.from_layout(S.level_layout(l, 0)), want.A, f"{what} A{l}")
    if want.P is None:
        return
    agg, nagg = S.level_aggregates(l)
    assert nagg == want.nagg, f"{what} level {l}: {nagg} aggregates, the restatement has {want.nagg}"
    np.testing.assert_array_equal(agg, want.agg, err_msg=f"{what} level {l}: aggregates")
    assert_same_csr(setup_ref.from_layout(S.level_layout(l, 1)), want.P, f"{what} P{l}")
    assert_same_csr(setup_ref.from_layout(S.level_layout(l, 2)), want.R, f"{what} R{l}")


def assert_hierarchy_equals(S, levels, what):
    assert S.num_levels == len(levels), f"{what}: {S.num_levels} levels, the restatement has {len(levels)}"
    for l, want in enumerate(levels):
        assert_level_equals(S, l, want, what)


@pytest.fixture(scope="module")
def tmpdir_mtx(tmp_path_factory):
    return tmp_path_factory.mktemp("mtx")


@pytest.fixture(scope="module")
def built(tmpdir_mtx):
    """name (+ option overrides) -> (A, AmgSolver), built once; Chebyshev, so that every level has its eigenvalue estimate"""
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = setup_cases.solver(name, tmpdir_mtx, smoother="chebyshev", **kw)
        return cache[key]
    return get


def restate(S, name, **kw):
    return setup_ref.hierarchy(setup_ref.from_layout(S.level_layout(0, 0)), setup_cases.options(name, **kw), max_products=setup_cases.MAX_PRODUCTS)


# ---- the whole hierarchy, every input -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wgrid16", "fxm3_6", "SiH4", "plat362"])
def test_the_hierarchy_is_the_restatement_s(name, built):
    _, S = built(name)
    levels = restate(S, name)
    print(name, [(lv.A.nrows, len(lv.A.col), lv.dropped) for lv in levels])
    assert_hierarchy_equals(S, levels, name)
    assert len(levels) >= 2
    if name == "fxm3_6":        # what the input is there for: the row maximum of -a_ik is negative in every row
        A = levels[0].A
        off = setup_ref.rows_of(A) != A.col
        assert np.all(A.val[off] > 0) and np.all(setup_ref.strength(A, 0.2))
    if name == "wgrid16":       # ... the filter rewrites levels; ... rows long enough for the second path of the sort in P's rows
        assert sum(lv.dropped for lv in levels) > 0 and len(levels) == 5
    if name in ("wgrid16", "SiH4"):
        assert max(np.diff(lv.A.ptr).max() for lv in levels[:-1]) > 16


def test_wgrid36_is_the_restatement_s(built):
    """level 0 is above the 32 768 rows from which the aggregation deals a round to threads.  Step 0 whole; of step 1 the
    aggregates, P and R whole and the Galerkin product (1.1e8 products) on four blocks of coarse rows"""
    name = "wgrid36"
    _, S = built(name)
    assert S.num_levels == 3 and S.level_info(0)["rows"] > 32768
    first = restate(S, name, max_level=1)
    assert len(first) == 2
    assert_level_equals(S, 0, first[0], name)
    A1 = setup_ref.from_layout(S.level_layout(1, 0))
    assert_same_csr(A1, first[1].A, f"{name} A1")
    opts = setup_cases.options(name)
    agg, nagg = setup_ref.plain_rounds(A1, setup_ref.strength(A1, opts["connStrength"]))
    P = setup_ref.smoothed_P(A1, agg, nagg)
    R = setup_ref.transpose(P)
    assert_level_equals(S, 1, setup_ref.Level(A1, agg, nagg, P, R, first[1].dropped), name)
    thre = setup_ref.filter_thresholds(opts, 2)[1]
    A2 = setup_ref.from_layout(S.level_layout(2, 0))
    assert A2.nrows == nagg
    width = nagg // 64
    for lo in (0, nagg // 3, (2 * nagg) // 3, nagg - width):
        hi = lo + width
        Rb = Csr(R.ptr[lo:hi + 1] - R.ptr[lo], R.col[R.ptr[lo]:R.ptr[hi]], R.val[R.ptr[lo]:R.ptr[hi]], width, R.ncols)
        RA = setup_ref.product(Rb, A1, row_offset=lo)
        assert setup_ref.n_products(Rb, A1) + setup_ref.n_products(RA, P) <= 2 * 10 ** 7
        want = setup_ref.filter(setup_ref.product(RA, P, row_offset=lo), thre, row_offset=lo)
        got = Csr(A2.ptr[lo:hi + 1] - A2.ptr[lo], A2.col[A2.ptr[lo]:A2.ptr[hi]], A2.val[A2.ptr[lo]:A2.ptr[hi]], width, A2.ncols)
        assert_same_csr(got, want, f"{name} A2, rows {lo}..{hi}")


def test_strength_at_the_threshold():
    """-a_ij / max is EQUAL to the threshold (the float32 option as a double: 0.20000000298...): not strong.  Triangles
    (3g, 3g + 1, 3g + 2) with two edges of weight s and the edge 3g -- 3g + 2 of weight s c (s = 1, then 4: the quotient is
    exact): on the threshold that edge is not strong, row 3g + 2 waits for 3g + 1, sees it join 3g and becomes a root of
    its own; one ulp above it the edge is strong and 3g + 2 joins 3g."""
    c = float(np.float32(0.2))
    groups = 8
    n = 3 * groups
    g = 3 * np.arange(groups)
    s = np.where(np.arange(groups) < 4, 1.0, 4.0)
    for bump, on_threshold in ((0, True), (1, False)):
        third = s * c
        assert np.all(third / s == c)
        if bump:
            third = np.nextafter(third, np.inf)
        a, b, ww = np.concatenate([g, g + 1, g]), np.concatenate([g + 1, g + 2, g + 2]), np.concatenate([s, s, third])
        rows, cols, vals = np.concatenate([a, b, np.arange(n)]), np.concatenate([b, a, np.arange(n)]), np.concatenate([-ww, -ww, np.full(n, 10.0)])
        A = host.Matrix(host.Comm("host", "self"))
        A.set_many(rows, cols, vals)
        A.assemble()
        S = host.AmgSolver(A, host.options(host.load("host"), **dict(host.OPTIONS001, max_level=1, dynamic_levels=0)))
        Ar = setup_ref.from_layout(S.level_layout(0, 0))
        strong = setup_ref.strength(Ar, 0.2)
        off = setup_ref.rows_of(Ar) != Ar.col
        assert int(strong[off].sum()) == (4 * groups if on_threshold else 6 * groups)
        agg, nagg = S.level_aggregates(0)
        want, nwant = setup_ref.plain_rounds(Ar, strong)
        np.testing.assert_array_equal(want, np.repeat(np.arange(2 * groups), [2, 1] * groups) if on_threshold else np.arange(n) // 3)
        assert nagg == nwant
        np.testing.assert_array_equal(agg, want)


# ---- filter options -------------------------------------------------------------------------------------------------
def test_a_coarse_filter_capped_at_filter_max(built):
    """filter_thre = 1e-3, filter_max = 1e-1, rate 2: the thresholds are 1e-3, then 1e-1 for good (uncapped: 10, 1000 ...)"""
    kw = dict(filter_thre=1e-3, filter_max=1e-1)
    _, S = built("wgrid16", **kw)
    levels = restate(S, "wgrid16", **kw)
    print([(lv.A.nrows, len(lv.A.col), lv.dropped) for lv in levels])
    assert setup_ref.filter_thresholds(setup_cases.options("wgrid16", **kw), 3) == [1e-3, 1e-1, 1e-1]
    assert len(levels) >= 4, "the cap is reached at the third step only"
    assert all(lv.dropped > 0 for lv in levels[1:4]), "the filter's rewriting path must have run"
    assert_hierarchy_equals(S, levels, "wgrid16, coarse filter")


def test_the_filter_switched_off(built):
    kw = dict(filter_start=100)
    _, S = built("wgrid16", **kw)
    levels = restate(S, "wgrid16", **kw)
    assert all(lv.dropped == 0 for lv in levels)
    assert_hierarchy_equals(S, levels, "wgrid16, no filter")
    _, S0 = built("wgrid16")
    assert S.level_info(2)["nnzA"] > S0.level_info(2)["nnzA"], "the default filter drops entries of level 2: this run must not"


# ---- thread count ---------------------------------------------------------------------------------------------------
WORKER = r"""
import sys, json
sys.path.insert(0, %(root)r)
from tests import setup_cases
A, S = setup_cases.solver("wgrid36", smoother="chebyshev")
out = setup_cases.hashes(S)
out["rows"] = [S.level_info(l)["rows"] for l in range(S.num_levels)]
out["eig"] = [S.level_info(l)["eig_max"] for l in range(S.num_levels)]
print("RESULT " + json.dumps(out))
"""


def _child(threads, timing):
    env = dict(os.environ, SAENA_SETUP_THREADS=str(threads))
    env.pop("SAENA_SETUP_TIMING", None)
    if timing:
        env["SAENA_SETUP_TIMING"] = "1"
    return subprocess.Popen([sys.executable, "-c", WORKER % dict(root=ROOT)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)


def test_one_thread_and_sixteen_build_the_same_hierarchy(built):
    """SAENA_SETUP_THREADS is read once per process: two fresh children.  Every array of every level is byte-identical
    between them (and with this process's build, whatever its thread count), and the aggregates of levels 0 and 1 -- the
    first rounds of level 0 dealt to 16 threads, waiting rows pushed onto their blockers' chains concurrently -- are the
    plain rounds'."""
    procs = [_child(1, False), _child(16, True)]
    res = []
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, out[-2000:] + err[-3000:]
        res.append((json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:]), err))
    (one, _), (sixteen, err16) = res
    assert one == sixteen, {k: (one.get(k), sixteen.get(k)) for k in set(one) | set(sixteen) if one.get(k) != sixteen.get(k)}
    first = re.search(r"\[aggregate\] (\d+) rounds, (\d+) row visits for (\d+) rows", err16)
    assert first and int(first.group(3)) > 32768 and int(first.group(3)) == one["rows"][0], err16[-2000:]
    _, S = built("wgrid36")
    here = setup_cases.hashes(S)
    assert {k: v for k, v in one.items() if k not in ("rows", "eig")} == here
    opts = setup_cases.options("wgrid36")
    for l in (0, 1):
        A = setup_ref.from_layout(S.level_layout(l, 0))
        want, nwant = setup_ref.plain_rounds(A, setup_ref.strength(A, opts["connStrength"]))
        agg, nagg = S.level_aggregates(l)
        assert nagg == nwant
        np.testing.assert_array_equal(agg, want, err_msg=f"level {l}")


# ---- eigenvalue estimate --------------------------------------------------------------------------------------------
def lambda_max(A):
    """largest eigenvalue of the symmetrised D^-1/2 A D^-1/2"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    isd = np.sqrt(np.abs(1.0 / setup_ref.diagonal(A)))
    M = sp.csr_matrix((A.val * isd[setup_ref.rows_of(A)] * isd[A.col], A.col, A.ptr), shape=(A.nrows, A.nrows))
    M = (M + M.T) * 0.5
    if A.nrows <= 1000:
        return float(np.linalg.eigvalsh(M.toarray())[-1])
    return float(spl.eigsh(M, k=1, which="LA", tol=1e-12, return_eigenvectors=False)[0])


@pytest.mark.parametrize("name", ["wgrid16", "plat362", "fxm3_6"])
def test_the_eigenvalue_estimate(name, built):
    _, S = built(name)
    assert name in setup_cases.SYMMETRIC
    for l in range(S.num_levels):
        A = setup_ref.from_layout(S.level_layout(l, 0))
        got, want = S.level_info(l)["eig_max"], setup_ref.lanczos_eig(A)
        lam = lambda_max(A)
        print(f"{name} level {l} ({A.nrows} rows): estimate {got!r}, restated {want!r} (relative difference {abs(got - want) / want:.2e}), "
              f"lambda_max {lam!r}, estimate / lambda_max {got / lam:.4f}")
        assert abs(got - want) <= EIG_BOUND * want, (name, l, got, want)
        assert got <= 1.0001 * lam * (1 + 1e-10), (name, l, got, lam)       # a Ritz value cannot exceed lambda_max
        assert got > 0.5 * lam


# ---- the filter itself, where the setup cannot lead it --------------------------------------------------------------
def _rows(C, lo, hi):
    return Csr(C.ptr[lo:hi + 1] - C.ptr[lo], C.col[C.ptr[lo]:C.ptr[hi]], C.val[C.ptr[lo]:C.ptr[hi]], hi - lo, C.ncols)


def _filtered(C, thre, row_offset=0):
    p, c, v = host.filter_csr(host.load("host"), C.ptr, C.col, C.val, thre, row_offset)
    return Csr(p, c, v, C.nrows, C.ncols)


TINY = setup_cases.tiny_operators()


@pytest.mark.parametrize("name,A,P,thre", TINY, ids=[t[0] for t in TINY])
def test_filter_on_the_hand_made_operators(name, A, P, thre):
    for t in (thre, 1e-8, 0.0):
        assert_same_csr(_filtered(A, t), setup_ref.filter(A, t), f"{name} at {t}")
        assert_same_csr(_filtered(_rows(A, 2, A.nrows), t, 2), setup_ref.filter(_rows(A, 2, A.nrows), t, 2), f"{name} at {t}, rows from 2")


def test_filter_on_rows_without_a_diagonal(built):
    """a row without a diagonal entry does not come out of an assembled operator's Galerkin product: wgrid16's unfiltered
    level 2 with the diagonal entries taken out of every third row, whole and as a block of rows with a row offset"""
    _, S = built("wgrid16", filter_start=100)
    C = setup_ref.from_layout(S.level_layout(2, 0))
    r = setup_ref.rows_of(C)
    gone = (r == C.col) & (r % 3 == 0)
    ptr = np.zeros(C.nrows + 1, np.int64)
    np.add.at(ptr, r[~gone] + 1, 1)
    D = Csr(np.cumsum(ptr), C.col[~gone], C.val[~gone], C.nrows, C.ncols)
    assert int(gone.sum()) == (C.nrows + 2) // 3
    for thre in (1e-12, 1e-6, 1e-2):
        want = setup_ref.filter(D, thre)
        assert len(want.col) < len(D.col) + int(gone.sum()), "the threshold drops nothing"
        assert_same_csr(_filtered(D, thre), want, f"level 2 at {thre}")
        assert_same_csr(_filtered(C, thre), setup_ref.filter(C, thre), f"level 2 with its diagonals at {thre}")
        lo, hi = C.nrows // 4 + 1, (3 * C.nrows) // 4
        assert_same_csr(_filtered(_rows(D, lo, hi), thre, lo), setup_ref.filter(_rows(D, lo, hi), thre, lo), f"rows {lo}..{hi} at {thre}")
        np.testing.assert_array_equal(_filtered(_rows(D, lo, hi), thre, lo).val, want.val[want.ptr[lo]:want.ptr[hi]])
    with pytest.raises(host.SgpuError, match="ascending"):
        host.filter_csr(host.load("host"), [0, 2], [1, 0], [1.0, 2.0], 0.0)
