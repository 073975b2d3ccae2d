"""CPU proof that the inputs and bounds of tests/test_gpu_solver_layer.py are fair: float64 restatements of the coarsest
CG, the Gauss-Jordan inverse and the dot's blocked summation (tests/solver_ref.py), and the oracle's own coarsest CG,
stay inside every bound the GPU module asserts, on every case it uses.  No GPU involved."""
import numpy as np
import pytest

from tests import hierarchy, solver_ref as sr

IDS = lambda c: f"{c[0]}{c[1]}"      # noqa: E731
CG_ALL = sr.CG_CASES + [c for c in sr.FALLBACK_CASES if c not in sr.CG_CASES] + sr.BLOCK_NEW_CASES


@pytest.mark.parametrize("case", sr.ALL_CASES, ids=IDS)
def test_cases_are_well_conditioned_and_the_reference_solves_them(case):
    c = sr.case(*case)
    assert c["cond"] <= 10, c["cond"]
    assert c["resid"] <= 1e-18, c["resid"]
    # the float64 rounding of that solution is what the tests compare with: its own residual is a few u
    assert sr.residual_hp(c["A"], c["x"], c["rhs"]) <= 8 * sr.U * c["cond"] * np.linalg.norm(c["rhs"])


def test_matrix_shapes():
    """the properties the families are chosen for"""
    per_row = lambda A: np.diff(A.indptr)       # noqa: E731
    assert per_row(sr.tri(65)).max() == 3
    B = sr.band17(65, 3)
    assert per_row(B).max() == 17 and abs(B - B.T).max() == 0
    A = sr.arrow(65)
    assert per_row(A)[0] == 65 and set(per_row(A)[1:]) == {2} and abs(A - A.T).max() == 0
    D = sr.dense_spd(200, 1)
    assert per_row(D).min() == 200 and abs(D - D.T).max() == 0
    S = sr.shifted(65, 2).toarray()
    assert np.all(np.abs(np.diag(S, -1)) == 2.5) and np.all(np.abs(np.diag(S)) < 1.0)
    assert np.linalg.matrix_rank(sr.singular(65).toarray()) == 64


@pytest.mark.parametrize("case", CG_ALL, ids=IDS)
def test_cg_restatement_stops_on_the_tolerance(case):
    """150 iterations are never needed: every CG case ends on `dot < thres`, in fewer than 100 iterations, and inside
    both contracts the GPU module holds the kernels to"""
    c = sr.case(*case)
    u, it = sr.coarsest_cg(c["A"], c["rhs"])
    print(f"{case[0]}({case[1]}): {it} iterations")
    assert 1 <= it < 100, it
    assert sr.rel(u, c["x"]) <= 2 * c["cond"] * sr.CG_TOL
    assert sr.residual_hp(c["A"], u, c["rhs"]) <= 2 * sr.CG_TOL * np.linalg.norm(c["rhs"])


@pytest.mark.parametrize("case", sr.CAPPED_CASES, ids=IDS)
def test_cg_restatement_cap(case):
    """CG_coarsest_max_iter = 6 -> five updates, 5 reported; far from converged, so the cap is what ended it"""
    c = sr.case(*case)
    u, it = sr.coarsest_cg(c["A"], c["rhs"], max_iter=6)
    assert it == 5
    assert sr.rel(u, c["x"]) > 1e-6
    O, _ = hierarchy.single_level_oracle(c["A"], cg_max_iter=6)
    u_o, it_o = O.coarsest_cg(c["rhs"])
    assert it_o == 5 and sr.rel(u, u_o) <= 1e-12


@pytest.mark.parametrize("n", [257, 1025])
def test_cg_restatement_early_outs(n):
    """rhs = 0 and ||rhs|| = 1e-13 (dot < tol^2): no iteration, u untouched, the count the oracle reports"""
    c = sr.case("tri", n)
    O, _ = hierarchy.single_level_oracle(c["A"])
    u0 = sr.rhs_for(n) + 2.0
    tiny = c["rhs"] * (1e-13 / np.linalg.norm(c["rhs"]))
    assert float(tiny @ tiny) < sr.CG_TOL ** 2
    for rhs in (np.zeros(n), tiny):
        u, it = sr.coarsest_cg(c["A"], rhs, u0=u0)
        assert np.array_equal(u, u0)
        assert it == O.coarsest_cg(rhs)[1]


@pytest.mark.parametrize("case", CG_ALL, ids=IDS)
def test_oracle_cg_meets_both_contracts(case):
    c = sr.case(*case)
    O, _ = hierarchy.single_level_oracle(c["A"])
    u, it = O.coarsest_cg(c["rhs"])
    assert abs(it - sr.coarsest_cg(c["A"], c["rhs"])[1]) <= 1
    assert sr.rel(u, c["x"]) <= 2 * c["cond"] * sr.CG_TOL
    assert sr.residual_hp(c["A"], u, c["rhs"]) <= 2 * sr.CG_TOL * np.linalg.norm(c["rhs"])


@pytest.mark.parametrize("case", sr.DIRECT_CASES + sr.BLOCK_NEW_CASES, ids=IDS)
def test_gauss_jordan_restatement_meets_the_direct_bound(case):
    """inverse(A) rhs by Gauss-Jordan with partial pivoting stays within 4 (n + 4) u cond_2 of the reference.  This test
    prints err / (n u cond_2) per case: the largest is 0.16, at tri(2); arrow(1024) gives 0.066, the other 1023- and
    1024-row cases less than 0.001, and tri(1) is exact."""
    f, n = case
    c = sr.case(f, n)
    inv, swaps = sr.inverse(f, n)
    err = sr.rel(inv @ c["rhs"], c["x"])
    print(f"{f}({n}): err / (n u cond) = {err / (n * sr.U * c['cond']):.3g}, {swaps} row swaps")
    assert err <= sr.direct_bound(n, c["cond"])
    if f == "shifted":
        assert swaps >= n - 2           # this family is where the pivot search and the swap are exercised
    else:
        assert swaps == 0


@pytest.mark.parametrize("n", sr.FAMILY_SIZES)
def test_shifted_is_refused_without_pivoting(n):
    """the family cannot be inverted with the diagonal as the pivot: entry (0, 0) is an exact zero, so an elimination
    without the pivot search stops at column 0 with the refusal meant for singular operators"""
    D = sr.case("shifted", n)["dense"]
    assert D[0, 0] == 0.0 and D[1, 0] == 2.5
    with pytest.raises(sr.Singular):
        sr.gauss_jordan_inverse(D, pivot=False)


def test_singular_is_refused():
    with pytest.raises(sr.Singular):
        sr.gauss_jordan_inverse(sr.singular(65).toarray())


def test_dot_roundings_formula():
    assert sr.dot_roundings(1) == 1 + 1 + 6 + 4 + 1 + 6 + 4 + 1 == 24
    assert sr.dot_roundings(262144) == 1 + 1 + 6 + 4 + 4 + 6 + 4 + 1
    assert sr.dot_roundings(262145) == 2 + 1 + 6 + 4 + 4 + 6 + 4 + 1
    assert sr.dot_roundings(2097155) == 9 + 1 + 6 + 4 + 4 + 6 + 4 + 1
    assert min(sr.dot_roundings(n) for n in sr.vec_sizes()) >= 23


@pytest.mark.parametrize("n", [n for n in sr.vec_sizes() if n > 0])
def test_blocked_dot_stays_within_its_roundings(n):
    """the summation order of k_dot_partial + k_reduce_partials, in float64 numpy, against the longdouble sum.  This
    test prints the error in roundings per size and kind: the largest is 0.88 (n = 1, where the one product's own
    rounding is all of it), then 0.87 at 262401 all-positive, where the bound allows 24 and 28"""
    for kind in ("normal", "positive", "cancelling"):
        x, y = sr.dot_inputs(n, kind)
        ref = sr.dot_hp(x, y)
        err = abs(float(np.longdouble(sr.dot_blocked(x, y)) - ref))
        scale = sr.U * float(np.sum(np.abs(x * y)))
        print(f"n={n} {kind}: {err / scale:.2f} roundings of {sr.dot_roundings(n)}")
        assert err <= sr.dot_bound(x, y)
    ones = np.ones(n)
    assert sr.dot_blocked(ones, ones) == n
    assert sr.dot_blocked(np.ones(0), np.ones(0)) == 0.0


@pytest.mark.parametrize("n", sr.KRYLOV_SIZES)
def test_oracle_cg_past_the_dot_grid_is_a_fair_reference(n):
    """tri(n), the Krylov cases of the GPU module: the oracle's solve_CG converges well inside 100 iterations, and
    the residual of its u, recomputed in longdouble, is the last entry of its history to 1e-10 of the first"""
    A, rhs = sr.tri(n), sr.rhs_for(n)
    O, _ = hierarchy.single_level_oracle(A, max_iter=100, tol=1e-8)
    u, it, hist = O.solve_CG(rhs)
    print(f"{it} iterations, {hist[0]:.6e} -> {hist[-1]:.6e}")
    assert 10 < it < 100 and len(hist) == it + 1 and hist[-1] < 1e-8 * hist[0]
    assert abs(sr.residual_hp(A, u, rhs) - hist[-1]) <= 1e-10 * hist[0]


# ---------------------------------------------------------------------------
# the block path: tests/test_gpu_block_solver_layer.py
def test_block_case_lists():
    """the sizes of the multi-pass direct solve are there: 512 rows (8 columns fill the 4096 doubles of LDS), 513 to 1024 (two
    passes of 4 columns at K = 8), 1024 (4 columns fill it); every case is in ALL_CASES, so it is shown well conditioned above"""
    n_direct = {n for _, n in sr.BLOCK_DIRECT_CASES}
    assert {511, 512, 513, 729, 1023, 1024} <= n_direct and max(n_direct) <= sr.CG_MAXN
    assert sr.BLOCK_NEW_CASES == [("tri", 511), ("tri", 512), ("tri", 513), ("tri", 729)]
    assert set(sr.BLOCK_DIRECT_CASES) <= set(sr.ALL_CASES) and set(sr.BLOCK_CG_CASES) <= set(sr.CG_CASES)
    assert ("tri", 1023) in sr.BLOCK_CG_CASES and ("tri", 1024) in sr.BLOCK_CG_CASES and ("arrow", 1024) in sr.BLOCK_CG_CASES
    assert sr.BLOCK_VEC_SIZES == tuple(sorted(set(sr.BLOCK_VEC_SIZES)))
    assert {sr.BLOCK * sr.N_PARTIALS + d for d in (0, 1)} <= set(sr.BLOCK_VEC_SIZES)            # the dot's and the update's wrap
    assert {sr.BLOCK * 2048 + d for d in (0, 1)} <= set(sr.BLOCK_VEC_SIZES)                     # direction, pack, unpack


@pytest.mark.parametrize("case", sr.BLOCK_DIRECT_CASES, ids=IDS)
def test_block_columns_of_the_direct_cases_meet_the_direct_bound(case):
    """the eight scaled and shifted columns of every direct case: inverse(A) b_j by the Gauss-Jordan restatement stays within
    direct_bound of that column's high-precision solution; column 1 is all zero and gives exact zeros.  Largest
    err / (n u cond_2) printed here: 0.12 (tri(9)); the bound allows 4 (n + 4) / n"""
    f, n = case
    c = sr.case(f, n)
    B, X = sr.coarse_columns(f, n, 8)
    assert not B[:, 1].any() and not X[:, 1].any()
    assert len({B[:, j].tobytes() for j in range(8)}) == 8
    inv, _ = sr.inverse(f, n)
    worst = 0.0
    for j in range(8):
        u = inv @ B[:, j]
        err = sr.rel(u, X[:, j])
        worst = max(worst, err / (n * sr.U * c["cond"]))
        assert err <= sr.direct_bound(n, c["cond"]), (j, err)
        if j == 1:
            assert not u.any()
    print(f"{f}({n}): largest err / (n u cond) over the columns = {worst:.3g}")


@pytest.mark.parametrize("case", sr.BLOCK_CG_CASES, ids=IDS)
def test_block_columns_of_the_cg_cases_meet_the_cg_contracts(case):
    """the same columns under the coarsest CG, from zero: fewer than 100 iterations and inside both contracts; from a nonzero guess
    u0 the oracle's CG returns u0 plus that (its residual starts from rhs, not from rhs - A u0), which is what the restatement gives"""
    f, n = case
    c = sr.case(f, n)
    B, X = sr.coarse_columns(f, n, 8)
    for j in range(8):
        u, it = sr.coarsest_cg(c["A"], B[:, j])
        if j == 1:
            assert not u.any()                                   # (no iteration: the early-out)
            continue
        assert 1 <= it < 100, (j, it)
        assert sr.rel(u, X[:, j]) <= 2 * c["cond"] * sr.CG_TOL
        assert sr.residual_hp(c["A"], u, B[:, j]) <= 2 * sr.CG_TOL * np.linalg.norm(B[:, j])
    u0 = sr.rhs_for(n) + 2.0
    u, _ = sr.coarsest_cg(c["A"], B[:, 2], u0=u0)
    uz, _ = sr.coarsest_cg(c["A"], B[:, 2])
    assert sr.rel(u - u0, uz) <= 1e-14
    O, _ = hierarchy.single_level_oracle(c["A"])
    assert sr.rel(O.vcycle(u0, B[:, 2]), u) <= 1e-12                # the one-level oracle's V-cycle is its coarsest CG from u0


def test_tri_two_level():
    A, P, R = sr.tri_two_level(1000, 7)
    assert [a.shape for a in A] == [(1000, 1000), (143, 143)] and P[0].shape == (1000, 143) and R[0].shape == (143, 1000)
    assert abs(A[0] - sr.tri(1000)).max() == 0 and abs(R[0] - P[0].T).max() == 0
    assert np.array_equal(P[0].indices, np.arange(1000) // 7) and np.all(P[0].data == 1.0)
    assert abs(A[1] - R[0] @ A[0] @ P[0]).max() == 0 and A[1].has_sorted_indices and np.diff(A[1].indptr).max() == 3
    assert abs(A[1] - A[1].T).max() == 0
    for (n, agg), nc in zip(sr.TWO_LEVEL, (1022, 1023)):
        assert -(-n // agg) == nc <= sr.CG_MAXN and n > sr.BLOCK * sr.N_PARTIALS
    assert sr.TWO_LEVEL[1][0] > 2 * sr.BLOCK * sr.N_PARTIALS


def test_pcg_restatements():
    """one rounding per operation, a frozen sign of zero included"""
    rng = np.random.default_rng(3)
    p, h, u, r, z = (rng.standard_normal(50) for _ in range(5))
    un, rn = sr.pcg_update(3.0, 7.0, p, h, u, r)
    a = np.float64(3.0) / np.float64(7.0)
    assert np.array_equal(un, u - a * p) and np.array_equal(rn, r - a * h)
    assert np.array_equal(sr.pcg_direction(3.0, 7.0, z, p), z + a * p)
    assert np.signbit(sr.pcg_direction(1.0, 1.0, np.array([-0.0]), np.array([-0.0])))[0]


def two_level_oracle(n, agg, smoother):
    from oracle import oracle as orc
    As, Ps, Rs = sr.tri_two_level(n, agg)
    OA, OP, OR = hierarchy.oracle_hierarchy(As, Ps, Rs)
    for a, e in zip(OA, hierarchy.eig_estimates(As)):
        a.set_eig(e)
    return orc.OracleAmg(OA, OP, OR, pre=2, post=1, smoother=smoother, max_iter=60, tol=1e-8)


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_oracle_pcg_on_the_two_level_hierarchy_is_a_fair_reference(smoother):
    """tri_two_level(262401, 257), the eight block_columns, pre = 2, post = 1, tol 1e-8, max_iter 60: every column converges in
    more than 3 and fewer than 60 iterations, the counts differ between columns (so the block solve freezes columns while others
    run on past the grid-stride wrap), no ||r_k|| lies within 10 % of its column's threshold (a summation-order difference cannot
    flip a count), and the residual of u recomputed in longdouble is the last history entry to 1e-10 of the first.
    Counts seen here: Jacobi 11, 13, 14, 14, 11, 9, 11, 12; Chebyshev 9, 11, 12, 12, 9, 8, 9, 10; 0.15 s per solve."""
    n, agg = sr.TWO_LEVEL[0]
    O = two_level_oracle(n, agg, smoother)
    A = sr.tri(n)
    cols = sr.block_columns(n, 8)
    assert len({c.tobytes() for c in cols}) == 8
    counts = []
    for j, c in enumerate(cols):
        u, it, hist = O.solve_pCG(c)
        counts.append(it)
        assert 3 < it < 60 and len(hist) == it + 1 and hist[-1] < 1e-8 * hist[0], (j, it)
        ratio = hist / (1e-8 * hist[0])
        assert not np.any((ratio > 0.9) & (ratio < 1.1)), (j, ratio)
        if j < 2:
            assert abs(sr.residual_hp(A, u, c) - hist[-1]) <= 1e-10 * hist[0]
    print(smoother, counts)
    assert len(set(counts)) >= 2 and len(set(counts[:2])) == 2      # (the K = 2 solve on the first two columns freezes one as well)
