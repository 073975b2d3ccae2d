"""CPU proof that the inputs and bounds of tests/test_gpu_solver_layer.py are fair: float64 restatements of the coarsest
CG, the Gauss-Jordan inverse and the dot's blocked summation (tests/solver_ref.py), and the oracle's own coarsest CG,
stay inside every bound the GPU module asserts, on every case it uses.  No GPU involved."""
import numpy as np
import pytest

from tests import hierarchy, solver_ref as sr

IDS = lambda c: f"{c[0]}{c[1]}"      # noqa: E731
CG_ALL = sr.CG_CASES + [c for c in sr.FALLBACK_CASES if c not in sr.CG_CASES]


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


@pytest.mark.parametrize("case", sr.DIRECT_CASES, ids=IDS)
def test_gauss_jordan_restatement_meets_the_direct_bound(case):
    """inverse(A) rhs by Gauss-Jordan with partial pivoting stays within 4 (n + 4) u cond_2 of the reference.  This test
    prints err / (n u cond_2) per case: the largest is 0.16, at tri(2); arrow(1024) gives 0.066, the other 1023- and
    1024-row cases less than 0.001, and tri(1) is exact."""
    f, n = case
    c = sr.case(f, n)
    inv, swaps = sr.gauss_jordan_inverse(c["dense"])
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
