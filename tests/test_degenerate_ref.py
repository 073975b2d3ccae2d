"""CPU companion of tests/test_gpu_degenerate_rhs.py: the numpy statement of include/saena_gpu.h's "Degenerate right-hand sides"
(tests/degenerate_ref.py, and the rules as tests/null_space_ref.pcg / stationary carry them) on the inputs the GPU test uses, so that
the GPU test is known to reach every branch and to ask what a correct implementation delivers.  No GPU."""
import numpy as np
import pytest

from tests import degenerate_ref as dg, null_space_ref as ns, solver_ref as sr

EXACT = (("neumann8", 1.0), ("neumann8", 0.1))            # the centred vector of c 1 is exactly zero
DUST = (("neumann12x8x5", np.pi),)                        # it is d 1, d != 0
PERTURBED = (("neumann8", 0.1), ("neumann12x8x5", np.pi))


def rows(name):
    return ns.hierarchy(name)["A"][0].shape[0]


def test_the_constants_reach_both_branches():
    """(512, 1.0) and (512, 0.1) centre to exactly zero -- rule 1 as it stands; (480, pi) and (1331, 0.1) centre to a constant d 1
    with d != 0 -- only rule 2 catches them"""
    for name, c in EXACT:
        y, m = ns.center(dg.constant(rows(name), c))
        assert not np.any(y) and m == c
    for n, c in [(rows(name), c) for name, c in DUST] + [(1331, 0.1)]:
        y, m = ns.center(dg.constant(n, c))
        print(f"n = {n}, c = {c!r}: d / c = {y[0] / c:.3e} ({y[0] / (np.spacing(c)):.1f} ulp of c)")
        assert y[0] != 0.0 and np.all(y == y[0])
        assert dg.at_start(float(y @ y), n, m, null_space=True) == "zero"
        assert dg.at_start(float(y @ y), n, m, null_space=False) is None


@pytest.mark.parametrize("n", ns.CENTER_SIZES[:-3] + (480, 1331, 4096))
def test_the_criterion_bounds_every_constant(n):
    """the derivation, against the restatement of the kernels: for constants of every size and sign the centred norm stays below
    n (k u |m|)^2 -- and the bound is not loose by more than the count of roundings squared"""
    worst = 0.0
    for c in (1.0, 0.1, -0.1, np.pi, 1.0 / 3.0, -1e-300, 1e300, 2.0 ** -40, 0.7):
        y, m = ns.center(dg.constant(n, c))
        with np.errstate(over="ignore", under="ignore"):
            dot = float(sr.dot_blocked(y, y))
        if abs(c) < 1e-150 or abs(c) > 1e150:          # the squares leave the range of float64: the comparison itself is what is tested
            assert dg.at_start(dot, n, m, null_space=True) in ("zero", "nonfinite")
            continue
        assert dot <= dg.criterion(n, m), (n, c, dot, dg.criterion(n, m))
        worst = max(worst, dot / dg.criterion(n, m))
    print(f"n = {n}: the largest ||y||^2 / criterion over the constants is {worst:.3f}")


@pytest.mark.parametrize("name,c", PERTURBED)
def test_the_other_side_of_the_criterion_is_solved(name, c):
    """rhs = c + a |c| v, a = 1e-3: the criterion sits at least 1e6 below its centred norm, and the restatement solves it to the four
    checks of check_solution against solve_plus"""
    H = ns.hierarchy(name)
    n = rows(name)
    rhs = dg.perturbed(n, c)
    y, m = ns.center(rhs)
    norm, crit = float(np.linalg.norm(y)), float(np.sqrt(dg.criterion(n, m)))
    print(f"{name}, c = {c!r}: centred norm {norm:.3e}, criterion {crit:.3e}, ratio {norm / crit:.2e}")
    assert norm >= 1e6 * crit
    for what, want in (("pcg", ns.pcg(H, rhs)), ("stationary", ns.stationary(H, rhs))):
        assert want["stopped"] is None
        dg.four_checks(H, want["u"], want["hist"], want["converged"], rhs, want, f"{name} {what} restatement at a = {dg.A_PERTURB}")


def test_the_restatements_carry_the_rules():
    H = ns.hierarchy("neumann8")
    n = rows("neumann8")
    for solve in (ns.pcg, lambda H, b: ns.pcg(H, b, precond=False), ns.stationary, lambda H, b: ns.stationary(H, b, with_coarse=False)):
        for rhs in (np.zeros(n), -np.zeros(n), dg.constant(n, 0.1), dg.constant(n, 1.0)):
            w = solve(H, rhs)
            assert w["stopped"] == "zero" and w["converged"] and w["iters"] == 0 and not np.any(w["u"]) and np.array_equal(w["hist"], [0.0])
        for bad in (np.nan, -np.inf):
            rhs = ns.rhs_for(n)
            rhs[n // 3] = bad
            with np.errstate(invalid="ignore"):
                w = solve(H, rhs)
            assert w["stopped"] == "nonfinite" and not w["converged"] and w["iters"] == 0 and len(w["hist"]) == 1 and not np.isfinite(w["hist"][0])
            assert not np.any(w["u"])
    H2 = ns.hierarchy("neumann12x8x5")
    w = ns.pcg(H2, dg.constant(480, np.pi))
    assert w["stopped"] == "zero" and w["iters"] == 0 and np.array_equal(w["hist"], [0.0])


def test_breakdown_on_the_indefinite_diagonal():
    """diag(+1 x 32, -1 x 32), rhs = 1: ||r_0|| = 8, the first p . A p is exactly 0, the first update's dot is not finite: iters = 1"""
    A = dg.indefinite_diag()
    r = -np.ones(64)
    assert float(r @ (A @ r)) == 0.0
    w = dg.cg(A, np.ones(64))
    assert w["stopped"] == "nonfinite" and w["iters"] == 1 and not w["converged"]
    assert w["hist"][0] == 8.0 and not np.isfinite(w["hist"][1])


def test_kind_zero_rules():
    A = sr.tri(65)
    for rhs in (np.zeros(65), -np.zeros(65)):
        w = dg.cg(A, rhs)
        assert w["stopped"] == "zero" and w["converged"] and w["iters"] == 0 and np.array_equal(w["hist"], [0.0]) and not np.any(w["u"])
    w = dg.cg(A, sr.rhs_for(65))
    assert w["converged"] and w["stopped"] is None and np.all(np.isfinite(w["hist"]))
    assert dg.at_start(1e-300) is None and dg.at_start(float("inf")) == "nonfinite" and dg.at_start(float("nan")) == "nonfinite"
