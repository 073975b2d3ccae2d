"""tests/gmres_ref.py checked on the CPU: the numpy FGMRES against scipy's GMRES, the iteration counts of the four convdiff cases,
the restated summation order of the Gram-Schmidt dots against its own error bound, and the proof that a correct implementation
stays inside the history bound tests/test_gpu_gmres.py asserts (the solver run with two other summation orders of its dots)."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from tests import gmres_ref as gr, solver_ref as sr

# (n, pe) -> (rows per level, inner iterations of FGMRES(30) and FGMRES(5)): properties of the reference, not of the code under test
CASES = {(8, 1.0): ((512, 64), 7), (8, 4.0): ((512, 64), 7), (14, 1.0): ((2744, 343, 64), 8), (14, 4.0): ((2744, 343, 64), 8)}


def precond_of(c):
    return lambda r: gr.vcycle(c["As"], c["Ps"], c["Rs"], r)


def test_convdiff_is_not_symmetric_and_has_the_stated_stencil():
    A = gr.convdiff(4, 4.0)
    assert A.shape == (64, 64) and abs(A - A.T).max() > 0.9
    D = A.toarray()
    i = 1 + 4 * (1 + 4 * 1)                                    # an interior row: x fastest
    assert D[i, i] == 6.0 + 4.0 * 1.75
    assert (D[i, i - 1], D[i, i + 1]) == (-1.0 - 4.0, -1.0)
    assert (D[i, i - 4], D[i, i + 4]) == (-1.0 - 2.0, -1.0)
    assert (D[i, i - 16], D[i, i + 16]) == (-1.0 - 1.0, -1.0)
    b = gr.rhs_for(5)
    assert b[0] == 0.25 and b[3] == np.sin(0.37 * 3) + 0.2 * np.cos(1.3 * 3) + 0.05


@pytest.mark.parametrize("restart", [5, 30])
def test_agrees_with_scipy_without_a_preconditioner(restart):
    """same restart, same tolerance (scipy's is on the estimate, relative to ||b||: the same test, since u_0 = 0): the same number of
    inner iterations and the same solution"""
    c = gr.case(8, 4.0)
    A, b = c["A"], c["rhs"]
    ref = gr.fgmres(A, b, restart, tol=1e-8, max_iter=400)
    assert ref["converged"]
    count = [0]
    x, info = spla.gmres(A, b, rtol=1e-8, atol=0.0, restart=restart, maxiter=400, callback=lambda _: count.__setitem__(0, count[0] + 1), callback_type="pr_norm")
    assert info == 0
    print(f"restart {restart}: {ref['iters']} inner iterations ({ref['restarts']} restarts), scipy {count[0]}; rel-l2 {sr.rel(ref['u'], x):.2e}")
    assert abs(ref["iters"] - count[0]) <= 1
    assert sr.rel(ref["u"], x) <= 1e-7                       # both stop at 1e-8 of ||b||; cond(A) is below 10
    assert sr.residual_hp(A, ref["u"], b) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-6)


@pytest.mark.parametrize("n,pe", sorted(CASES))
def test_iteration_counts_of_the_four_cases(n, pe):
    """FGMRES(30) and FGMRES(5) converge in 7-8 V-cycles where pCG with the same V-cycle stalls; FGMRES(5) restarts once; the Givens
    estimate and the recomputed residual agree to 8 digits at the end"""
    c = gr.case(n, pe)
    rows, its = CASES[(n, pe)]
    assert tuple(a.shape[0] for a in c["As"]) == rows
    M = precond_of(c)
    for restart in (30, 5):
        s = gr.fgmres(c["A"], c["rhs"], restart, precond=M)
        assert s["converged"] and s["iters"] == its, (restart, s["iters"])
        assert s["restarts"] == (1 if restart == 5 else 0)
        assert abs(s["hist"][-1] - s["true_res"]) <= 1e-8 * s["true_res"]
        assert sr.residual_hp(c["A"], s["u"], c["rhs"]) <= 1e-8 * s["hist"][0] * (1 + 1e-6)
        assert gr.monotone_within_cycles(s["hist"], restart)
    it, conv, best = gr.pcg(c["A"], c["rhs"], M, max_iter=100)
    assert not conv and best > 1e-8, (it, best)


@pytest.mark.parametrize("n", sr.vec_sizes() + (gr.GS_WRAP + 5,))
def test_dot_restatement_within_its_bound(n):
    for kind in ("normal", "positive", "cancelling"):
        x, y = sr.dot_inputs(n, kind)
        got, ref = gr.gs_dot_blocked(x, y), sr.dot_hp(x, y)
        assert abs(float(np.longdouble(got) - ref)) <= gr.gs_dot_bound(x, y), (n, kind)


def test_update_restatement_is_the_sequential_sum():
    rng = np.random.default_rng(5)
    V, h, w = rng.standard_normal((37, 11)), rng.standard_normal(11), rng.standard_normal(37)
    want = w.copy()
    for i in range(37):
        for c in range(11):
            want[i] = want[i] - h[c] * V[i, c]
    assert np.array_equal(gr.gs_update(V, h, w), want)
    assert np.array_equal(gr.gs_update(V[:, 8:], h[8:], gr.gs_update(V[:, :8], h[:8], w)), want)       # chunks continue the running value


@pytest.mark.parametrize("case,restart,precond", [((8, 4.0), 5, False), ((8, 4.0), 30, False), ((14, 4.0), 5, True), ((14, 4.0), 30, True),
                                                  ((8, 1.0), 5, True), ((8, 1.0), 30, True)])
def test_histories_do_not_depend_on_the_dots_order_beyond_the_bound(case, restart, precond):
    """the cases of the GPU test, each run with numpy's dot, with the kernel's blocked order and with longdouble dots: equal
    iteration counts, histories inside the GPU test's bound, solutions to 1e-9"""
    c = gr.case(*case)
    M = precond_of(c) if precond else None
    runs = [gr.fgmres(c["A"], c["rhs"], restart, max_iter=400, precond=M, dot=d) for d in (gr.dot_ld, gr.gs_dot_blocked, gr.dot64)]
    ref = runs[0]
    assert ref["converged"]
    for s in runs[1:]:
        assert s["iters"] == ref["iters"] and s["converged"]
        d = np.abs(s["hist"] - ref["hist"])
        print(f"{case} restart {restart}: {s['iters']} iterations, max |hist - ref| / r0 = {d.max() / ref['hist'][0]:.2e}, / own = {(d / ref['hist']).max():.2e}")
        assert gr.hist_within(s["hist"], ref["hist"])
        assert sr.rel(s["u"], ref["u"]) <= 1e-9
