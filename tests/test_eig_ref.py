"""The LOBPCG reference of tests/eig_ref.py on the CPU: a correct implementation of the algorithm stays inside every bound
tests/test_gpu_eig.py asserts, and the numbers that file takes from eig_ref (iteration counts, orthonormality, the ratio of plain to
preconditioned iterations) are what the reference gives."""
import numpy as np
import pytest

from tests import eig_ref as er

_RUN = {}


def run(shape, precond=True):
    """the reference on one shape, once"""
    if (shape, precond) not in _RUN:
        m, K, nev = shape
        c = er.case(m)
        _RUN[(shape, precond)] = er.lobpcg(c["A"], er.start_vectors(m ** 3, K), nev, max_iter=100 if precond else 400,
                                          precond=er.vcycle_block(c) if precond else None)
    return _RUN[(shape, precond)]


def test_analytic_is_the_spectrum_of_the_generated_operator():
    """the closed form against numpy.linalg.eigvalsh on 8^3 -- the generator's (m+1)^2 scaling included -- and the clusters of
    1 + 3 + 3 eigenvalues the shapes rely on"""
    ev = np.linalg.eigvalsh(er.poisson(8).toarray())
    assert np.max(np.abs(ev - er.analytic(8, 512)) / ev) <= 1e-12
    for m in (8, 16):
        lam = er.analytic(m, 11)
        gaps = np.diff(lam) / lam[1:]
        assert np.all(gaps[[0, 3, 6]] > 0.05) and np.all(np.delete(gaps, [0, 3, 6, 9]) < 1e-12), (m, gaps)
        assert er.case(m)["As"][-1].shape[0] == 64 and len(er.case(m)["As"]) == (2 if m == 8 else 3)


@pytest.mark.parametrize("shape", er.SHAPES, ids=str)
def test_reference_converges_inside_the_bounds(shape):
    """assertions 1 to 4 of the GPU test on the reference itself, and the recorded numbers"""
    m, K, nev = shape
    r = run(shape)
    assert r["converged"]
    A = er.case(m)["A"]
    er.check_pairs(A, r["X"], r["lam"], nev, m, what=str(shape))
    defect = er.ortho_defect(r["X"])
    print(f"{shape}: {r['iters']} iterations, max |X^T X - I| = {defect:.3e}")
    assert r["iters"] == er.ITERS[shape]
    assert r["iters"] <= er.iteration_bound(shape)
    assert defect <= 2 * er.ORTHO[shape]                       # recorded here; twice: another BLAS adds in another order
    assert np.all(r["res"][:nev] < er.TOL * r["lam"][:nev])
    assert r["hist"].shape == (r["iters"] + 1, K)
    assert np.all(np.diff(r["lam"]) >= -1e-12 * r["lam"][1:])


@pytest.mark.parametrize("shape", er.SHAPES, ids=str)
def test_the_vcycle_buys_iterations(shape):
    p = run(shape, precond=False)
    assert p["converged"] and p["iters"] == er.ITERS_PLAIN[shape]
    ratio = p["iters"] / er.ITERS[shape]
    print(f"{shape}: {p['iters']} plain iterations, {ratio:.1f} x the preconditioned count")
    assert ratio >= er.PLAIN_RATIO_MIN


def test_a_second_solve_from_the_result_takes_no_iteration():
    shape = er.SHAPES[0]
    m, K, nev = shape
    r = run(shape)
    c = er.case(m)
    again = er.lobpcg(c["A"], r["X"], nev, precond=er.vcycle_block(c))
    assert again["converged"] and again["iters"] == 0
    assert np.all(np.abs(again["lam"][:nev] - r["lam"][:nev]) <= er.TOL * r["lam"][:nev])


def test_max_iter_and_dependent_start_vectors():
    m, K, nev = er.SHAPES[0]
    c = er.case(m)
    X0 = er.start_vectors(m ** 3, K)
    r = er.lobpcg(c["A"], X0, nev, max_iter=2, precond=er.vcycle_block(c))
    assert not r["converged"] and r["iters"] == 2 and np.all(np.isfinite(r["X"])) and np.all(np.isfinite(r["lam"])) and np.all(np.isfinite(r["res"]))
    X0[:, 2] = 2.0 * X0[:, 0] - X0[:, 1]
    with pytest.raises(ValueError, match="dependent"):
        er.lobpcg(c["A"], X0, nev)


def test_restatements_of_the_kernels():
    """block_mix is the matrix product up to rounding, in the documented order; a zero coefficient row contributes 0 * S (a NaN
    there propagates, as IEEE says); eig_residual is AX - X diag(lam)"""
    rng = np.random.default_rng(3)
    S = [rng.standard_normal((37, 4)) for _ in range(3)]
    Cm = [rng.standard_normal((4, 4)) for _ in range(3)]
    add = rng.standard_normal((37, 4))
    for ns in (1, 2, 3):
        want = sum(S[s] @ Cm[s] for s in range(ns))
        assert np.max(np.abs(er.block_mix(S[:ns], Cm[:ns]) - want)) <= 1e-13
        assert np.max(np.abs(er.block_mix(S[:ns], Cm[:ns], add=add) - (want + add))) <= 1e-13
    one = er.block_mix(S[:1], Cm[:1])
    acc = np.zeros(37)
    for a in range(4):
        acc = acc + S[0][:, a] * Cm[0][a, 2]
    assert np.array_equal(one[:, 2], acc)
    Sn, Cz = S[0].copy(), Cm[0].copy()
    Sn[5, 1], Cz[1] = np.nan, 0.0
    out = er.block_mix([Sn], [Cz])
    assert np.all(np.isnan(out[5])) and np.all(np.isfinite(np.delete(out, 5, axis=0)))
    lam = rng.standard_normal(4)
    assert np.array_equal(er.eig_residual(S[0], S[1], lam)[:, 3], S[0][:, 3] - S[1][:, 3] * lam[3])
