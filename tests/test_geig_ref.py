"""The generalised LOBPCG reference of tests/geig_ref.py on the CPU: a correct implementation of the algorithm stays inside every bound
tests/test_gpu_geig.py asserts, the numbers that file takes from geig_ref (iteration counts, B-orthonormality) are what the reference
gives, and the two bounds the GPU test rests on -- the eigenvalue bound and the rounding term of the residual assertion -- hold."""
import numpy as np
import pytest
import scipy.linalg

from tests import eig_ref as er, geig_ref as gg

_RUN = {}
CASES = [(shape, mass) for mass in gg.MASSES for shape in gg.SHAPES]


def run(shape, mass, precond=True):
    """the reference on one shape and mass matrix, once"""
    key = (shape, mass, precond)
    if key not in _RUN:
        m, K, nev = shape
        c = er.case(m)
        _RUN[key] = gg.lobpcg_gen(c["A"], gg.mass(mass, m), er.start_vectors(m ** 3, K), nev, max_iter=100 if precond else 600,
                                  precond=er.vcycle_block(c) if precond else None)
    return _RUN[key]


def test_the_mass_matrices_and_the_closed_form():
    """mass27 is symmetric with 27 entries in an interior row and rows summing to 1 there; its closed-form generalised spectrum with
    poisson(8) against a dense scipy.linalg.eigh(A, B); the clusters of 1 + 3 + 3 the shapes rely on; lumped is diagonal with a jump;
    LAMBDA_MIN_B bounds the smallest eigenvalue of either from below"""
    m = 8
    A, B = er.poisson(m), gg.mass27(m)
    assert abs(B - B.T).max() == 0.0 and int(np.diff(B.indptr).max()) == 27
    interior = (m * m + m + 1) * (m // 2)
    assert abs(B[interior].sum() - 1.0) <= 1e-15
    ev = scipy.linalg.eigh(A.toarray(), B.toarray(), eigvals_only=True)
    assert np.max(np.abs(ev - gg.analytic_mass27(m, m ** 3)) / ev) <= 1e-12
    for mm in (8, 16):
        lam = gg.analytic_mass27(mm, 11)
        gaps = np.diff(lam) / lam[1:]
        assert np.all(gaps[[0, 3, 6]] > 0.05) and np.all(np.delete(gaps, [0, 3, 6, 9]) < 1e-12), (mm, gaps)
    assert np.linalg.eigvalsh(B.toarray())[0] > gg.LAMBDA_MIN_B["mass27"]
    for mm in (8, 16):
        L = gg.lumped(mm)
        d = L.diagonal()
        assert L.nnz == mm ** 3 and d.min() >= gg.LAMBDA_MIN_B["lumped"] and d.max() > 4.0 and d.min() < 1.01
    lam8 = gg.exact("lumped", 8, 7)
    assert np.all(np.diff(lam8) > 0.0)


@pytest.mark.parametrize("shape,mass", CASES, ids=str)
def test_reference_converges_inside_the_bounds(shape, mass):
    """assertions 1 to 3 of the GPU test on the reference itself, and the recorded numbers"""
    m, K, nev = shape
    r = run(shape, mass)
    assert r["converged"]
    A, B = er.case(m)["A"], gg.mass(mass, m)
    rhos = gg.check_pairs(A, B, r["X"], r["lam"], nev, gg.exact(mass, m, nev), gg.LAMBDA_MIN_B[mass], what=f"{shape} {mass}")
    defect = gg.ortho_defect(r["X"], B)
    print(f"{shape} {mass}: {r['iters']} iterations, max |X^T B X - I| = {defect:.3e}")
    assert r["iters"] == gg.ITERS_GEN[(shape, mass)]
    assert r["iters"] <= gg.iteration_bound(shape, mass)
    assert defect <= 2 * gg.ORTHO_GEN[(shape, mass)]           # recorded here; twice: another BLAS adds in another order
    assert np.all(r["res"][:nev] < gg.TOL * r["lam"][:nev] * r["bnorm"][:nev])
    for j in range(nev):                                        # the reported residual is the recomputed one
        assert abs(r["res"][j] - rhos[j] * r["bnorm"][j]) <= 1e-3 * r["res"][j] + 1e-12 * r["lam"][j]
    assert r["hist"].shape == (r["iters"] + 1, K)
    assert np.all(np.diff(r["lam"]) >= -1e-12 * r["lam"][1:])


@pytest.mark.parametrize("shape,mass", CASES, ids=str)
def test_the_vcycle_buys_iterations(shape, mass):
    """the plain counts, and on 16^3 -- where the GPU test asserts it -- the ratio plain / preconditioned >= PLAIN_RATIO_MIN (the
    reference: at least 5 there; 8^3 with `lumped` gives 3.6, too close to 3 to assert on the GPU)"""
    m = shape[0]
    p = run(shape, mass, precond=False)
    assert p["converged"] and p["iters"] == gg.ITERS_GEN_PLAIN[(shape, mass)]
    ratio = p["iters"] / gg.ITERS_GEN[(shape, mass)]
    print(f"{shape} {mass}: {p['iters']} plain iterations, {ratio:.1f} x the preconditioned count")
    if m == 16:
        assert ratio >= 5 > gg.PLAIN_RATIO_MIN
    else:
        assert ratio >= gg.PLAIN_RATIO_MIN


@pytest.mark.parametrize("mass", gg.MASSES)
def test_the_eigenvalue_bound(mass):
    """for a B-normalised x and any lambda, some eigenvalue lambda* of (A, B) has |lambda - lambda*| <= ||A x - lambda B x||_2 /
    sqrt(lambda_min(B)): on 8^3 against the dense spectrum, for iterates far from converged (2 and 6 iterations) and the converged
    ones, with the lower bound LAMBDA_MIN_B in lambda_min's place (a weaker, still true, statement)"""
    m, K, nev = gg.SHAPES[0]
    c = er.case(m)
    A, B = c["A"], gg.mass(mass, m)
    ev = scipy.linalg.eigh(A.toarray(), B.toarray(), eigvals_only=True)
    lmin = np.linalg.eigvalsh(B.toarray())[0]
    assert lmin >= gg.LAMBDA_MIN_B[mass]
    for max_iter in (2, 6, 100):
        r = gg.lobpcg_gen(A, B, er.start_vectors(m ** 3, K), nev, max_iter=max_iter, precond=er.vcycle_block(c))
        for j in range(K):
            x, lam = r["X"][:, j], r["lam"][j]
            assert abs(x @ (B @ x) - 1.0) <= 1e-13
            rho, _, nbx = gg.residual_hp(A, B, x, lam)
            dist = np.min(np.abs(ev - lam))
            assert dist <= rho * nbx / np.sqrt(lmin) * (1 + 1e-12) + 1e-12 * lam, (mass, max_iter, j, dist, rho * nbx)
            assert rho * nbx / np.sqrt(lmin) <= rho * nbx / np.sqrt(gg.LAMBDA_MIN_B[mass])


@pytest.mark.parametrize("shape,mass", CASES, ids=str)
def test_the_rounding_term_covers_float64(shape, mass):
    """the rounding term of assertion 1 dominates the difference between the residual recomputed in longdouble and in float64 on the
    reference's results: a GPU that forms A x - lambda B x in float64 cannot fail assertion 1 through its rounding alone"""
    m, K, nev = shape
    r = run(shape, mass)
    A, B = er.case(m)["A"], gg.mass(mass, m)
    for j in range(nev):
        x, lam = r["X"][:, j], r["lam"][j]
        rho, rounding, nbx = gg.residual_hp(A, B, x, lam)
        Bx = B @ x
        rho64 = np.linalg.norm(A @ x - lam * Bx) / np.linalg.norm(Bx)
        assert abs(rho64 - rho) <= rounding, (shape, mass, j, rho64, rho, rounding)
        assert rounding < 1e-3 * gg.TOL * lam                  # and it is small against the tolerance


def test_scaling_b_scales_the_result():
    """the criterion ||A x - lambda B x|| < tol lambda ||B x|| does not change when B is rescaled: with 4 B the reference takes the
    same iterations, lambda' = lambda / 4 and X' = X / 2"""
    shape = gg.SHAPES[0]
    m, K, nev = shape
    c = er.case(m)
    for mass in gg.MASSES:
        r = run(shape, mass)
        s = gg.lobpcg_gen(c["A"], 4.0 * gg.mass(mass, m), er.start_vectors(m ** 3, K), nev, precond=er.vcycle_block(c))
        assert s["converged"] and abs(s["iters"] - r["iters"]) <= 1
        assert np.all(np.abs(4.0 * s["lam"][:nev] - r["lam"][:nev]) <= 1e-12 * r["lam"][:nev])


def test_max_iter_stop_and_a_b_that_is_not_positive_definite():
    m, K, nev = gg.SHAPES[0]
    c = er.case(m)
    A, B = c["A"], gg.mass("lumped", m)
    X0 = er.start_vectors(m ** 3, K)
    r = gg.lobpcg_gen(A, B, X0, nev, max_iter=2, precond=er.vcycle_block(c))
    assert not r["converged"] and r["iters"] == 2 and np.all(np.isfinite(r["X"])) and np.all(np.isfinite(r["lam"]))
    import scipy.sparse as sp
    with pytest.raises(ValueError, match="not positive definite"):
        gg.lobpcg_gen(A, -sp.identity(m ** 3, format="csr"), X0, nev)
    dep = X0.copy()
    dep[:, 2] = 2.0 * dep[:, 0] - dep[:, 1]
    with pytest.raises(ValueError, match="linearly dependent"):
        gg.lobpcg_gen(A, B, dep, nev)


@pytest.mark.parametrize("mass", gg.STOP_MASSES)
def test_a_solve_stopped_after_its_orthonormalisation(mass):
    """what the GPU test reads after sgpu_debug_eig_stop at iterations 0 and 1: W^T B W = I on the active columns and X^T B W = 0 to
    the recorded figures, the carried BW within bw_bound of B W, exact zeros in the inactive columns (with mass27 column 0 starts as an
    exact eigenvector and is inactive from iteration 0 on; with lumped every column is active), no P in iteration 0"""
    m, K, nev = gg.SHAPES[0]
    c = er.case(m)
    A, B = c["A"], gg.mass(mass, m)
    X0 = gg.stop_start(mass, m, K)
    full = gg.lobpcg_gen(A, B, X0, nev, precond=er.vcycle_block(c))
    assert full["converged"] and full["iters"] > 2
    for k in (0, 1):
        s = gg.lobpcg_gen(A, B, X0, nev, precond=er.vcycle_block(c), stop=k)
        act = s["act"]
        assert act == ([1, 2, 3] if mass == "mass27" else [0, 1, 2, 3])
        wbw, xbw = gg.stop_defects(s, B)
        print(f"{mass}, iteration {k}: max |W^T B W - I| = {wbw:.2e}, max |X^T B W| = {xbw:.2e}")
        assert wbw <= 2 * gg.STOP_GEN[(mass, k)][0] and xbw <= 2 * gg.STOP_GEN[(mass, k)][1]
        assert np.all(np.abs(s["BW"] - B @ s["W"]) <= gg.bw_bound(B, s["W"], s["Tw"], K))
        for name in ("W", "BW", "AW") + (("P", "BP") if k else ()):
            for j in range(K):
                assert np.all(s[name][:, j] == 0.0) == (j not in act), (name, j)
        assert (s["P"] is None) == (k == 0)


def test_restatement_of_the_kernel():
    rng = np.random.default_rng(5)
    AX, BX = rng.standard_normal((37, 4)), rng.standard_normal((37, 4))
    lam = rng.standard_normal(4)
    R, rr, bb = gg.geig_residual(AX, BX, lam)
    assert np.array_equal(R, er.eig_residual(AX, BX, lam))
    assert np.array_equal(R[:, 3], AX[:, 3] - BX[:, 3] * lam[3])
    assert np.allclose(rr, np.sum(R * R, axis=0), rtol=1e-15) and np.allclose(bb, np.sum(BX * BX, axis=0), rtol=1e-15)
