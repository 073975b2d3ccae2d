"""LOBPCG with locking through the public layers: saena_amg_eigs_many (include/saena_c.h, via saena_amd/host.py's
AmgSolver.eigs_many) and sgpu_eigs_LOBPCG_many (via capi.Amg.lobpcg_many) on the product's own hierarchy of Poisson 16^3, for the
standard problem and with the 27-point consistent mass matrix, against the closed-form spectra of tests/eig_ref.py and
tests/geig_ref.py: 20 pairs from blocks of 8.  Every layer returns the C ABI's values: the host layer's call is the same device
call."""
import ctypes as C

import numpy as np
import pytest

from tests import eig_lock_ref as lr, eig_ref as er, geig_ref as gg
from tests.test_gpu_geig_surface import host_matrix

pytestmark = pytest.mark.gpu
M, K, NEV, SWEEP = 16, 8, 20, 4
MASS = "mass27"


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def world(capi):
    """-> (AmgSolver of laplacian3D 18^3 = 16^3 interior rows on the device, host Matrix of mass27(16), the scipy pair)"""
    from saena_amd import host
    L = host.load("gpu")
    comm = host.Comm("gpu", "rccl")
    A = host.Matrix(comm).laplacian3D(M + 2).assemble()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    Bs = gg.mass(MASS, M)
    return S, host_matrix(comm, Bs), er.poisson(M), Bs


def check(Q, lam, res, As, Bs, what):
    """both assertions of check_pairs on all pairs, Q B-orthonormal to 16 x the largest figure the reference records, lambda
    ascending, the reported residuals below the tolerance"""
    nev = len(lam)
    if Bs is None:
        er.check_pairs(As, Q, lam, nev, M, what=what)
        defect = er.ortho_defect(Q)
    else:
        gg.check_pairs(As, Bs, Q, lam, nev, gg.exact(MASS, M, nev), gg.LAMBDA_MIN_B[MASS], what=what)
        defect = gg.ortho_defect(Q, Bs)
    assert defect <= lr.ORTHO_MARGIN * max(lr.ORTHO.values())
    assert np.all(np.diff(lam) >= 0.0)
    for j in range(nev):
        assert res[j] < lr.TOL * lam[j] * (np.linalg.norm(Bs @ Q[:, j]) if Bs is not None else np.linalg.norm(Q[:, j]))


def device_amg(capi, S):
    G = capi.Amg.__new__(capi.Amg)
    G.h, G.destroy = C.c_void_p(S.device_handle()), lambda: None                 # owned by the solver
    return G


@pytest.mark.parametrize("gen", [False, True], ids=["standard", "mass27"])
def test_every_layer_returns_the_c_abi_s_values(capi, world, gen):
    """AmgSolver.eigs_many (saena_amg_eigs_many) finds 20 valid pairs from blocks of 8; Amg.lobpcg_many (sgpu_eigs_LOBPCG_many) on the
    solver's own device hierarchy returns the same bits: lambda, res, Q, the iterations and the sweeps -- with generated start
    vectors and with given ones"""
    from saena_amd import host
    S, B, As, Bs = world
    n = M ** 3
    lam, Q, res, it, sweeps, conv = S.eigs_many(NEV, K, SWEEP, max_iter=lr.MAX_ITER, tol=lr.TOL, B=B if gen else None)
    print(f"{'mass27' if gen else 'standard'}: {it} iterations in {sweeps} sweeps, lambda {lam}")
    assert conv and Q.shape == (n, NEV) and sweeps >= NEV // K and 0 < it <= lr.MAX_ITER
    Q = np.ascontiguousarray(Q)
    check(Q, lam, res, As, Bs if gen else None, "AmgSolver.eigs_many")
    G = device_amg(capi, S)
    Bop = host.device_operator(B) if gen else None
    lam_d, res_d, Q_d, it_d, sweeps_d, conv_d = G.lobpcg_many(n, NEV, K, SWEEP, B=Bop, max_iter=lr.MAX_ITER, tol=lr.TOL)
    assert conv_d and (it_d, sweeps_d) == (it, sweeps)
    for a, b in ((lam_d, lam), (res_d, res), (Q_d, Q)):
        np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    X0 = er.start_vectors(n, K)
    lam_g, Q_g, res_g, it_g, sweeps_g, conv_g = S.eigs_many(NEV, K, SWEEP, x0=X0, max_iter=lr.MAX_ITER, tol=lr.TOL, B=B if gen else None)
    assert conv_g
    check(np.ascontiguousarray(Q_g), lam_g, res_g, As, Bs if gen else None, "given start vectors")
    lam_gd, _, Q_gd, it_gd, _, conv_gd = G.lobpcg_many(n, NEV, K, SWEEP, X0=capi.BlockVector(n, K, X0), B=Bop, max_iter=lr.MAX_ITER, tol=lr.TOL)
    assert conv_gd and it_gd == it_g
    np.testing.assert_array_equal(lam_gd.view(np.uint64), lam_g.view(np.uint64))
    np.testing.assert_array_equal(np.ascontiguousarray(Q_gd).view(np.uint64), np.ascontiguousarray(Q_g).view(np.uint64))


def test_refusals_and_a_small_max_iter(world):
    S, B, As, Bs = world
    with pytest.raises(Exception, match="2, 4 or 8"):
        S.eigs_many(4, 3)
    for nev in (0, 65):
        with pytest.raises(Exception, match="nev must be in 1..64"):
            S.eigs_many(nev, 4)
    with pytest.raises(Exception, match="sweep_nev must be in 1..K"):
        S.eigs_many(4, 4, 5)
    lam, Q, res, it, sweeps, conv = S.eigs_many(NEV, K, SWEEP, max_iter=40, tol=lr.TOL)
    assert not conv and 0 < len(lam) < NEV and Q.shape == (M ** 3, len(lam)) and it <= 40
    check(np.ascontiguousarray(Q), lam, res, As, None, "locked so far")
    # the old entry points still refuse more pairs than a block holds
    with pytest.raises(Exception, match="nev must be in 1..K"):
        S.eigs(K, K + 1)
