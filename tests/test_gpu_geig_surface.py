"""The generalised LOBPCG through the public layers: saena_amg_eigs_gen (include/saena_c.h, via saena_amd/host.py's
AmgSolver.eigs(B=...)) and sgpu_eigs_LOBPCG_gen (via capi.Amg.lobpcg(B=...)) on the product's own hierarchy of Poisson 16^3 with the
27-point consistent mass matrix, against the closed-form spectrum of tests/geig_ref.py; and B=None, which must reach the old symbols
with the bits of a direct old call."""
import ctypes as C

import numpy as np
import pytest

from tests import eig_ref as er, geig_ref as gg

pytestmark = pytest.mark.gpu
SHAPE = gg.SHAPES[1]                 # (16, 4, 4)
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
    m = SHAPE[0]
    L = host.load("gpu")
    comm = host.Comm("gpu", "rccl")
    A = host.Matrix(comm).laplacian3D(m + 2).assemble()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    Bs = gg.mass(MASS, m)
    return S, host_matrix(comm, Bs), er.poisson(m), Bs


def host_matrix(comm, Bs, remove_boundary=True):
    """the scipy matrix Bs assembled as a host Matrix, the ordinary way or with the boundary removal switched off"""
    from saena_amd import host
    coo = Bs.tocoo()
    B = host.Matrix(comm)
    if not remove_boundary:
        B.set_remove_boundary(False)
    B.set_many(coo.row.astype(np.int32), coo.col.astype(np.int32), coo.data)
    B.assemble()
    return B


def check(X, lam, res, nev, As, Bs, what, mass=MASS):
    m = SHAPE[0]
    gg.check_pairs(As, Bs, X, lam, nev, gg.exact(mass, m, nev), gg.LAMBDA_MIN_B[mass], what=what)
    assert gg.ortho_defect(X, Bs) <= gg.ORTHO_MARGIN * gg.ORTHO_GEN[(SHAPE, mass)]
    assert np.all(np.diff(lam) >= 0.0)
    for j in range(nev):
        assert res[j] < gg.TOL * lam[j] * np.linalg.norm(Bs @ X[:, j])


@pytest.mark.parametrize("start", ["default", "given"])
def test_host_layer_eigs_gen(world, start):
    """saena_amg_eigs_gen through AmgSolver.eigs(B=...): the pairs meet assertions 1 and 2 of tests/test_gpu_geig.py, X is
    B-orthonormal, the reported residuals are below tol lambda ||B x||"""
    S, B, As, Bs = world
    m, K, nev = SHAPE
    x0 = None if start == "default" else er.start_vectors(m ** 3, K)
    lam, X, res, it, conv = S.eigs(K, nev, x0=x0, max_iter=100, tol=gg.TOL, B=B)
    print(f"{start} start: {it} iterations, lambda {lam}")
    assert conv and 0 < it <= 100 and X.shape == (m ** 3, K)
    check(np.ascontiguousarray(X), lam, res, nev, As, Bs, start)


def test_device_layer_lobpcg_with_b(capi, world):
    """sgpu_eigs_LOBPCG_gen through Amg.lobpcg(B=...) on the solver's own device hierarchy, B's device operator made from the host
    matrix: the same pairs; the host layer's call from the same start gives the same bits (it is the same device call)"""
    from saena_amd import host
    S, B, As, Bs = world
    m, K, nev = SHAPE
    G = capi.Amg.__new__(capi.Amg)
    G.h, G.destroy = C.c_void_p(S.device_handle()), lambda: None                 # owned by the solver
    Bop = host.device_operator(B)
    X0 = er.start_vectors(m ** 3, K)
    dX = capi.BlockVector(m ** 3, K, X0)
    lam, res, it, _, conv = G.lobpcg(dX, nev, max_iter=100, tol=gg.TOL, B=Bop)
    X = dX.download().copy()
    assert conv
    check(X, lam, res, nev, As, Bs, "Amg.lobpcg(B=)")
    lam_h, X_h, res_h, it_h, conv_h = S.eigs(K, nev, x0=X0, max_iter=100, tol=gg.TOL, B=B)
    assert conv_h and it_h == it
    np.testing.assert_array_equal(lam_h.view(np.uint64), lam.view(np.uint64))
    np.testing.assert_array_equal(np.ascontiguousarray(X_h).view(np.uint64), np.ascontiguousarray(X).view(np.uint64))


def test_b_none_reaches_the_old_symbols(capi, world):
    """AmgSolver.eigs() and Amg.lobpcg() without B: the bits of a direct call of saena_amg_eigs / sgpu_eigs_LOBPCG"""
    from saena_amd import host
    S, _, _, _ = world
    m, K, nev = SHAPE
    n = m ** 3
    X0 = er.start_vectors(n, K)
    lam, X, res, it, conv = S.eigs(K, nev, x0=X0, max_iter=100, tol=er.TOL)
    x0 = np.asfortranarray(X0)
    X2 = np.zeros((n, K), order="F")
    lam2, res2, it2 = np.full(K, np.nan), np.full(K, np.nan), C.c_int()
    PD = host._PD
    st = S.L.saena_amg_eigs(S.h, x0.ctypes.data_as(PD), K, nev, 100, er.TOL, 1, lam2.ctypes.data_as(PD), X2.ctypes.data_as(PD), res2.ctypes.data_as(PD),
                            C.byref(it2))
    assert st == 0 and conv and it2.value == it
    for a, b in ((lam, lam2), (res, res2), (np.asfortranarray(X), X2)):
        np.testing.assert_array_equal(np.asarray(a).ravel(order="K").view(np.uint64), np.asarray(b).ravel(order="K").view(np.uint64))
    G = capi.Amg.__new__(capi.Amg)
    G.h, G.destroy = C.c_void_p(S.device_handle()), lambda: None
    dX = capi.BlockVector(n, K, X0)
    lam3, res3, it3, _, conv3 = G.lobpcg(dX, nev, max_iter=100, tol=er.TOL)
    X3 = dX.download().copy()
    dX.upload(X0)
    lam4, res4, it4 = np.full(K, np.nan), np.full(K, np.nan), C.c_int()
    st = capi.lib().sgpu_eigs_LOBPCG(G.h, dX.ptr, K, nev, 100, er.TOL, 1, lam4.ctypes.data_as(capi._PD), res4.ctypes.data_as(capi._PD), C.byref(it4), None, 0)
    assert st == 0 and conv3 and it4.value == it3
    for a, b in ((lam3, lam4), (res3, res4), (X3, dX.download())):
        np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_host_layer_eigs_gen_refuses_and_reports(world):
    S, B, _, _ = world
    with pytest.raises(Exception, match="2, 4 or 8"):
        S.eigs(3, 1, B=B)
    with pytest.raises(Exception, match="nev must be in 1..K"):
        S.eigs(4, 5, B=B)
    assert S.L.saena_amg_eigs_gen(S.h, None, None, 4, 4, 10, 1e-8, 1, None, None, None, None) == -1
    lam, X, res, it, conv = S.eigs(4, 4, max_iter=1, B=B)
    assert not conv and it == 1 and np.all(np.isfinite(lam)) and np.all(np.isfinite(X)) and np.all(np.isfinite(res))


def test_host_layer_eigs_gen_with_a_lumped_mass_matrix(world):
    """the other use case, a diagonal B, through saena_amg_eigs_gen (AmgSolver.eigs(B=...)): assembled with set_remove_boundary(False)
    it gives the pairs of test 1 for `lumped` on (16, 4, 4); assembled the ordinary way assemble() removes every one of its
    single-entry rows as a boundary node, and the call refuses the B that is left with a message that names the switch"""
    S, B27, As, _ = world
    m, K, nev = SHAPE
    Bs = gg.mass("lumped", m)
    B = host_matrix(B27.comm, Bs, remove_boundary=False)
    assert B.num_local_rows == m ** 3
    lam, X, res, it, conv = S.eigs(K, nev, x0=er.start_vectors(m ** 3, K), max_iter=100, tol=gg.TOL, B=B)
    print(f"lumped: {it} iterations, lambda {lam}")
    assert conv and 0 < it <= 100
    check(np.ascontiguousarray(X), lam, res, nev, As, Bs, "lumped", mass="lumped")
    gone = host_matrix(B27.comm, Bs)
    assert gone.num_local_rows == 0
    with pytest.raises(Exception, match="set_remove_boundary"):
        S.eigs(K, nev, B=gone)
