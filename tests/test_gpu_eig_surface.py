"""LOBPCG through the public layers: saena_amg_eigs (include/saena_c.h, via saena_amd/host.py's AmgSolver.eigs) with the default
start and with given start vectors, and saena::amg::eigs (include/saena.hpp, via examples/poisson_eigs.cpp), on the product's own
hierarchy, against the closed-form spectrum of tests/eig_ref.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import eig_ref as er

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def solver(capi):
    from saena_amd import host
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(10).assemble()        # 8^3 interior rows
    return host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()


@pytest.mark.parametrize("start", ["default", "given"])
def test_host_layer_eigs(solver, start):
    """K = 4, nev = 4 on laplacian3D 10^3: the pairs meet assertions 1 and 2 of tests/test_gpu_eig.py, X is orthonormal and the
    reported residuals are below the tolerance"""
    m, K, nev = 8, 4, 4
    x0 = None if start == "default" else er.start_vectors(m ** 3, K)
    lam, X, res, it, conv = solver.eigs(K, nev, x0=x0, max_iter=100, tol=er.TOL)
    print(f"{start} start: {it} iterations, lambda {lam}")
    assert conv and 0 < it <= 100 and X.shape == (m ** 3, K)
    er.check_pairs(er.poisson(m), X, lam, nev, m, what=start)
    assert er.ortho_defect(X) <= 1e-13
    assert np.all(res[:nev] < er.TOL * lam[:nev])


def test_host_layer_eigs_refuses_and_reports(solver):
    with pytest.raises(Exception, match="2, 4 or 8"):
        solver.eigs(3, 1)
    with pytest.raises(Exception, match="nev must be in 1..K"):
        solver.eigs(4, 5)
    lam, X, res, it, conv = solver.eigs(4, 4, max_iter=1)
    assert not conv and it == 1 and np.all(np.isfinite(lam)) and np.all(np.isfinite(X)) and np.all(np.isfinite(res))


def test_cpp_surface_poisson_eigs_driver():
    """examples/poisson_eigs 16: exits 0, and every wanted eigenvalue it prints equals the closed form -- its own and
    eig_ref.analytic's -- to the digits printed"""
    exe = os.path.join(ROOT, "examples", "poisson_eigs")
    assert os.path.exists(exe), "build first (__graft_entry__.build())"
    out = subprocess.run([exe, "16"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = re.findall(r"lambda_(\d) = (\S+)\s+closed form = (\S+)\s+residual = (\S+)", out.stdout)
    assert [int(r[0]) for r in rows] == [0, 1, 2, 3], out.stdout
    exact = er.analytic(16, 4)
    for j, lam, closed, res in rows:
        j, lam, closed, res = int(j), float(lam), float(closed), float(res)
        assert abs(closed - exact[j]) <= 1e-10 * exact[j], out.stdout
        assert abs(lam - exact[j]) <= 1e-10 * exact[j], out.stdout               # (eleven digits are printed)
        assert res < er.TOL * lam, out.stdout
    assert "every wanted pair converged" in out.stdout
