"""Flexible GMRES through the public layers: saena_amg_solve_pFGMRES (include/saena_c.h, via saena_amd/host.py) on the product's
own hierarchy of laplacian3D 16^3 against saena_amg_solve_pCG, and saena::amg::solve_pFGMRES (include/saena.hpp, via
examples/poisson_fgmres.cpp) on the nonsymmetric convdiff(14, 4.0) with the product's own setup."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def test_host_layer_solve_pfgmres(capi):
    """laplacian3D 16^3, the product's setup: FGMRES converges and finds solve_pCG's solution (both held to rtol 1e-8)"""
    from saena_amd import host
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(16).assemble()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    rhs = A.laplacian3D_rhs()
    u, it, hist, ok = S.solve_pFGMRES(rhs, restart=30)
    up, itp, histp, okp = S.solve_pCG(rhs)
    print(f"FGMRES {it} iterations, estimate {hist[-1] / hist[0]:.2e}; pCG {itp} iterations; rel-l2 {np.linalg.norm(u - up) / np.linalg.norm(up):.2e}")
    assert ok and okp and len(hist) == it + 1 and hist[-1] <= 1e-8 * hist[0]
    assert np.linalg.norm(u - up) <= 1e-7 * np.linalg.norm(up)
    u5, it5, _, ok5 = S.solve_pFGMRES(rhs, restart=3)                       # restarts
    assert ok5 and it5 >= it and np.linalg.norm(u5 - up) <= 1e-7 * np.linalg.norm(up)
    with pytest.raises(Exception, match="restart length"):
        S.solve_pFGMRES(rhs, restart=65)


def test_cpp_surface_poisson_fgmres_driver():
    """examples/poisson_fgmres 14 4: convdiff(14, 4.0) through matrix::set, the product's setup with the Jacobi smoother,
    solve_pFGMRES; the residual recomputed by the driver on the host is below 1e-8 of ||b||"""
    exe = os.path.join(ROOT, "examples", "poisson_fgmres")
    assert os.path.exists(exe), "build first (__graft_entry__.build())"
    out = subprocess.run([exe, "14", "4"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "solve_pFGMRES: converged" in out.stdout
    it = int(re.search(r"iterations = (\d+)", out.stdout).group(1))
    res = float(re.search(r"recomputed relative residual = (\S+)", out.stdout).group(1))
    assert 0 < it <= 100 and res < 1e-8 * (1 + 1e-6), out.stdout
