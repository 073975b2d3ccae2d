"""Block solves through the public layers: saena_amg_solve_pCG_block (include/saena_c.h, via saena_amd/host.py) and
saena::amg::set_rhs_block / solve_pCG_block (include/saena.hpp, via examples/poisson_block.cpp), on the product's own hierarchy
of laplacian3D 12^3, against the scalar solve of every column."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_HIST = 1e-10                      # tests/test_gpu_vcycle.py: history entries relative to ||r_0|| between two summation orders


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def test_host_layer_solve_pcg_block(capi):
    """K = 2 on laplacian3D 12^3: each column has the iteration count, history and solution of the scalar saena_amg_solve_pCG"""
    from saena_amd import host
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(12).assemble()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    n = A.num_local_rows
    B = np.stack([A.laplacian3D_rhs(), inputs.rhs2(n)], axis=1)
    U, its, hists, conv = S.solve_pCG_block(B)
    assert conv and U.shape == (n, 2)
    for j in range(2):
        u, it, hist, ok = S.solve_pCG(B[:, j])
        assert ok and its[j] == it and len(hists[j]) == len(hist), (j, its[j], it)
        assert np.all(np.abs(hists[j] - hist) <= TOL_HIST * hist[0]) and np.all(np.abs(hists[j] - hist) <= 1e-6 * hist)
        assert np.linalg.norm(U[:, j] - u) <= 1e-9 * np.linalg.norm(u)
    with pytest.raises(Exception, match="2, 4 or 8"):
        S.solve_pCG_block(np.ones((n, 3)))


def test_cpp_surface_poisson_block_driver():
    """examples/poisson_block 12 4: column j is the scalar driver's right-hand side times 2^j, so it takes the scalar
    ./examples/poisson run's iterations and reaches its residuals times 2^j"""
    exe, exe_b = os.path.join(ROOT, "examples", "poisson"), os.path.join(ROOT, "examples", "poisson_block")
    assert os.path.exists(exe) and os.path.exists(exe_b), "build first (__graft_entry__.build())"
    ref = subprocess.run([exe, "12"], capture_output=True, text=True, timeout=120)
    assert ref.returncode == 0, ref.stdout + ref.stderr
    r0 = float(re.search(r"initial residual\s+= (\S+)", ref.stdout).group(1))
    it = int(re.search(r"stopped at iteration\s+= (\d+)", ref.stdout).group(1))
    rn = float(re.search(r"final absolute residual = (\S+)", ref.stdout).group(1))
    out = subprocess.run([exe_b, "12", "4"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    cols = re.findall(r"column (\d): iterations = (\d+), initial residual = (\S+), final absolute residual = (\S+)", out.stdout)
    assert [int(c[0]) for c in cols] == [0, 1, 2, 3], out.stdout
    for c, its, a, b in cols:
        s = 2.0 ** int(c)
        assert int(its) == it, out.stdout
        assert abs(float(a) / (s * r0) - 1) < 2e-6, (out.stdout, ref.stdout)            # (the drivers print seven digits)
        assert abs(float(b) - s * rn) <= TOL_HIST * s * r0 + 2e-6 * s * rn, (out.stdout, ref.stdout)
    assert "every column converged" in out.stdout
