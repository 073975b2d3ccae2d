"""saena::amg::set_null_space on the public surfaces (include/saena.hpp, include/saena_c.h, saena_amd/host.py):
examples/poisson_neumann.cpp builds against the library, the Makefile builds it with the other examples, and on the card it solves the
pure-Neumann Laplacian of a 12^3 box with an inconsistent right-hand side, then finds its smallest nonzero eigenvalues.  The setter's
names are checked on the host library; the refusals of the solvers that do not take such a hierarchy, and AmgSolver.eigs against the
C ABI's locked solve, on the card."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_neumann_example_builds(tmp_path):
    exe = str(tmp_path / "poisson_neumann")
    lib = os.path.join(ROOT, "saena_amd")
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                          os.path.join(ROOT, "examples", "poisson_neumann.cpp"), "-L" + lib, "-lsaena_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert os.path.exists(os.path.join(ROOT, "examples", "poisson_neumann")), "the Makefile builds it with the other examples"


def test_the_names_of_the_null_spaces():
    """saena_amg_set_null_space on the host library: the two names, and a refusal of anything else"""
    from saena_amd import host
    L = host.load("host")
    h = L.saena_amg_new()
    try:
        for name in (b"none", b"constant"):
            assert L.saena_amg_set_null_space(h, name) == 0
        for bad in (b"constants", b"", b"Constant"):
            assert L.saena_amg_set_null_space(h, bad) == -1
            assert b"neither none nor constant" in L.saena_last_error()
        assert L.saena_amg_set_null_space(h, None) == -1
        assert L.saena_amg_set_null_space(None, b"none") == -1
    finally:
        L.saena_amg_free(h)


@pytest.mark.gpu
def test_the_neumann_example_runs():
    exe = os.path.join(ROOT, "examples", "poisson_neumann")
    assert os.path.exists(exe), "build first (__graft_entry__.build())"
    out = subprocess.run([exe, "12"], capture_output=True, text=True, timeout=300)
    txt = out.stdout
    assert out.returncode == 0, txt[-3000:] + out.stderr[-3000:]
    print(txt)
    assert "rows = 1728" in txt and "solve_pCG: converged" in txt and "every wanted pair converged" in txt
    its = int(re.search(r"iterations = (\d+)", txt).group(1))
    res = float(re.search(r"recomputed relative residual = (\S+)", txt).group(1))
    mean = float(re.search(r"mean\(u\) = (\S+)", txt).group(1))
    assert abs(float(re.search(r"mean\(b\) = (\S+)", txt).group(1)) - 0.5) < 0.01        # the right-hand side is not consistent
    assert 4 <= its <= 10                                    # 6 to 8 in tests/test_null_space_ref.py's hierarchies of this kind
    assert res <= 1.01e-8
    assert abs(mean) <= 1e-13                                # dot_roundings(1728) = 24 roundings of mean|u| <= rms(b~) / lambda_2 = 0.72 / 0.068: 2.8e-14
    exact = 2.0 - 2.0 * np.cos(np.pi / 12)
    lam = [float(v) for v in re.findall(r"lambda_\d = (\S+)", txt)]
    assert len(lam) == 3 and max(abs(v - exact) / exact for v in lam) <= 1e-9


REFUSALS_DRIVER = r"""
// every refusal of a solver that knows the constant null space, through include/saena.hpp: each exception's what() on a line of its own
#include "saena.hpp"
#include <cstdio>
#include <exception>
#include <vector>

static void neumann(saena::matrix &A, index_t n, bool pin) {
    A.set_remove_boundary(false);
    for (index_t k = 0; k < n; ++k) for (index_t j = 0; j < n; ++j) for (index_t i = 0; i < n; ++i) {
        const index_t r = (k * n + j) * n + i;
        const index_t nb[6] = {i > 0 ? r - 1 : -1, i < n - 1 ? r + 1 : -1, j > 0 ? r - n : -1, j < n - 1 ? r + n : -1, k > 0 ? r - n * n : -1, k < n - 1 ? r + n * n : -1};
        int deg = 0;
        for (index_t c : nb) if (c >= 0) { ++deg; if (!pin || (r != 0 && c != 0)) A.set(r, c, -1.0); }
        A.set(r, r, pin && r == 0 ? 1.0 : (value_t)deg);
    }
    A.assemble();
}

template <class F> static void attempt(const char *name, F f) {
    try { f(); printf("%s: no exception\n", name); }
    catch (const std::exception &e) { printf("%s: %s\n", name, e.what()); }
}

int main() {
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;
    const index_t n = 6, N = n * n * n;
    saena::options opts(100, 1e-8, "jacobi", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);
    {
        saena::amg s;
        attempt("NAME", [&] { s.set_null_space("bogus"); });
        attempt("NAME_OK", [&] { s.set_null_space("none"); s.set_null_space("constant"); });
    }
    {
        saena::matrix P(comm);
        neumann(P, n, true);
        saena::amg s;
        s.set_scale(false);
        s.set_null_space("constant");
        attempt("PINNED", [&] { s.set_matrix(&P, &opts); });
    }
    saena::matrix A(comm);
    neumann(A, n, false);
    saena::amg solver;
    solver.set_scale(false);
    solver.set_null_space("constant");
    solver.set_matrix(&A, &opts);
    std::vector<value_t> b((size_t)N, 0.0);
    for (index_t i = 0; i < N; ++i) b[(size_t)i] = 0.5 + (i % 7) * 0.1;
    solver.set_rhs(b.data(), N);
    value_t *u = nullptr, *x = nullptr, *q = nullptr;
    std::vector<value_t> lambda;
    attempt("PCG", [&] { printf("pcg status %d\n", solver.solve_pCG(u, &opts, false)); });
    attempt("FGMRES", [&] { solver.solve_pFGMRES(u, &opts); });
    attempt("EIGS_GEN", [&] { solver.eigs_gen(x, lambda, &A, &opts, 4, 3); });
    attempt("EIGS_MANY", [&] { solver.eigs_many(q, lambda, &opts, 6, 4); });
    saena::finalize();
    return 0;
}
"""


@pytest.mark.gpu
def test_the_refusals_through_the_cpp_surface(tmp_path):
    """include/saena.hpp: set_null_space refuses a name that is none, set_matrix a pinned matrix (the level and the value are in the
    message), solve_pFGMRES, eigs_gen and eigs_many a solver that knows the null space -- each as an exception whose text says why;
    solve_pCG on the same solver runs"""
    src, exe = tmp_path / "refusals.cpp", str(tmp_path / "refusals")
    src.write_text(REFUSALS_DRIVER)
    lib = os.path.join(ROOT, "saena_amd")
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src),
                          "-L" + lib, "-lsaena_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    print(run.stdout)
    line = {ln.split(":", 1)[0]: ln.split(":", 1)[1] for ln in run.stdout.splitlines() if ":" in ln}
    assert 'set_null_space: "bogus" is neither none nor constant' in line["NAME"]
    assert "no exception" in line["NAME_OK"] and "no exception" in line["PCG"] and "pcg status 0" in run.stdout
    assert re.search(r"level 0 does not annihilate constants: max\|A 1\| / max\|a_ii\| = 1\.\d+e-01 exceeds 1e-10", line["PINNED"])
    assert "symmetric solvers only" in line["FGMRES"]
    assert "eigs_LOBPCG_gen" in line["EIGS_GEN"] and "sgpu_eigs_LOBPCG_locked" in line["EIGS_GEN"]
    assert "eigs_LOBPCG_many" in line["EIGS_MANY"] and "sgpu_eigs_LOBPCG_locked" in line["EIGS_MANY"]


@pytest.mark.gpu
def test_the_host_layer_on_the_card():
    """AmgSolver(null_space="constant"): solve_pCG on an inconsistent right-hand side returns the zero-mean solution; eigs returns the
    smallest nonzero pairs of the 12 x 8 x 5 box; solve_pFGMRES, eigs with B and eigs_many pass the library's refusals through; a
    pinned matrix is refused by to_device with the reason"""
    from saena_amd import capi, host
    from tests import null_space_ref as ns, solver_ref as sr
    capi.init(0)
    L = host.load("gpu")

    def solver(A0, **kw):
        M = host.Matrix(host.Comm("gpu", "rccl"))
        M.set_remove_boundary(False)
        coo = A0.tocoo()
        M.set_many(coo.row.astype(np.int32), coo.col.astype(np.int32), coo.data)
        M.assemble()
        return M, host.AmgSolver(M, host.options(L, **host.OPTIONS001), **kw)

    A0 = ns.neumann3d(*ns.EIG_BOX)
    n = A0.shape[0]
    M, S = solver(A0, null_space="constant")
    S.to_device()
    rhs = ns.rhs_for(n) + 0.5
    u, it, hist, conv = S.solve_pCG(rhs)
    bt = ns.center(rhs)[0]
    assert conv and 4 <= it <= 10
    assert sr.residual_hp(A0, u, bt) <= 1.01 * ns.TOL * np.linalg.norm(bt)
    assert abs(float(sr.dot_hp(u, np.ones(n)) / n)) <= sr.dot_bound(u, np.ones(n)) / n
    lam, X, res, its, ok = S.eigs(4, 3)
    c = lambda k: 2 - 2 * np.cos(np.pi / k)      # noqa: E731
    exact = np.array([c(12), c(8), c(12) + c(8)])
    print(its, lam[:3], exact)
    assert ok and np.max(np.abs(lam[:3] - exact) / exact) <= 1e-9
    assert np.max(np.abs(np.ones(n) @ X[:, :3])) <= 1e-10 * np.sqrt(n)
    with pytest.raises(capi.SgpuError, match="symmetric solvers only"):
        S.solve_pFGMRES(rhs)
    with pytest.raises(capi.SgpuError, match="sgpu_eigs_LOBPCG_locked"):
        S.eigs_many(6, K=4)
    with pytest.raises(capi.SgpuError, match="sgpu_eigs_LOBPCG_locked"):
        S.eigs(4, 3, B=M)
    _, Sp = solver(ns.pinned(A0), null_space="constant")
    with pytest.raises(capi.SgpuError, match="level 0 does not annihilate constants"):
        Sp.to_device()
