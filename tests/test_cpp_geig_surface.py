"""saena::amg::eigs_gen on the public C++ surface (include/saena.hpp): examples/poisson_geigs.cpp builds against the library, the
Makefile builds it with the other examples, and on the card it solves K x = lambda M x on Poisson 16^3 with the 27-point consistent
mass matrix and prints the pairs next to the closed form.  The C entry's stub is checked on the host library."""
import os
import re
import subprocess

import pytest

from tests import geig_ref as gg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_geigs_example_builds(tmp_path):
    exe = str(tmp_path / "poisson_geigs")
    lib = os.path.join(ROOT, "saena_amd")
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                          os.path.join(ROOT, "examples", "poisson_geigs.cpp"), "-L" + lib, "-lsaena_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert os.path.exists(os.path.join(ROOT, "examples", "poisson_geigs")), "the Makefile builds it with the other examples"


def test_the_host_library_has_the_stub():
    """saena_amg_eigs_gen on the host-only library: present, and it says that it needs the GPU library"""
    from saena_amd import host
    L = host.load("host")
    assert L.saena_amg_eigs_gen(None, None, None, 4, 4, 10, 1e-8, 1, None, None, None, None) == -1
    assert b"needs libsaena_amd.so" in L.saena_last_error()


@pytest.mark.gpu
def test_the_geigs_example_runs_and_prints_the_closed_form():
    """examples/poisson_geigs 16: exits 0, and every wanted eigenvalue it prints equals the closed form -- its own and
    geig_ref.analytic_mass27's -- within 1e-6 relative"""
    exe = os.path.join(ROOT, "examples", "poisson_geigs")
    assert os.path.exists(exe), "build first (__graft_entry__.build())"
    out = subprocess.run([exe, "16"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    rows = re.findall(r"lambda_(\d) = (\S+)\s+closed form = (\S+)\s+residual = (\S+)", out.stdout)
    assert [int(r[0]) for r in rows] == [0, 1, 2, 3], out.stdout
    exact = gg.analytic_mass27(16, 4)
    for j, lam, closed, res in rows:
        j, lam, closed, res = int(j), float(lam), float(closed), float(res)
        assert abs(closed - exact[j]) <= 1e-10 * exact[j], out.stdout
        assert abs(lam - exact[j]) <= 1e-6 * exact[j], out.stdout
    assert "every wanted pair converged" in out.stdout
