"""saena::amg::eigs_many on the public C++ surface (include/saena.hpp): examples/poisson_eigs_many.cpp builds against the library, the
Makefile builds it with the other examples, and on the card it finds the first 20 modes of Poisson 16^3 from blocks of 8 and prints
them next to the closed form, each inside the closed form's bound.  The C entry's stub is checked on the host library."""
import os
import re
import subprocess

import pytest

from tests import eig_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_eigs_many_example_builds(tmp_path):
    exe = str(tmp_path / "poisson_eigs_many")
    lib = os.path.join(ROOT, "saena_amd")
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                          os.path.join(ROOT, "examples", "poisson_eigs_many.cpp"), "-L" + lib, "-lsaena_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert os.path.exists(os.path.join(ROOT, "examples", "poisson_eigs_many")), "the Makefile builds it with the other examples"


def test_the_host_library_has_the_stub():
    """saena_amg_eigs_many on the host-only library: present, and it says that it needs the GPU library"""
    from saena_amd import host
    L = host.load("host")
    assert L.saena_amg_eigs_many(None, None, 20, 8, 4, None, 100, 1e-8, 1, None, None, None, None, None, None) == -1
    assert b"needs libsaena_amd.so" in L.saena_last_error()


@pytest.mark.gpu
def test_the_eigs_many_example_runs_and_prints_the_closed_form():
    """examples/poisson_eigs_many 16: exits 0 and prints 20 values; every one equals the closed form -- its own and eig_ref.analytic's
    -- within 1e-6 relative and lies within the bound |lambda - closed form| <= residual the driver checks itself"""
    exe = os.path.join(ROOT, "examples", "poisson_eigs_many")
    assert os.path.exists(exe), "build first (__graft_entry__.build())"
    out = subprocess.run([exe, "16"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    rows = re.findall(r"lambda_(\d+) = (\S+)\s+closed form = (\S+)\s+residual = (\S+)\s+(within|OUTSIDE) the bound", out.stdout)
    assert [int(r[0]) for r in rows] == list(range(20)), out.stdout
    exact = er.analytic(16, 20)
    for j, lam, closed, res, verdict in rows:
        j, lam, closed, res = int(j), float(lam), float(closed), float(res)
        assert abs(closed - exact[j]) <= 1e-10 * exact[j], out.stdout
        assert abs(lam - exact[j]) <= 1e-6 * exact[j], out.stdout
        assert abs(lam - exact[j]) <= res + 1e-9 * exact[j] and verdict == "within", out.stdout      # (the values are printed to 11 digits)
    assert "every wanted pair converged" in out.stdout and "20 pairs in" in out.stdout
