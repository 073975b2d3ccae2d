"""saena::amg::set_coarse_solver on the public C++ surface (include/saena.hpp): examples/poisson_device_cg.cpp builds against the
library, the Makefile builds it with the other examples, and on the card it solves Poisson 24^3 cut at max_level = 1 (5 324 coarse
rows) with the default coarsest solve and with the device CG side by side.  The C setter's names are checked on the host library."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_device_cg_example_builds(tmp_path):
    exe = str(tmp_path / "poisson_device_cg")
    lib = os.path.join(ROOT, "saena_amd")
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                          os.path.join(ROOT, "examples", "poisson_device_cg.cpp"), "-L" + lib, "-lsaena_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert os.path.exists(os.path.join(ROOT, "examples", "poisson_device_cg")), "the Makefile builds it with the other examples"


def test_the_names_of_the_coarsest_solvers():
    """saena_amg_set_coarse_solver on the host library: the three names, and a refusal that says which they are"""
    from saena_amd import host
    L = host.load("host")
    h = L.saena_amg_new()
    try:
        for name in (b"direct", b"cg", b"device_cg"):
            assert L.saena_amg_set_coarse_solver(h, name) == 0
        for bad in (b"CG", b"", b"lu", None):
            assert L.saena_amg_set_coarse_solver(h, bad) == -1
        assert L.saena_amg_set_coarse_solver(None, b"cg") == -1
    finally:
        L.saena_amg_free(h)


@pytest.mark.gpu
def test_the_device_cg_example_runs_and_every_check_passes():
    exe = os.path.join(ROOT, "examples", "poisson_device_cg")
    assert os.path.exists(exe), "build first (__graft_entry__.build())"
    out = subprocess.run([exe, "24", "1"], capture_output=True, text=True, timeout=300)
    txt = out.stdout
    assert out.returncode == 0, txt[-3000:] + out.stderr[-3000:]
    print(txt)
    assert "rows = 13824, 2 levels" in txt and "every check passed" in txt
    h = int(re.search(r"default: +pCG iterations (-?\d+)", txt).group(1))
    d = int(re.search(r"device_cg: +pCG iterations (-?\d+)", txt).group(1))
    assert 1 <= h <= 100 and abs(h - d) <= 1
    assert float(re.search(r"relative: (\S+)", txt).group(1)) <= 1e-6
