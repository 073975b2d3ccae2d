"""saena::amg::set_device_eig and saena::matrix::estimate_eig on the public C++ surface (include/saena.hpp):
examples/poisson_device_eig.cpp builds against the library, the Makefile builds it with the other examples, and on the card it runs
the host and the device estimate side by side at 12^3 -- set_matrix, update2, and update1 after set_eig(estimate_eig())."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_device_eig_example_builds(tmp_path):
    exe = str(tmp_path / "poisson_device_eig")
    lib = os.path.join(ROOT, "saena_amd")
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                          os.path.join(ROOT, "examples", "poisson_device_eig.cpp"), "-L" + lib, "-lsaena_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert os.path.exists(os.path.join(ROOT, "examples", "poisson_device_eig")), "the Makefile builds it with the other examples"


@pytest.mark.gpu
def test_the_device_eig_example_runs_and_every_check_passes():
    exe = os.path.join(ROOT, "examples", "poisson_device_eig")
    assert os.path.exists(exe), "build first (__graft_entry__.build())"
    out = subprocess.run([exe, "12"], capture_output=True, text=True, timeout=300)
    txt = out.stdout
    assert out.returncode == 0, txt[-3000:] + out.stderr[-3000:]
    print(txt)
    assert "rows = 1728" in txt and "every check passed" in txt
    e20, e5 = (float(t) for t in re.search(r"estimate_eig\(\) = (\S+), with 5 steps (\S+)", txt).groups())
    assert 1.0 < e5 < e20 < 2.0002
    for line in ("set_matrix", "update2"):
        h, d = (int(t) for t in re.search(line + r": +pCG iterations host (-?\d+), device (-?\d+)", txt).groups())
        assert 1 <= h <= 100 and abs(h - d) <= 1
    assert 1 <= int(re.search(r"update1 after set_eig\(estimate_eig\(\) = \S+\): pCG iterations (-?\d+)", txt).group(1)) <= 100
