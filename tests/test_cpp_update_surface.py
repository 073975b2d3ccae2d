"""saena::amg::update1 / update2 on the public C++ surface (include/saena.hpp): examples/poisson_update.cpp builds against the
library, the Makefile builds it with the other examples, and on the card it runs a sequence of operators at 16^3 -- fresh
set_matrix, update2 and update1 for each -- with every solve converged."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_update_example_builds(tmp_path):
    exe = str(tmp_path / "poisson_update")
    lib = os.path.join(ROOT, "saena_amd")
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                          os.path.join(ROOT, "examples", "poisson_update.cpp"), "-L" + lib, "-lsaena_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert os.path.exists(os.path.join(ROOT, "examples", "poisson_update")), "the Makefile builds it with the other examples"


@pytest.mark.gpu
def test_the_update_example_runs_and_every_solve_converges():
    exe = os.path.join(ROOT, "examples", "poisson_update")
    assert os.path.exists(exe), "build first (__graft_entry__.build())"
    out = subprocess.run([exe, "16", "3"], capture_output=True, text=True, timeout=300)
    txt = out.stdout
    assert out.returncode == 0, txt[-3000:] + out.stderr[-3000:]
    print(txt)
    assert "rows = 4096" in txt and "every solve converged" in txt
    steps = re.findall(r"step (\d) \(c = (\S+)\): set_matrix (\S+) s, update2 (\S+) s, update1 (\S+) s; pCG iterations fresh (-?\d+), update2 (-?\d+), update1 (-?\d+)", txt)
    assert [int(s[0]) for s in steps] == [1, 2, 3], txt
    for s in steps:
        assert all(float(t) > 0 for t in s[2:5])
        assert all(1 <= int(it) <= 100 for it in s[5:8]), s
