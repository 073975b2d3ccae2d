"""Irregular hierarchies (tests/setup_cases.py; held to the setup's restatement on the CPU by tests/test_setup_contract.py)
through the device:

  * the setup's products on the device kernel (sgpu_spgemm.hip) build the hierarchy the host kernel builds, bit for bit:
    long rows of level 1, positive off-diagonals, lumped diagonals -- rows the Poisson hierarchies of
    tests/test_gpu_spgemm.py do not have.  wgrid16 and SiH4 at the setup's own threshold (200 000 stored entries per
    product); every product of fxm3_6 is below it (at most 112 167 stored entries), so its children lower the threshold
    (SAENA_SPGEMM_HOOK_MIN=1: every product on the device).
  * V-cycle iteration and pCG on the device on a hierarchy the setup built from an irregular operator, against the
    oracle's restatement on the same hierarchy, to the contract of tests/test_gpu_vcycle.py::test_solve_and_pcg_histories."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_HIST = 1e-10

WORKER = r"""
import sys, json
sys.path.insert(0, %(root)r)
from saena_amd import capi, host
from tests import setup_cases
capi.init(0)
L = host.load("gpu")
host.spgemm_stats_reset(L)
A, S = setup_cases.solver(%(name)r, %(tmp)r, which="gpu", kind="rccl", smoother="chebyshev")
out = setup_cases.hashes(S)
out["eig"] = [S.level_info(l)["eig_max"] for l in range(S.num_levels)]
out["stats"] = host.spgemm_stats(L, total=True)
print("RESULT " + json.dumps(out))
"""


def _build(name, tmp, host_spgemm, hook_min=None):
    env = dict(os.environ)
    env.pop("SAENA_HOST_SPGEMM", None)
    env.pop("SAENA_SPGEMM_HOOK_MIN", None)
    if host_spgemm:
        env["SAENA_HOST_SPGEMM"] = "1"
    if hook_min is not None:
        env["SAENA_SPGEMM_HOOK_MIN"] = str(hook_min)
    out = subprocess.run([sys.executable, "-c", WORKER % dict(root=ROOT, name=name, tmp=str(tmp))], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(f"{name} host_spgemm={host_spgemm}: " + " ".join(f"{k}={v}" for k, v in res["stats"].items() if v))
    return res


@pytest.mark.parametrize("name,hook_min", [("wgrid16", None), ("fxm3_6", 1), ("SiH4", None)])
def test_the_device_products_build_the_host_s_irregular_hierarchy(name, hook_min, tmp_path):
    gpu = _build(name, tmp_path, host_spgemm=False, hook_min=hook_min)      # (a child that fails ends the test: nothing runs after it)
    ref = _build(name, tmp_path, host_spgemm=True, hook_min=hook_min)
    sg, sr = gpu.pop("stats"), ref.pop("stats")
    assert sg["on_device"] > 0 and sg["declined"] == 0, sg
    assert sr["on_device"] == 0 and sr["host_hash"] + sr["host_dense"] > 0, sr
    assert gpu["levels"] >= 2
    assert gpu == ref, {k: (gpu.get(k), ref.get(k)) for k in set(gpu) | set(ref) if gpu.get(k) != ref.get(k)}


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_solve_and_pcg_on_an_irregular_hierarchy(capi, smoother):
    from tests import setup_cases
    from tests.test_amg_setup import oracle_amg_from_host
    A, S = setup_cases.solver("wgrid16", which="gpu", kind="rccl", smoother=smoother)
    S.to_device()
    assert S.num_levels == 5
    n = S.level_info(0)["rows"]
    rhs = np.sin(0.37 * np.arange(n) + 0.1)
    amg, _ = oracle_amg_from_host(S, smoother, pre=3, post=3, max_iter=50, tol=1e-8)
    for fn in ("solve_pCG", "solve"):
        u, it, hist, conv = getattr(S, fn)(rhs)
        u_o, it_o, hist_o = getattr(amg, fn)(rhs)
        hist_o = np.asarray(hist_o)
        print(f"wgrid16 {smoother} {fn}: {it} iterations (oracle {it_o}), residual {hist[0]:.6e} -> {hist[-1]:.6e}")
        assert conv and it == it_o, (fn, it, it_o)
        assert len(hist) == len(hist_o)
        assert np.all(np.abs(hist - hist_o) <= TOL_HIST * hist_o[0]), (fn, hist, hist_o)
        assert np.all(np.abs(hist - hist_o) <= 1e-6 * hist_o), (fn, hist, hist_o)
        assert hist[-1] <= 1e-8 * hist[0]
        assert np.linalg.norm(u - u_o) <= 1e-9 * np.linalg.norm(u_o)
