"""tests/lanczos_ref.py held to the host library, and what the order of the sums can move the estimate by (no GPU).

  * anchor: on every level of a Chebyshev hierarchy (Poisson 12^3, plat362) the restatement is within 1e-12 relative of the value the
    host setup computed (saena_amg_level_info) -- the bound tests/test_setup_contract.py holds the setup to;
  * spread: the same recurrence with its dots summed sequentially, pairwise, exactly (math.fsum) and in k_dot_partial's grid-stride
    shape, and with the product taken as (val isd) x and as val (isd x), on five operators.  All estimates of one operator lie within
    1e-13 relative of one another.  Measured here: at most 1.2e-15 (the 9-row diagonal operator; 7e-16 and below on the others).
    sgpu_op_eig_max is held to ten times this bound, 1e-12 (tests/test_gpu_lanczos.py): the margin is for what numpy cannot restate,
    the row sums of the tile forms and fused multiply-adds;
  * the switch without a device: in a process that never called sgpu_init there is no hook, so saena_amg_set_device_eig(1) and
    SAENA_DEVICE_EIG=1 change no bit of any level's estimate, in either library; nor does switching both off again."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from saena_amd import host
from tests import lanczos_ref as lr
from tests import setup_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHOR_BOUND = 1e-12
SPREAD_BOUND = 1e-13
SPREAD_OPERATORS = ("poisson12", "scaled16", "plat362", "diagonal9", "poisson2")


def chebyshev_hierarchy(name):
    L = host.load("host")
    A = host.Matrix(host.Comm("host", "self"))
    if name == "plat362":
        A.read_file(lr.PLAT362)
    else:
        A.laplacian3D(12)
    A.assemble()
    return A, host.AmgSolver(A, host.options(L, **dict(host.OPTIONS001, smoother="chebyshev")))


@pytest.mark.parametrize("name", ["poisson12", "plat362"])
def test_restatement_is_the_host_librarys_estimate(name):
    A, S = chebyshev_hierarchy(name)
    assert S.num_levels >= 2
    for l in range(S.num_levels):
        d = S.level_layout(l, 0)
        got, want = lr.estimate(setup_ref.from_layout(d), d["inv_diag"]), S.level_info(l)["eig_max"]
        rel = abs(got - want) / abs(want)
        print(f"{name} level {l} ({d['M']} rows): restated {got!r}, library {want!r}, relative difference {rel:.2e}")
        assert rel <= ANCHOR_BOUND, (name, l, got, want)


def test_steps_and_short_operators():
    """m = min(steps, n): Poisson 2^3 has 8 rows, so 20 and 64 steps are the same 8; one row ends at its first step with b = 0"""
    A, inv = lr.operator("poisson2")
    assert len(lr.tridiagonal(A, inv, 20)[0]) <= 8
    assert lr.estimate(A, inv, 20) == lr.estimate(A, inv, 64)
    A, inv = lr.operator("one_row")
    alpha, beta = lr.tridiagonal(A, inv, 20)
    assert alpha == [1.0] and beta == []
    assert lr.estimate(A, inv) == lr.FACTOR
    A, inv = lr.operator("poisson12")
    assert lr.estimate(A, inv, 5) < lr.estimate(A, inv, 20) <= lr.estimate(A, inv, 64) * (1 + 1e-14)      # Ritz values grow with the Krylov space


@pytest.mark.parametrize("name", SPREAD_OPERATORS)
def test_summation_order_spread(name):
    A, inv = lr.operator(name)
    est = {(dn, ap): lr.estimate(A, inv, 20, dot, ap) for dn, dot in lr.DOTS.items() for ap in lr.APPLIES}
    v = np.array(list(est.values()))
    spread = (v.max() - v.min()) / abs(v).min()
    print(f"{name} ({A.nrows} rows): {len(v)} orderings, estimates {v.min()!r} .. {v.max()!r}, spread {spread:.2e}")
    assert np.isfinite(v).all()
    assert spread <= SPREAD_BOUND, est


WORKER = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
os.environ.pop("SAENA_DEVICE_EIG", None)
from saena_amd import host
out = {}
for which in ("host", "gpu"):
    L = host.load(which)
    def eigs(device_eig=None, env=None, after=None):
        if env is None:
            os.environ.pop("SAENA_DEVICE_EIG", None)
        else:
            os.environ["SAENA_DEVICE_EIG"] = env
        A = host.Matrix(host.Comm(which, "self")).laplacian3D(12).assemble()
        S = host.AmgSolver(A, host.options(L, **dict(host.OPTIONS001, smoother="chebyshev")), device_eig=device_eig)
        if after is not None:
            S.set_device_eig(after)
            B = host.Matrix(host.Comm(which, "self")).laplacian3D(12).assemble()
            S.update(B, 2)
        return [float(S.level_info(l)["eig_max"]).hex() for l in range(S.num_levels)]
    out[which] = dict(off=eigs(), on_call=eigs(device_eig=True), on_env=eigs(env="1"), on_both_update2=eigs(device_eig=True, env="1", after=True),
                      off_again=eigs(device_eig=False), off_again_update2=eigs(device_eig=True, after=False))
print("RESULT " + json.dumps(out))
"""


def test_switch_without_a_device_changes_no_bit():
    out = subprocess.run([sys.executable, "-c", WORKER % dict(root=ROOT)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for which in ("host", "gpu"):
        r = res[which]
        assert len(r["off"]) >= 2 and all(float.fromhex(e) > 1.0 for e in r["off"])
        for k, v in r.items():
            assert v == r["off"], (which, k, v, r["off"])
    assert res["host"]["off"] == res["gpu"]["off"]
