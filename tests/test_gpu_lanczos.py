"""sgpu_op_eig_max (include/saena_gpu.h): the Chebyshev eigenvalue estimate of the host setup, its recurrence on the device.

What is held:
  * the value is tests/lanczos_ref.py's within 1e-12 relative -- ten times the spread tests/test_lanczos_ref.py bounds for the order of
    the sums on the CPU (1e-13; measured 1.2e-15), the margin being what numpy cannot restate: the row sums of the tile forms and fused
    multiply-adds.  The reference sums its dots in k_dot_partial's shape and takes the product as val (isd x), as the device does;
    every case prints its deviation.  Operators: Poisson 12^3 as created and after the autotune, the scaled Poisson 16^3 (entries over
    e^+-6), plat362, a 9-row diagonal operator (the recurrence runs on rounding noise after its first step), Poisson 2^3 (8 rows:
    m = 8 < 20), one row (b = 0 at the first step), Poisson 65^3 (274 625 rows: the first cube past 1024 x 256, where the workgroups of
    the partial sums make a second grid-stride trip); 5 and 64 steps;
  * two calls give the same bits, and so does a second process;
  * the operator afterwards: variant, x-window mode, kernel and code width, and the bits of sgpu_spmv are what they were;
  * every refusal is SGPU_ERR_ARG with its reason in sgpu_last_error()."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lanczos_ref as lr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12
SGPU_ERR_ARG = -1


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


_OPS, _REF = {}, {}


def operator(name):
    if name not in _OPS:
        _OPS[name] = lr.operator(name)
    return _OPS[name]


def reference(name, steps=20):
    """computed once per (operator, steps), never changed"""
    if (name, steps) not in _REF:
        A, inv = operator(name)
        _REF[(name, steps)] = lr.estimate(A, inv, steps, lr.dot_blocked, "val*(isd*x)")
    return _REF[(name, steps)]


def device_operator(capi, name, **kw):
    A, inv = operator(name)
    d = lr.descriptor(A, inv)
    d.update(kw)
    return capi.Operator(**d)


def held(name, got, want):
    rel = abs(got - want) / abs(want)
    print(f"{name}: device {got!r}, reference {want!r}, relative deviation {rel:.2e}")
    assert np.isfinite(got) and rel <= BOUND, (name, got, want, rel)


@pytest.mark.parametrize("name", ["poisson12", "scaled16", "plat362", "diagonal9", "poisson2", "one_row", "poisson65"])
def test_against_the_reference(capi, name):
    op = device_operator(capi, name)
    held(name, op.eig_max(), reference(name))
    assert op.eig_max(0) == op.eig_max(20)                  # 0 steps: the setup's 20
    op.destroy()


def test_after_the_autotune(capi):
    op = device_operator(capi, "poisson12")
    op.autotune()
    print("poisson12 after the autotune:", op.variant(), "x windows", op.x_windows())
    held("poisson12 (autotuned)", op.eig_max(), reference("poisson12"))
    op.destroy()


@pytest.mark.parametrize("steps", [5, 64])
def test_other_step_counts(capi, steps):
    op = device_operator(capi, "poisson12")
    held(f"poisson12, {steps} steps", op.eig_max(steps), reference("poisson12", steps))
    assert op.eig_max(5) < op.eig_max(20)
    op.destroy()


WORKER = r"""
import sys
sys.path.insert(0, %(root)r)
from saena_amd import capi
from tests import lanczos_ref as lr
capi.init(0)
out = []
for name in ("poisson12", "poisson65"):
    op = capi.Operator(**lr.descriptor(*lr.operator(name)))
    out.append(float(op.eig_max()).hex())
print("RESULT " + " ".join(out))
"""


def test_same_bits_from_call_to_call_and_in_a_second_process(capi):
    here = []
    for name in ("poisson12", "poisson65"):
        op = device_operator(capi, name)
        a, b = op.eig_max(), op.eig_max()
        assert float(a).hex() == float(b).hex(), (name, a, b)
        op2 = device_operator(capi, name)                   # another operator of the same entries
        assert float(op2.eig_max()).hex() == float(a).hex()
        here.append(float(a).hex())
        op.destroy(); op2.destroy()
    out = subprocess.run([sys.executable, "-c", WORKER % dict(root=ROOT)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    there = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1].split()[1:]
    assert there == here


@pytest.mark.parametrize("tuned", [False, True])
def test_the_operator_is_left_as_a_product_leaves_it(capi, tuned):
    A, inv = operator("poisson12")
    op = device_operator(capi, "poisson12")
    if tuned:
        op.autotune()
    n = A.nrows
    x, y = capi.DeviceVector(n, np.sin(0.37 * np.arange(n) + 0.1)), capi.DeviceVector(n)
    op.spmv(x, y)
    y0 = y.download()
    state = lambda: (op.variant(), op.x_windows(), op.x_window_kernel(), op.x_window_code_width(), op.info(), op.storage_mask())     # noqa: E731
    before, live = state(), capi.live_bytes()
    op.eig_max()
    assert state() == before
    assert capi.live_bytes() == live, "the call's work space is still allocated"
    y.fill(0.0)
    op.spmv(x, y)
    assert np.array_equal(y.download().view(np.uint64), y0.view(np.uint64))
    op.destroy()


def refused(capi, call, reason):
    st = call()
    msg = capi.lib().sgpu_last_error().decode()
    assert st == SGPU_ERR_ARG and reason in msg, (st, msg, reason)


def test_refusals(capi):
    L, v = capi.lib(), C.c_double(-7.0)
    op = device_operator(capi, "poisson2")
    refused(capi, lambda: L.sgpu_op_eig_max(None, 20, C.byref(v)), "null argument")
    refused(capi, lambda: L.sgpu_op_eig_max(op.h, 20, None), "null argument")
    for steps in (-1, 65, 1000):
        refused(capi, lambda: L.sgpu_op_eig_max(op.h, steps, C.byref(v)), "1..64")
    empty = capi.Operator(M=0, N_local=0, col_offset=0, nnzPerRow_local=[], col_local=[], val_local=[], inv_diag=[])
    refused(capi, lambda: L.sgpu_op_eig_max(empty.h, 20, C.byref(v)), "M == 0")
    wide = capi.Operator(M=3, N_local=5, col_offset=0, nnzPerRow_local=[2, 1, 2], col_local=[0, 3, 1, 2, 4], val_local=[2.0, -1.0, 2.0, 2.0, -1.0],
                         inv_diag=[0.5, 0.5, 0.5])
    refused(capi, lambda: L.sgpu_op_eig_max(wide.h, 20, C.byref(v)), "not square")
    bare = device_operator(capi, "poisson2", inv_diag=None)
    refused(capi, lambda: L.sgpu_op_eig_max(bare.h, 20, C.byref(v)), "no inv_diag")
    from tests import mirror_world as mw
    half = capi.Operator(**mw.rank0_descriptor(mw.mirror_oracle(mw.problem("tridiagonal"), ("rows", mw.EDGE_ROWS))))
    assert half.info()["nnz_remote"] > 0
    refused(capi, lambda: L.sgpu_op_eig_max(half.h, 20, C.byref(v)), "remote part")
    capi.check(L.sgpu_debug_capture(1))
    try:
        refused(capi, lambda: L.sgpu_op_eig_max(op.h, 20, C.byref(v)), "capture is open")
    finally:
        capi.check(L.sgpu_debug_capture(0))
    assert v.value == -7.0, "a refused call wrote its output"
    held("poisson2 after the refusals", op.eig_max(), reference("poisson2"))
    for o in (op, empty, wide, bare, half):
        o.destroy()


MULTI_RANK_WORKER = r"""
import ctypes as C, sys
sys.path.insert(0, %(root)r)
from saena_amd import capi
from tests import lanczos_ref as lr
L = capi.lib()
XF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int)
AF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)
xf, af = XF(lambda *a: 1), AF(lambda *a: 1)                 # never called: nothing is exchanged or reduced before the refusal
capi.check(L.sgpu_debug_init_host_transport(0, 0, 2, C.cast(xf, C.c_void_p), C.cast(af, C.c_void_p), None))
capi._initialised = True
op = capi.Operator(**lr.descriptor(*lr.operator("poisson2")))
v = C.c_double()
st = L.sgpu_op_eig_max(op.h, 20, C.byref(v))
print("RESULT", st, L.sgpu_last_error().decode())
"""


def test_refused_in_a_context_of_two_ranks(capi):
    out = subprocess.run([sys.executable, "-c", MULTI_RANK_WORKER % dict(root=ROOT)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    assert line.split()[1] == str(SGPU_ERR_ARG) and "one rank only (this context has 2)" in line, line
