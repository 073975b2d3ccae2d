"""The sparse product C = A B of the AMG setup -- the host kernel (amg_setup.cpp, spgemm_host) and the device kernels
(sgpu_spgemm.hip) -- held to ONE contract, per accumulator path, by two references that share no code with either
(tests/spgemm_ref.py): for every case

  1. the pattern (row pointers, columns) equals the sequential reference's exactly;
  2. the values equal it bit for bit (a NaN only has to be a NaN);
  3. the finite values lie within n eps S of the exactly summed products;
  4. the statistics of the product (host.spgemm_stats) show, row for row, the paths the operands call for, and at least
     one row on the path the case is named after.

Every case runs on the host kernel without a GPU (libsaena_host.so) and on the device under the `gpu` mark, through
saena_debug_spgemm (mode "host" / "device": no size threshold, no quiet fall-back).  The operands and what each case pins
are in tests/spgemm_cases.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from saena_amd import host
from tests import spgemm_cases as K
from tests import spgemm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["light", "medium", "try", "lds", "hbm", "chunks", "offsets", "threshold", "specials", "rehash", "real"]


@pytest.fixture(scope="module")
def gpu_lib():
    from saena_amd import capi
    capi.init(0)
    return host.load("gpu")


# ---- the references themselves ------------------------------------------------------------------------------------------------
def _small_operands(seed):
    rng = np.random.default_rng(seed)
    k, n, m = 23, 31, 19
    Brows = [K.brow(rng, np.arange(n), rng.integers(0, 9)) for _ in range(k)]
    Arows = [K.arow(rng, rng.choice(k, rng.integers(0, 8))) for _ in range(m)]          # with replacement: repeated columns
    Arows[3] = (np.array([5, 5, 5]), np.array([1e16, 1.0, -1e16]))
    Brows[5] = (np.array([0, 3, 30]), np.array([1.0, 1.0, np.inf]))
    Arows[4] = (np.array([6, 7]), np.array([3.0, -3.0]))
    Brows[6] = Brows[7] = (np.array([4, 9]), np.array([0.1, 0.7]))                        # exact zeros on (4, 4) and off the diagonal
    return R.csr(Arows, k), R.csr(Brows, n)


@pytest.mark.parametrize("row_offset", [0, 5])
def test_the_vectorised_reference_is_the_plain_loop(row_offset):
    for seed in (1, 2, 3):
        A, B = _small_operands(seed)
        R.check_operands(A, B)
        ptr, col, val, info = R.sequential(A, B, row_offset)
        lptr, lcol, lval = R.sequential_loop(A, B, row_offset)
        np.testing.assert_array_equal(ptr, lptr)
        np.testing.assert_array_equal(col, lcol)
        R.assert_same_values(val, lval, "vectorised against loop")
        assert len(col) > 40
        if row_offset == 0:
            assert 4 in col[ptr[4]:ptr[5]] and 9 not in col[ptr[4]:ptr[5]]               # the zero stays on the diagonal only
        ex, S = R.exact(info["E"])
        fin = np.isfinite(S)
        assert np.all(np.abs(info["value"][fin] - ex[fin]) <= R.bound(info["E"], S)[fin])


def test_the_exact_reference_sees_what_a_sequential_sum_loses():
    A = R.csr([([0, 1, 2], [1.0, 1.0, 1.0])], 3)
    B = R.csr([([0, 1], [1e16, 1e16]), ([0, 1], [1.0, -1e16]), ([0, 1], [-1e16, 1.0])], 2)
    _, col, val, info = R.sequential(A, B, row_offset=7)
    assert col.tolist() == [1] and val.tolist() == [1.0]                                  # 1e16 + 1 - 1e16 = 0 is dropped, 1e16 - 1e16 + 1 = 1
    ex, S = R.exact(info["E"])
    assert ex.tolist() == [1.0, 1.0] and S.tolist() == [2e16 + 1, 2e16 + 1]
    assert np.all(np.abs(info["value"] - ex) <= R.bound(info["E"], S))


def test_operand_check_refuses_what_the_kernels_must_not_see():
    """precondition violations are an error of the entry point; they never reach a kernel"""
    L = host.load("host")
    ap, ac, av = [0, 2], [0, 1], [1.0, 1.0]
    for b_col, a_col in (([2, 1, 0], ac), ([1, 1, 2], ac), ([0, 1, 7], ac), ([0, 1, 2], [0, 2])):
        with pytest.raises(host.SgpuError):
            host.spgemm(L, ap, a_col, av, [0, 2, 3], b_col, [1.0, 2.0, 3.0], 3, mode="host")
    with pytest.raises(host.SgpuError, match="no device kernel"):                            # and "device" never means "host"
        host.spgemm(L, ap, ac, av, [0, 2, 3], [0, 1, 2], [1.0, 2.0, 3.0], 3, mode="device")


# ---- the cases, host and device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_kernel(name):
    K.run_case(host.load("host"), "host", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_kernels(gpu_lib, name):
    K.run_case(gpu_lib, "device", name)
    if name == "chunks":
        K.decline_legs(gpu_lib)


CHILD = r"""
import sys, json
sys.path.insert(0, %(root)r)
from saena_amd import capi, host
from tests import spgemm_cases as K
capi.init(0)
L = host.load("gpu")
print("RESULT " + json.dumps({name: K.run_case(L, "device", name) for name in %(names)r}))
"""


@pytest.mark.gpu
def test_device_kernels_hbm_accumulator_in_a_process_without_the_lds_form():
    """SAENA_SPGEMM_NO_LDS=1: the rows that overflow the table accumulate in HBM -- the `lds` operands of up to two windows
    and a column, and the `threshold` and `chunks` products, with the same assertions (run in the child)"""
    env = dict(os.environ, SAENA_SPGEMM_NO_LDS="1")
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, names=["hbm_no_lds", "threshold", "chunks"])], env=env,
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for name, stats in res.items():
        assert all(s["lds"] == 0 and s["windows"] == 0 for s in stats) and sum(s["hbm"] for s in stats) > 0, (name, stats)


# ---- the public product and its size threshold --------------------------------------------------------------------------------
def _bidiagonal(L, which, n_entries):
    """an assembled matrix of exactly n_entries stored entries: a diagonal, an upper diagonal, and entries (i, i + 7) as needed"""
    rng = np.random.default_rng(77)
    M = 50000
    rows = np.concatenate([np.arange(M), np.arange(M - 1), np.arange(n_entries - 2 * M + 1)])
    cols = np.concatenate([np.arange(M), np.arange(1, M), np.arange(n_entries - 2 * M + 1) + 7])
    vals = rng.uniform(1.0, 2.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    A = host.Matrix(host.Comm(which, "self" if which == "host" else "rccl"))
    A.set_remove_boundary(False)
    A.set_many(rows, cols, vals)
    A.assemble()
    assert A.local_nnz == n_entries == len(rows)
    import scipy.sparse as sp
    return A, R.from_scipy(sp.csr_matrix((vals, (rows, cols)), shape=(M, M)))


def _matmat_leg(L, which, n_entries, on_device):
    A, ref_A = _bidiagonal(L, which, n_entries)
    C = A.matmat(A)
    st = host.spgemm_stats(L)
    print(f"matmat {2 * n_entries} stored entries [{which}]: " + " ".join(f"{k}={v}" for k, v in st.items() if v))
    assert st["on_device"] == on_device and st["declined"] == 0
    assert (st["host_hash"] + st["host_dense"] == 0) == bool(on_device) and (st["light"] > 0) == bool(on_device)
    ptr, col, val, _ = R.sequential(ref_A, ref_A)
    d = C.layout()
    np.testing.assert_array_equal(np.cumsum(d["nnzPerRow_local"]), ptr[1:])
    np.testing.assert_array_equal(d["col_local"], col)
    R.assert_same_values(d["val_local"], val, "matmat")
    C.free(); A.free()


def test_matmat_host_library_multiplies_on_the_host_on_both_sides_of_the_threshold():
    L = host.load("host")
    _matmat_leg(L, "host", 99999, 0)
    _matmat_leg(L, "host", 100000, 0)


@pytest.mark.gpu
def test_matmat_takes_the_device_kernel_from_200000_stored_entries(gpu_lib):
    """saena::amg::matmat below the threshold (199 998 stored entries in A and B) multiplies on the host, at it (200 000) on the
    device: same C as the reference either way"""
    _matmat_leg(gpu_lib, "gpu", 99999, 0)
    _matmat_leg(gpu_lib, "gpu", 100000, 1)
