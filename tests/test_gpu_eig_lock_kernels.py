"""The kernels of LOBPCG's hard locking on the GPU (saena_amd/csrc/kernels_eig_lock.hip.h), held to their written contracts through
sgpu_debug_lock_gram / _lock_project / _block_refill, which run the solver's own launch helpers on the caller's arrays.

The locked set is column-major, column l at l * ld: 64 columns of standard normal values are uploaded once, and every (n, ld) is
built from them ON THE DEVICE (a NaN fill, then one copy of n values per column), so the padding rows n .. ld-1 hold NaN and a
kernel that reads one poisons its result.  Sizes are solver_ref.BLOCK_VEC_SIZES (the second grid-stride trip of the Gram kernel past
262144 rows and of the projection past 524288 included), K in {2, 4, 8}, L in {1, 7, 8, 9, 17, 64} -- a lone tail pass, the fullest
tail, one full pass, full + 1, two full + 1, eight full passes -- and ld = n rounded up to even, and n + 6 rounded up to even.
"""
import ctypes as C

import numpy as np
import pytest

from tests import eig_lock_ref as lr, solver_ref as sr
from tests.test_gpu_block_solver_layer import KS, Blk, same_bits
from tests.test_gpu_solver_layer import SENTINEL, Padded, gpu_dot, one_level

pytestmark = pytest.mark.gpu

NMAX = max(sr.BLOCK_VEC_SIZES)
LD0 = NMAX + 1                      # even
LS = (1, 7, 8, 9, 17, 64)
LMAX = 64


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def H(capi):
    """a hierarchy for the debug wrapper of the Gram: it takes it for the lock partial sums and indexes nothing of it"""
    return one_level(capi, sr.tri(9), "direct")[1]


class At:
    """n values at an offset (in doubles) inside a device allocation"""

    def __init__(self, base, off, n):
        self.ptr, self.n, self.keep = C.c_void_p(base.ptr.value + 8 * int(off)), int(n), base


_HOST = {}


def host_base():
    """Z (64, LD0), Y and W (NMAX, 8), C (64, 8): made once, read-only"""
    if not _HOST:
        rng = np.random.default_rng(77)
        _HOST.update(Z=rng.standard_normal((LMAX, LD0)), Y=rng.standard_normal((NMAX, 8)), W=rng.standard_normal((NMAX, 8)),
                     C=rng.standard_normal((LMAX, 8)))
        _HOST["C"][5] = 0.0                       # a zero row of coefficients
        for a in _HOST.values():
            a.setflags(write=False)
    return _HOST


@pytest.fixture(scope="module")
def dev_base(capi):
    """the 64 columns on the device, column l at l * LD0, and two allocations the cases are built in (one per leading dimension)"""
    hb = host_base()
    return capi.DeviceVector(LMAX * LD0, hb["Z"].ravel()), capi.DeviceVector(LMAX * (LD0 + 8)), capi.DeviceVector(LMAX * (LD0 + 8))


def lds(n):
    return (n + (n & 1), n + 6 + (n & 1))


def build(capi, dev_base, n, ld, which=1):
    """-> the 64 columns of n rows with leading dimension ld in work allocation `which`, NaN everywhere else"""
    dZ0, dZ = dev_base[0], dev_base[which]
    dZ.fill(float("nan"))
    for l in range(LMAX):
        if n:
            capi.check(capi.lib().sgpu_vec_copy(At(dZ, l * ld, n).ptr, At(dZ0, l * LD0, n).ptr, n))
    return dZ


def columns_back(capi, dZ, n, ld):
    """-> the (64, ld) array behind dZ"""
    out = np.empty(LMAX * ld)
    if LMAX * ld:
        capi.check(capi.lib().sgpu_vec_download(out.ctypes.data, dZ.ptr, LMAX * ld))
    return out.reshape(LMAX, ld)


CHECK_Z_UP_TO = 100003        # the locked columns are const arguments: they are read back and compared up to this size


@pytest.mark.parametrize("n", sr.BLOCK_VEC_SIZES)
def test_lock_gram(capi, H, dev_base, n):
    """entry (l, b): the bits of sgpu_dot on column l of Z and column b of Y -- what tests/test_gpu_eig_kernels.py holds
    k_gram_block_partial's entries to -- for every K, L and ld: an entry depends on neither L, K, the pass it fell in nor ld.  Up to
    513 rows the bits are also those of the numpy restatement.  L K doubles are written and no more; Z and Y are left as they were"""
    hb = host_base()
    Y = hb["Y"][:n]
    dYc = [Padded(capi, Y[:, b]) for b in range(8)]
    want = np.array([[gpu_dot(capi, At(dev_base[0], l * LD0, n), dYc[b]) for b in range(8)] for l in range(LMAX)]) if n else np.zeros((LMAX, 8))
    if n <= 513:
        same_bits(want, lr.lock_gram(hb["Z"][:, :n].T, Y) if n else np.zeros((LMAX, 8)), "sgpu_dot against the restatement")
    for ld in lds(n):
        dZ = build(capi, dev_base, n, ld)
        for K in KS:
            dY = Blk(capi, Y[:, :K])
            for L in LS:
                out = Padded(capi, np.full(L * K, SENTINEL))
                H.debug_lock_gram(dZ, ld, L, dY, n, K, out)
                same_bits(out.head().reshape(L, K), want[:L, :K], (n, ld, K, L))
            same_bits(dY.get(), Y[:, :K])
        if n <= CHECK_Z_UP_TO:
            got = columns_back(capi, dZ, n, ld)
            same_bits(got[:, :n], hb["Z"][:, :n])
            assert np.all(np.isnan(got[:, n:]))


def test_lock_gram_does_not_depend_on_what_the_partials_held(capi, H, dev_base):
    """the partial sums are shared by every pass of every call: 3 rows after a call that filled all 1024 blocks of all 8 passes"""
    hb = host_base()
    K, big, small = 8, sr.BLOCK * sr.N_PARTIALS + 257, 3
    out_b, out_s = Padded(capi, np.full(LMAX * K, SENTINEL)), Padded(capi, np.full(9 * K, SENTINEL))
    dZb = build(capi, dev_base, big, big + 1)
    dYb, dYs = Blk(capi, hb["Y"][:big]), Blk(capi, hb["Y"][:small])
    H.debug_lock_gram(dZb, big + 1, LMAX, dYb, big, K, out_b)
    H.debug_lock_gram(dZb, big + 1, 9, dYs, small, K, out_s)
    got = out_s.head().reshape(9, K).copy()
    assert np.max(np.abs(got - hb["Z"][:9, :small] @ hb["Y"][:small])) <= 1e-13
    H.debug_lock_gram(dZb, big + 1, 9, dYs, small, K, out_s)
    same_bits(out_s.head().reshape(9, K), got)


@pytest.mark.parametrize("n", sr.BLOCK_VEC_SIZES)
def test_lock_project(capi, dev_base, n):
    """bit for bit the numpy restatement -- sum over l ascending of Q[i, l] (-C[l, b]) from 0.0, every product rounded, then added, W
    last -- in place (W is input and output), for every K, L and ld; the restatement's running sum over l IS the result for every
    L, and its first K columns the result for that K (a row's columns do not meet).  Nothing is written past n K; Q and C stay"""
    hb = host_base()
    W8, C8 = hb["W"][:n], hb["C"]
    dC = {K: Padded(capi, np.ascontiguousarray(C8[:, :K]).ravel()) for K in KS}
    dZ = {ld: build(capi, dev_base, n, ld, which) for ld, which in zip(lds(n), (1, 2))}
    dW = {K: Blk(capi, W8[:, :K]) for K in KS}
    run = np.zeros((n, 8))
    for l in range(LMAX):
        run = run + hb["Z"][l, :n][:, None] * (-C8[l:l + 1, :])
        L = l + 1
        if L not in LS:
            continue
        want = run + W8
        if L == 9 and n <= 513:
            same_bits(want, lr.lock_project(hb["Z"][:L, :n].T, C8[:L], W8))
        for ld in lds(n):
            for K in KS:
                dW[K].upload(W8[:, :K])
                capi.lock_project(K, dZ[ld], ld, dC[K], L, dW[K], n)
                same_bits(dW[K].get(), want[:, :K], (n, ld, K, L))
    for K in KS:
        same_bits(dC[K].head(), np.ascontiguousarray(C8[:, :K]).ravel())
    if n <= CHECK_Z_UP_TO:
        for ld in lds(n):
            same_bits(columns_back(capi, dZ[ld], n, ld)[:, :n], hb["Z"][:, :n])


def test_lock_project_propagates_a_nan_as_ieee_says(capi, dev_base):
    """0 * NaN = NaN: a NaN in a locked column poisons its row of W although that column's coefficients are zero, and no other row"""
    hb = host_base()
    n, K, L, ld = 300, 4, 9, 300
    Z = np.array(hb["Z"][:L, :n])
    Z[5, 17] = np.nan                                          # row 5 of C is zero
    dZ, dC, dW = capi.DeviceVector(L * ld, Z.ravel()), Padded(capi, np.ascontiguousarray(hb["C"][:L, :K]).ravel()), Blk(capi, hb["W"][:n, :K])
    capi.lock_project(K, dZ, ld, dC, L, dW, n)
    got = dW.get()
    assert np.all(np.isnan(got[17])) and np.all(np.isfinite(np.delete(got, 17, axis=0)))


@pytest.mark.parametrize("n", sr.BLOCK_VEC_SIZES)
def test_block_refill(capi, n):
    """column col of a block vector becomes the generator's values, bit for bit the numpy restatement, in [-1, 1); the other columns
    and everything past n K stay"""
    for K in KS:
        X = np.full((n, K), SENTINEL)
        dX = Blk(capi, X)
        for col, counter in ((0, 0), (K - 1, 7), (K // 2, 2 ** 32 - 1)):
            capi.block_refill(dX, n, K, col, counter)
            X[:, col] = lr.refill(n, counter)
            same_bits(dX.get(), X, (n, K, col, counter))
            assert np.all(X[:, col] >= -1.0) and np.all(X[:, col] < 1.0)
    if n >= 100003:
        v = lr.refill(n, 3)
        assert abs(v.mean()) < 0.02 and abs(v.std() - 1 / np.sqrt(3)) < 0.02 and len(np.unique(v)) == n


def test_the_lock_wrappers_refuse_what_they_cannot_take(capi, H):
    x = capi.DeviceVector(1024)
    for K, L, ld, n, msg in ((3, 1, 4, 4, "2, 4 or 8"), (4, 0, 4, 4, "L is 1..64"), (4, 65, 4, 4, "L is 1..64"), (4, 1, 5, 4, "ld even"), (4, 1, 2, 4, "ld even")):
        with pytest.raises(capi.SgpuError, match=msg):
            H.debug_lock_gram(x, ld, L, x, n, K, x)
        with pytest.raises(capi.SgpuError, match=msg):
            capi.lock_project(K, x, ld, x, L, x, n)
    with pytest.raises(capi.SgpuError, match="col must be in"):
        capi.block_refill(x, 4, 4, 4, 0)
