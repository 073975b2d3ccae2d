"""k_geig_residual on the GPU (saena_amd/csrc/kernels_eig.hip.h), held to its written contract through sgpu_debug_geig_residual, which
runs the generalised solver's own launch helper on the caller's arrays: R has the bits of k_eig_residual called with BX in X's place,
and both norms -- formed in the same pass -- have the bits of the block dot of R with R and of BX with BX.

Block vectors are staged as in tests/test_gpu_eig_kernels.py; the sizes are solver_ref.BLOCK_VEC_SIZES: 0, 1, 2, 3, wave and block
edges, odd sizes, and one row past each grid-stride threshold (the kernel runs on the dot's grid of at most 1024 blocks, so its second
trip starts at row 262144): the places a norm's partial sum can go wrong.
"""
import numpy as np
import pytest

from tests import geig_ref as gg, solver_ref as sr
from tests.test_gpu_block_solver_layer import KS, Blk, same_bits
from tests.test_gpu_eig_kernels import base
from tests.test_gpu_solver_layer import SENTINEL, SENTINEL_BITS, Padded, bits, one_level

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def H(capi):
    """a hierarchy for the debug wrappers: they take it for its per-K partial sums and index nothing of it"""
    return one_level(capi, sr.tri(9), "direct")[1]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", sr.BLOCK_VEC_SIZES)
def test_geig_residual(capi, H, n, K):
    """R: the bits of the numpy restatement AX - BX diag(lambda) (product rounded, then subtracted) and of sgpu_debug_eig_residual with
    BX passed as X; ||r_j||^2: the bits of the block dot of (R, R) and of sgpu_debug_eig_residual's norms; ||(BX)_j||^2: the bits of
    the block dot of (BX, BX); both within dot_bound of the longdouble sums; AX, BX and lambda are read only; nothing is written past
    R or past either set of K norms; a second run reproduces every bit"""
    AX, BX = base(0)[:n, :K], base(1)[:n, :K]
    lam = np.array([0.5, -1.25, 3.0, 1e-3, 7.5, 2.0, -0.0, 11.0])[:K]
    dAX, dBX = Blk(capi, AX), Blk(capi, BX)
    dR, dR2 = Blk(capi, np.full((n, K), SENTINEL)), Blk(capi, np.full((n, K), SENTINEL))
    dl = Padded(capi, lam)
    rr, bb, rr_dot, bb_dot, rr_std = (Padded(capi, np.full(K, SENTINEL)) for _ in range(5))
    H.debug_geig_residual(dAX, dBX, dl, dR, n, K, rr, bb)
    want, _, _ = gg.geig_residual(AX, BX, lam)
    R = dR.get().copy()
    same_bits(R, want, (K, "R against the restatement"))
    got_rr, got_bb = rr.head().copy(), bb.head().copy()
    assert SENTINEL_BITS not in bits(got_rr) and SENTINEL_BITS not in bits(got_bb)
    H.debug_block_dot(dR, dR, n, K, (1 << K) - 1, rr_dot)
    same_bits(got_rr, rr_dot.head(), (K, "||r||^2 against the block dot of (R, R)"))
    H.debug_block_dot(dBX, dBX, n, K, (1 << K) - 1, bb_dot)
    same_bits(got_bb, bb_dot.head(), (K, "||Bx||^2 against the block dot of (BX, BX)"))
    H.debug_eig_residual(dAX, dBX, dl, dR2, n, K, rr_std)
    same_bits(R, dR2.get(), (K, "R against sgpu_debug_eig_residual with BX as X"))
    same_bits(got_rr, rr_std.head(), (K, "||r||^2 against sgpu_debug_eig_residual"))
    for j in range(min(K, 2)):
        assert abs(float(np.longdouble(got_rr[j]) - sr.dot_hp(want[:, j], want[:, j]))) <= sr.dot_bound(want[:, j], want[:, j])
        assert abs(float(np.longdouble(got_bb[j]) - sr.dot_hp(BX[:, j], BX[:, j]))) <= sr.dot_bound(BX[:, j], BX[:, j])
    if n == 0:
        assert np.all(bits(got_rr) == bits(0.0)) and np.all(bits(got_bb) == bits(0.0))
    same_bits(dAX.get(), AX); same_bits(dBX.get(), BX); same_bits(dl.head(), lam)
    dR.upload(np.full((n, K), SENTINEL))
    H.debug_geig_residual(dAX, dBX, dl, dR, n, K, rr, bb)
    same_bits(dR.get(), R, "not reproducible"); same_bits(rr.head(), got_rr); same_bits(bb.head(), got_bb)


def test_geig_residual_does_not_depend_on_what_the_partials_held(capi, H):
    """both sets of partial sums are shared by every call on a hierarchy: 3 rows after a call that filled all 1024 blocks, and back"""
    K, big, small = 8, sr.BLOCK * sr.N_PARTIALS + 257, 3
    lam = Padded(capi, np.linspace(0.5, 4.0, K))

    def run(n):
        dAX, dBX, dR = Blk(capi, base(0)[:n, :K]), Blk(capi, base(1)[:n, :K]), Blk(capi, np.full((n, K), SENTINEL))
        rr, bb = Padded(capi, np.full(K, SENTINEL)), Padded(capi, np.full(K, SENTINEL))
        H.debug_geig_residual(dAX, dBX, lam, dR, n, K, rr, bb)
        return rr.head().copy(), bb.head().copy()
    s0, b0 = run(small), run(big)
    s1, b1 = run(small), run(big)
    for a, b in ((s0, s1), (b0, b1)):
        same_bits(a[0], b[0]); same_bits(a[1], b[1])
    assert np.max(np.abs(s0[1] - np.sum(base(1)[:small, :K] ** 2, axis=0))) <= 1e-13


def test_geig_residual_refuses_what_it_cannot_take(capi, H):
    x = capi.DeviceVector(64)
    with pytest.raises(capi.SgpuError, match="2, 4 or 8"):
        H.debug_geig_residual(x, x, x, x, 4, 3, x, x)
    with pytest.raises(capi.SgpuError, match="null argument"):
        capi.check(capi.lib().sgpu_debug_geig_residual(H.h, x.ptr, None, x.ptr, x.ptr, 4, 4, x.ptr, x.ptr))
