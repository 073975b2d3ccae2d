"""The three tall-skinny kernels of sgpu_eigs_LOBPCG on the GPU (saena_amd/csrc/kernels_eig.hip.h), held to their written contracts
through sgpu_debug_block_gram / _block_mix / _eig_residual, which run the solver's own launch helpers on the caller's arrays.

Block vectors are staged as in tests/test_gpu_block_solver_layer.py: host.ravel() of an (n, K) C-ordered array is X[i * K + j], in
an allocation of n K + 8 doubles whose tail holds the NaN sentinel.  Sizes are solver_ref.BLOCK_VEC_SIZES: 0, 1, 2, 3, wave and
block edges, 262145 rows and more (the second grid-stride trip of the Gram and residual kernels, which run on the dot's grid of at
most 1024 blocks) and 524289 and more (the mix kernel's, at most 2048 blocks of one row per thread).
"""
import numpy as np
import pytest

from tests import eig_ref as er, solver_ref as sr
from tests.test_gpu_block_solver_layer import KS, Blk, same_bits
from tests.test_gpu_solver_layer import SENTINEL, SENTINEL_BITS, Padded, bits, gpu_dot, one_level

pytestmark = pytest.mark.gpu

NMAX = max(sr.BLOCK_VEC_SIZES)


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def H(capi):
    """a hierarchy for the debug wrappers: they take it for its per-K partial sums and index nothing of it"""
    return one_level(capi, sr.tri(9), "direct")[1]


_BASE = {}


def base(k):
    """four (NMAX, 8) standard normal arrays, made once; a test takes the first n rows and K columns"""
    if not _BASE:
        rng = np.random.default_rng(2024)
        for i in range(4):
            _BASE[i] = rng.standard_normal((NMAX, 8))
            _BASE[i].setflags(write=False)
    return _BASE[k]


# ---------------------------------------------------------------------------
# the Gram block
@pytest.mark.parametrize("n", sr.BLOCK_VEC_SIZES)
def test_block_gram(capi, H, n):
    """entry (a, b): the bits of sgpu_dot on column a of X and column b of Y -- hence within dot_bound of the longdouble sum (asserted
    directly on the diagonal and the two corners) and the same at K = 2, 4 and 8; X == Y gives a bit-symmetric result with the bits of
    the scalar dots; K^2 doubles are written and no more"""
    if n == 0:
        for K in KS:
            e, out = Blk(capi, np.zeros((0, K))), Padded(capi, np.full(K * K, SENTINEL))
            H.debug_block_gram(e, e, 0, K, out)
            assert np.all(bits(out.head()) == bits(0.0))
        return
    for kind in ("normal", "cancelling"):
        xy = [sr.dot_inputs(n, kind, seed=j) for j in range(8)]
        X, Y = np.stack([x for x, _ in xy], axis=1), np.stack([y for _, y in xy], axis=1)
        cx, cy = [Padded(capi, X[:, j]) for j in range(8)], [Padded(capi, Y[:, j]) for j in range(8)]
        scalar = np.array([[gpu_dot(capi, cx[a], cy[b]) for b in range(8)] for a in range(8)])
        scalar_xx = np.array([[gpu_dot(capi, cx[a], cx[b]) for b in range(8)] for a in range(8)])
        for a, b in [(j, j) for j in range(8)] + [(0, 7), (7, 0)]:
            err = abs(float(np.longdouble(scalar[a, b]) - sr.dot_hp(X[:, a], Y[:, b])))
            assert err <= sr.dot_bound(X[:, a], Y[:, b]), (kind, a, b, err)
        for K in KS:
            dX, dY, out = Blk(capi, X[:, :K]), Blk(capi, Y[:, :K]), Padded(capi, np.full(K * K, SENTINEL))
            H.debug_block_gram(dX, dY, n, K, out)
            got = out.head().reshape(K, K).copy()
            same_bits(got, scalar[:K, :K], (kind, K))
            H.debug_block_gram(dX, dY, n, K, out)
            same_bits(out.head().reshape(K, K), got, "not reproducible")
            H.debug_block_gram(dX, dX, n, K, out)
            sym = out.head().reshape(K, K)
            same_bits(sym, sym.T, (kind, K, "X == Y is not bit-symmetric"))
            same_bits(sym, scalar_xx[:K, :K], (kind, K, "X == Y"))
            same_bits(dX.get(), X[:, :K]); same_bits(dY.get(), Y[:, :K])


def test_block_gram_does_not_depend_on_what_the_partials_held(capi, H):
    """the partial sums are shared by every Gram block of a hierarchy: a 3-row block after one that filled all 1024 blocks, and back"""
    K, big, small = 8, sr.BLOCK * sr.N_PARTIALS + 257, 3
    Xb, Yb, Xs, Ys = base(0)[:big, :K], base(1)[:big, :K], base(2)[:small, :K], base(3)[:small, :K]
    dXb, dYb, dXs, dYs = (Blk(capi, a) for a in (Xb, Yb, Xs, Ys))
    out = Padded(capi, np.full(K * K, SENTINEL))

    def gram(x, y, n):
        H.debug_block_gram(x, y, n, K, out)
        return out.head().copy()
    ws, wb = gram(dXs, dYs, small), gram(dXb, dYb, big)
    same_bits(gram(dXs, dYs, small), ws)
    same_bits(gram(dXb, dYb, big), wb)
    assert np.max(np.abs(ws.reshape(K, K) - Xs.T @ Ys)) <= 1e-13


def test_gram_and_residual_refuse_what_they_cannot_take(capi, H):
    x = capi.DeviceVector(64)
    with pytest.raises(capi.SgpuError, match="2, 4 or 8"):
        H.debug_block_gram(x, x, 4, 3, x)
    with pytest.raises(capi.SgpuError, match="1 to 3 sources"):
        capi.check(capi.lib().sgpu_debug_block_mix(4, 4, x.ptr, x.ptr, x.ptr, x.ptr, x.ptr, x.ptr, None, x.ptr, 4))


# ---------------------------------------------------------------------------
# the mix
def coefs(K, ns, zero_rows):
    rng = np.random.default_rng(100 * K + ns)
    Cm = [rng.standard_normal((K, K)) for _ in range(ns)]
    for c in Cm:
        c[list(zero_rows)] = 0.0
    return Cm


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", sr.BLOCK_VEC_SIZES)
def test_block_mix(capi, n, K):
    """bit for bit the numpy restatement (sources in argument order, a ascending, product rounded then added, from 0.0; Add last) for
    NS = 1, 2, 3: into a separate output, in place of every source, and in place of Add; zero rows in C; sources and coefficients
    are left as they were and nothing is written past n K.  NS = 1 and 2 are the instantiations the solver launches; every one runs at
    every size, the second grid-stride trip (n > 524288) included.  Past 1000 rows the output takes the place of the last source and of
    Add only (which source it replaces changes no address arithmetic)"""
    S = [base(i)[:n, :K] for i in range(3)]
    add = base(3)[:n, :K]
    for ns in (1, 2, 3):
        Cm = coefs(K, ns, zero_rows=(1,) if ns != 2 else ())
        dC = [Padded(capi, c.ravel()) for c in Cm]
        want = er.block_mix(S[:ns], Cm)
        want_add = er.block_mix(S[:ns], Cm, add=add)
        dS = [Blk(capi, s) for s in S[:ns]]
        dAdd, out = Blk(capi, add), Blk(capi, np.full((n, K), SENTINEL))
        capi.block_mix(K, dS, dC, out, n)
        same_bits(out.get(), want, (K, ns, "separate output"))
        out.upload(np.full((n, K), SENTINEL))
        capi.block_mix(K, dS, dC, out, n, add=dAdd)
        same_bits(out.get(), want_add, (K, ns, "separate output, Add"))
        for s in range(ns):
            same_bits(dS[s].get(), S[s])
        same_bits(dAdd.get(), add)
        for s in (range(ns) if n <= 1000 else (ns - 1,)):       # in place of source s
            capi.block_mix(K, dS, dC, dS[s], n, add=dAdd)
            same_bits(dS[s].get(), want_add, (K, ns, "aliased with source", s))
            dS[s].upload(S[s])
        capi.block_mix(K, dS, dC, dAdd, n, add=dAdd)          # in place of Add
        same_bits(dAdd.get(), want_add, (K, ns, "aliased with Add"))
        for c, d in zip(Cm, dC):
            same_bits(d.head(), c.ravel())


@pytest.mark.parametrize("K", KS)
def test_block_mix_propagates_a_nan_as_ieee_says(capi, K):
    """0 * NaN = NaN: a NaN in column 1 of a source poisons its whole output row although row 1 of C is zero, and no other row.  So
    the columns LOBPCG leaves out of a mix must hold finite values, not be skipped: the solver zero-fills them (a zero column of T
    gives an exactly zero output column, asserted here; tests/test_gpu_eig.py checks the solver's own vectors)"""
    n = 300
    S, Cm = np.array(base(0)[:n, :K]), coefs(K, 1, zero_rows=(1,))
    S[17, 1] = np.nan
    dS, out = Blk(capi, S), Blk(capi, np.full((n, K), SENTINEL))
    dC = [Padded(capi, Cm[0].ravel())]
    capi.block_mix(K, [dS], dC, out, n)
    got = out.get()
    assert np.all(np.isnan(got[17])) and np.all(np.isfinite(np.delete(got, 17, axis=0)))
    same_bits(np.delete(got, 17, axis=0), np.delete(er.block_mix([S], Cm), 17, axis=0))
    T = Cm[0].copy()
    T[:, 0] = 0.0                                                 # column 0 is inactive: a zero column of T
    dS.upload(base(0)[:n, :K])
    dC = [Padded(capi, T.ravel())]
    capi.block_mix(K, [dS], dC, dS, n)
    got = dS.get()
    assert np.all(bits(got[:, 0]) == bits(0.0)), "an inactive column is not zero-filled"
    same_bits(got, er.block_mix([base(0)[:n, :K]], [T]))


# ---------------------------------------------------------------------------
# the residual
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", sr.BLOCK_VEC_SIZES)
def test_eig_residual(capi, H, n, K):
    """R: the bits of AX - X diag(lambda) with the product rounded; ||r_j||^2: the bits of the block dot of R with itself, within
    dot_bound of the longdouble sum; AX, X and lambda are read only, nothing is written past R or the K norms"""
    AX, X = base(0)[:n, :K], base(1)[:n, :K]
    lam = np.array([0.5, -1.25, 3.0, 1e-3, 7.5, 2.0, -0.0, 11.0])[:K]
    dAX, dX, dR = Blk(capi, AX), Blk(capi, X), Blk(capi, np.full((n, K), SENTINEL))
    dl, rr, rr2 = Padded(capi, lam), Padded(capi, np.full(K, SENTINEL)), Padded(capi, np.full(K, SENTINEL))
    H.debug_eig_residual(dAX, dX, dl, dR, n, K, rr)
    want = er.eig_residual(AX, X, lam)
    same_bits(dR.get(), want, K)
    H.debug_block_dot(dR, dR, n, K, (1 << K) - 1, rr2)
    got = rr.head()
    same_bits(got, rr2.head(), (K, "norms"))
    for j in range(min(K, 2)):
        assert abs(float(np.longdouble(got[j]) - sr.dot_hp(want[:, j], want[:, j]))) <= sr.dot_bound(want[:, j], want[:, j])
    same_bits(dAX.get(), AX); same_bits(dX.get(), X); same_bits(dl.head(), lam)
    assert SENTINEL_BITS not in bits(got)
