"""k_vidx (variant 17): the row-pattern form with the values as 8-bit codes into a dictionary of at most 256 values per workgroup
of 256 rows.  A code decodes to the exact fp64 bit pattern and every row sums in k_sellp's order, so every fused epilogue must be
BIT-IDENTICAL to k_sellp (11) and k_sellp2 (14) -- and to the oracle's sequential loop."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import hierarchy, inputs, util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same_bits(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


def _stencil_like(M, vals, seed=0):
    """a tridiagonal band (one row pattern inside, two at the ends) whose entries take `vals` in turn: entry k gets vals[k % len]"""
    r = np.arange(M)
    rows = np.concatenate([r, r[1:], r[:-1]])
    cols = np.concatenate([r, r[1:] - 1, r[:-1] + 1])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    v = np.asarray(vals, np.float64)[np.arange(len(rows)) % len(vals)]
    return orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), v)


def _every_epilogue(capi, G, A, M, N, square=True):
    """the outputs of every launch form the operator can take: product, residual, Jacobi, Chebyshev (step 0 and k), u -= A e"""
    x, rhs = inputs.v2(N), inputs.rhs2(M)
    dx, dy, dr = capi.DeviceVector(N, x), capi.DeviceVector(M), capi.DeviceVector(M, rhs)
    out = {}
    G.spmv(dx, dy)
    out["spmv"] = dy.download()
    du = capi.DeviceVector(M, rhs)
    G.prolong_correct(dx, du)
    out["sub"] = du.download()
    if square:
        G.residual(dx, dr, dy)
        out["residual"] = dy.download()
        du = capi.DeviceVector(M, x)
        G.jacobi(2, du, dr)
        out["jacobi"] = du.download()
        du = capi.DeviceVector(M, x)
        G.chebyshev(3, 1.9371, du, dr)
        out["chebyshev"] = du.download()
    return out


@pytest.mark.parametrize("name", ["poisson32", "poisson64", "band"])
def test_value_index_bit_identical_to_row_patterns(capi, name, monkeypatch):
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    if name.startswith("poisson"):
        entries, M = orc.laplacian3d(int(name[7:]))
    else:
        M = 5000
        entries = _stencil_like(M, [4.0, -1.25, -0.75, 1.0 / 3.0, 2.5])
    A = orc.OracleOp(entries, M, M, orc.split_even(M, 1))
    x = inputs.v2(M)
    ref = {}
    for v in (11, 14, 17):
        G = util.gpu_operator(A)
        G.set_variant(v)
        if v == 17:
            assert G.variant() == (17, "k_vidx")
        ref[v] = _every_epilogue(capi, G, A, M, M)
    np.testing.assert_array_equal(ref[17]["spmv"], A.matvec(x))
    for k in ref[11]:
        assert_same_bits(ref[17][k], ref[11][k])
        assert_same_bits(ref[17][k], ref[14][k])


def test_value_index_on_a_transfer_operator(capi):
    """P0 / R0 of a small smoothed-aggregation hierarchy (a handful of distinct values; P0's rows repeat relative to their first
    column: the rowbase table), and the V-cycle that restricts with the fused first sweep of the next level (RSWEEP)"""
    As, Ps, Rs = hierarchy.poisson_hierarchy(34, 3)
    OA, OP, OR = hierarchy.oracle_hierarchy(As, Ps, Rs)
    for O in (OP[0], OR[0]):
        M, N = O.Mbig, O.Nbig
        out = {}
        for v in (11, 17):
            G = util.gpu_operator(O)
            G.set_variant(v)
            if v == 17:
                assert G.variant()[1].startswith("k_vidx")
            out[v] = _every_epilogue(capi, G, O, M, N, square=False)
        np.testing.assert_array_equal(out[17]["spmv"], O.matvec(inputs.v2(N)))
        for k in out[11]:
            assert_same_bits(out[17][k], out[11][k])
    eig = hierarchy.eig_estimates(As)
    res = {}
    for v in (11, 17):
        GA = [util.gpu_operator(a) for a in OA]
        GP = [util.gpu_operator(p) for p in OP]
        GR = [util.gpu_operator(r) for r in OR]
        for op in GA[:1] + GP[:1] + GR[:1]:
            op.set_variant(v)
        for smoother in ("jacobi", "chebyshev"):
            G = capi.Amg(GA, GP, GR, eig_max=eig, pre=2, post=2, smoother=smoother, coarse_solver="direct")
            n = OA[0].Mbig
            du, dr = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, inputs.rhs2(n))
            G.vcycle(du, dr)
            res[(v, smoother)] = du.download()
            G.destroy()
    for smoother in ("jacobi", "chebyshev"):
        assert_same_bits(res[(17, smoother)], res[(11, smoother)])


def test_more_than_256_distinct_values_are_refused(capi):
    """256 distinct values in a workgroup of 256 rows: served, bit-identical; 257: refused.  Values count as BIT PATTERNS: +0.0 and
    -0.0 are two values, and so are two NaNs with different payloads."""
    M = 600
    base = [1.0 + k / 1024.0 for k in range(254)]
    ok = _stencil_like(M, base + [0.0, 5.0])
    A = orc.OracleOp(ok, M, M, orc.split_even(M, 1), orc.split_even(M, 1), square=False)     # (no inverse diagonal: zeros on it)
    G = util.gpu_operator(A)
    G.set_variant(17)
    x = inputs.v2(M)
    dx, dy = capi.DeviceVector(M, x), capi.DeviceVector(M)
    G.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), A.matvec(x))
    nan1 = np.array([0x7ff8000000000001], np.uint64).view(np.float64)[0]
    nan2 = np.array([0x7ff8000000000002], np.uint64).view(np.float64)[0]
    for extra in ([0.0, -0.0, 5.0], [nan1, nan2, 5.0], [k + 2000.0 for k in range(3)]):
        A2 = orc.OracleOp(_stencil_like(M, base + extra), M, M, orc.split_even(M, 1), orc.split_even(M, 1), square=False)
        G2 = util.gpu_operator(A2)
        with pytest.raises(capi.SgpuError, match="value-indexed"):
            G2.set_variant(17)
        G2.set_variant(11)                                   # (the form without codes still serves it)


def test_signed_zeros_infinities_and_nans_keep_their_bits(capi):
    """+-0.0, +-Inf and NaNs with payloads (including the all-ones pattern, the build's empty-slot key) decode to their own bits:
    the products come out as k_sellp's, bit for bit"""
    M = 3000
    specials = np.array([0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000123,
                         0xfff8000000000456, 0xffffffffffffffff, 0x3ff8000000000000], np.uint64).view(np.float64)
    vals = [1.5, -2.25, 3.0] * 40 + list(specials)
    A = orc.OracleOp(_stencil_like(M, vals), M, M, orc.split_even(M, 1), orc.split_even(M, 1), square=False)
    out = {}
    for v in (11, 17):
        G = util.gpu_operator(A)
        G.set_variant(v)
        out[v] = _every_epilogue(capi, G, A, M, M, square=False)
    for k in out[11]:
        assert_same_bits(out[17][k], out[11][k])
    assert np.isnan(out[17]["spmv"]).any() and np.isinf(out[17]["spmv"]).any()


@pytest.mark.parametrize("nprocs", [2, 3])
def test_value_index_with_emulated_halos(capi, nprocs, monkeypatch):
    """several ranks on one device: the interior launch masks the boundary rows (HALO); k_vidx gives k_sellp's bits on every rank"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    entries, M = orc.laplacian3d(20)
    split = orc.split_nnz(entries, M, nprocs)
    A = orc.OracleOp(entries, M, M, split)
    W = util.EmulatedWorld(A)
    x, rhs = inputs.v2(M), inputs.rhs2(M)
    out = {}
    for variant in (11, 17):
        xs, ys, rs, us = W.slices(x, split), W.slices(np.zeros(M), split), W.slices(rhs, split), W.slices(x, split)
        W.exchange(xs); W.exchange(us)
        for r in range(nprocs):
            W.g[r].set_variant(variant); W.g[r].set_lanes_per_row(1)
            if variant == 17:
                assert W.g[r].variant() == (17, "k_vidx")
            W.g[r].spmv(xs[r], ys[r])
            W.g[r].jacobi(1, us[r], rs[r])
        out[variant] = (W.gather(ys), W.gather(us))
    assert_same_bits(out[17][0], out[11][0])
    assert_same_bits(out[17][1], out[11][1])


def test_autotune_offers_and_opt_out(capi, monkeypatch):
    """the autotune times k_vidx next to the other forms where the values exceed the L2s (32 MiB; timing alone decides among them);
    SAENA_NO_VALUE_INDEX=1 leaves it out"""
    monkeypatch.setenv("SAENA_PLAN_CACHE", "off")
    entries, M = orc.laplacian3d(100)                       # 941 192 rows, 6.5 M entries: 52 MB of values
    A = orc.OracleOp(entries, M, M, orc.split_even(M, 1))
    x = inputs.v2(M)
    dx, dy = capi.DeviceVector(M, x), capi.DeviceVector(M)
    G = util.gpu_operator(A)
    G.autotune()
    assert G.variant()[1] in ("k_sellp", "k_sellp2", "k_vidx")   # the forms with the sequential row sum
    G.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), A.matvec(x))
    monkeypatch.setenv("SAENA_NO_VALUE_INDEX", "1")
    G2 = util.gpu_operator(A)
    G2.autotune()
    assert G2.variant()[0] != 17
    G2.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), A.matvec(x))
