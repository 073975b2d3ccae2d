"""The x-window launch mode of k_vidx (variant 17 + set_x_windows(R)): a workgroup of R rows stages the windows of x its rows reach
in LDS and gathers from there.  The stored operator, the products and the sequential row sums are k_vidx's, so every fused
epilogue must be BIT-IDENTICAL to k_sellp (variant 11) -- and the product to the oracle's sequential loop -- at every R."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import hierarchy, inputs, util

pytestmark = pytest.mark.gpu

ROWS = (256, 512, 1024)


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same_bits(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


def _stencil_like(M, vals):
    """a tridiagonal band (one row pattern inside, two at the ends) whose entries take `vals` in turn: entry k gets vals[k % len]"""
    r = np.arange(M)
    rows = np.concatenate([r, r[1:], r[:-1]])
    cols = np.concatenate([r, r[1:] - 1, r[:-1] + 1])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    v = np.asarray(vals, np.float64)[np.arange(len(rows)) % len(vals)]
    return orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), v)


def _diagonals(M, offsets, vals):
    """the diagonals at `offsets` of an M x M operator, entry k taking vals[k % len]"""
    r = np.arange(M)
    rows = np.concatenate([r[(r + o >= 0) & (r + o < M)] for o in offsets])
    cols = np.concatenate([r[(r + o >= 0) & (r + o < M)] + o for o in offsets])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    v = np.asarray(vals, np.float64)[np.arange(len(rows)) % len(vals)]
    return orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), v)


def _every_epilogue(capi, G, M, N, x, rhs, square=True):
    """the outputs of every launch form the operator can take: product, residual, Jacobi, Chebyshev (step 0 and k), u -= A e"""
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


_SPECIALS = np.array([0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000123,
                      0xfff8000000000456, 0xffffffffffffffff, 0x3ff8000000000000], np.uint64).view(np.float64)


def _case(name):
    """-> (OracleOp, M, square, x): built once per module"""
    if name in _CASES:
        return _CASES[name]
    x = None
    if name.startswith("poisson"):
        entries, M = orc.laplacian3d(int(name[7:]))
        A, square = orc.OracleOp(entries, M, M, orc.split_even(M, 1)), True
    elif name == "band5":
        M = 5000
        A, square = orc.OracleOp(_stencil_like(M, [4.0, -1.25, -0.75, 1.0 / 3.0, 2.5]), M, M, orc.split_even(M, 1)), True
    elif name == "band256":                     # 254 + 2 distinct values: dictionaries of about 250 entries, two to four per workgroup of 512 / 1024 rows
        M = 3000
        vals = [1.0 + k / 1024.0 for k in range(254)] + [0.0, 5.0]
        A, square = orc.OracleOp(_stencil_like(M, vals), M, M, orc.split_even(M, 1), orc.split_even(M, 1), square=False), False
    elif name == "specials":                    # +-0.0, +-Inf, NaNs with payloads among the values; +-Inf and NaN at a dozen positions of x
        M = 3000
        vals = [1.5, -2.25, 3.0] * 40 + list(_SPECIALS)
        A, square = orc.OracleOp(_stencil_like(M, vals), M, M, orc.split_even(M, 1), orc.split_even(M, 1), square=False), False
        x = inputs.v2(M).copy()
        at = [0, 1, 255, 256, 511, 512, 1023, 1024, 1500, 2047, 2998, 2999]
        x[at] = [np.inf, -np.inf, np.nan, np.inf, -np.inf, _SPECIALS[4], np.inf, _SPECIALS[5], -np.inf, np.nan, np.inf, -np.inf]
    else:
        raise KeyError(name)
    if x is None:
        x = inputs.v2(M)
    _CASES[name] = (A, M, square, x)
    return _CASES[name]


_CASES = {}
_REF = {}


def _reference(capi, name):
    """variant 11's outputs on the case's inputs, computed once and left unchanged"""
    if name not in _REF:
        A, M, square, x = _case(name)
        G = util.gpu_operator(A)
        G.set_variant(11)
        _REF[name] = _every_epilogue(capi, G, M, M, x, inputs.rhs2(M), square)
        for v in _REF[name].values():
            v.setflags(write=False)
    return _REF[name]


# poisson12: 1 000 rows, all offsets in one window, one partial workgroup; poisson35: 35 937 rows (no multiple of 64), n = 33 and
# n^2 = 1 089: three windows at every R, those of the first and last workgroups leave the vector at both ends
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", ["poisson12", "poisson35", "band5", "band256", "specials"])
def test_x_windows_bit_identical_to_row_patterns(capi, name, rows, monkeypatch):
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    A, M, square, x = _case(name)
    ref = _reference(capi, name)
    G = util.gpu_operator(A)
    G.set_variant(17)
    assert G.x_windows() == 0                                # variant 17 alone: direct gathers
    G.set_x_windows(rows)
    assert G.x_windows() == rows
    assert G.variant() == (17, "k_vidx")                     # a launch mode, not a variant of its own
    out = _every_epilogue(capi, G, M, M, x, inputs.rhs2(M), square)
    for k in ref:
        assert_same_bits(out[k], ref[k])
    if name == "specials":
        assert np.isnan(out["spmv"]).any() and np.isinf(out["spmv"]).any()
    else:
        np.testing.assert_array_equal(out["spmv"], A.matvec(x))
    G.set_x_windows(0)                                       # and back: the direct gathers of the same operator
    assert G.x_windows() == 0
    dx, dy = capi.DeviceVector(M, x), capi.DeviceVector(M)
    G.spmv(dx, dy)
    assert_same_bits(dy.download(), ref["spmv"])


_HALO_REF = {}


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nprocs", [2, 3])
def test_x_windows_with_emulated_halos(capi, nprocs, rows, monkeypatch):
    """several ranks on one device: the interior launch masks the boundary rows (HALO); the window mode gives k_sellp's bits"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    entries, M = orc.laplacian3d(20)
    split = orc.split_nnz(entries, M, nprocs)
    A = orc.OracleOp(entries, M, M, split)
    W = util.EmulatedWorld(A)
    x, rhs = inputs.v2(M), inputs.rhs2(M)

    def run(variant):
        xs, ys, rs, us = W.slices(x, split), W.slices(np.zeros(M), split), W.slices(rhs, split), W.slices(x, split)
        W.exchange(xs); W.exchange(us)
        for r in range(nprocs):
            W.g[r].set_variant(variant); W.g[r].set_lanes_per_row(1)
            if variant == 17:
                W.g[r].set_x_windows(rows)
                assert W.g[r].x_windows() == rows and W.g[r].variant() == (17, "k_vidx")
            W.g[r].spmv(xs[r], ys[r])
            W.g[r].jacobi(1, us[r], rs[r])
        return W.gather(ys), W.gather(us)

    if nprocs not in _HALO_REF:
        _HALO_REF[nprocs] = run(11)
    got = run(17)
    assert_same_bits(got[0], _HALO_REF[nprocs][0])
    assert_same_bits(got[1], _HALO_REF[nprocs][1])


def test_x_windows_refused_on_the_rowbase_table(capi):
    """P0 of a small smoothed-aggregation hierarchy: its patterns are relative to the rows' first columns"""
    As, Ps, Rs = hierarchy.poisson_hierarchy(34, 3)
    OA, OP, OR = hierarchy.oracle_hierarchy(As, Ps, Rs)
    O = OP[0]
    M, N = O.Mbig, O.Nbig
    G = util.gpu_operator(O)
    G.set_variant(17)
    assert G.variant()[1] == "k_vidx<rowbase>"
    for rows in ROWS:
        with pytest.raises(capi.SgpuError, match="x windows"):
            G.set_x_windows(rows)
        assert G.x_windows() == 0
    x = inputs.v2(N)
    dx, dy = capi.DeviceVector(N, x), capi.DeviceVector(M)
    G.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), O.matvec(x))


def test_x_windows_refused_beyond_sixteen_windows(capi):
    """the diagonal and 20 more diagonals 1 500 columns apart: 21 windows at every R"""
    M = 20000
    A = orc.OracleOp(_diagonals(M, [1500 * k for k in range(-10, 11)], [4.0, -1.25, -0.75, 2.5]), M, M,
                     orc.split_even(M, 1), orc.split_even(M, 1), square=False)
    G = util.gpu_operator(A)
    G.set_variant(17)
    for rows in ROWS:
        with pytest.raises(capi.SgpuError, match="x windows"):
            G.set_x_windows(rows)
        assert G.x_windows() == 0
    assert G.variant() == (17, "k_vidx")
    x = inputs.v2(M)
    dx, dy = capi.DeviceVector(M, x), capi.DeviceVector(M)
    G.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), A.matvec(x))


def test_x_windows_need_variant_17(capi):
    entries, M = orc.laplacian3d(12)
    G = util.gpu_operator(orc.OracleOp(entries, M, M, orc.split_even(M, 1)))
    G.set_variant(11)
    with pytest.raises(capi.SgpuError, match="x windows"):
        G.set_x_windows(512)
    G.set_variant(17)
    with pytest.raises(capi.SgpuError, match="x windows"):
        G.set_x_windows(384)                                 # not a workgroup size of the mode
    G.set_x_windows(512)
    G.set_variant(17)                                        # setting the variant again selects direct gathers
    assert G.x_windows() == 0


def test_autotune_times_the_mode_and_opt_out(capi, monkeypatch):
    """wherever the autotune offers 17 it also times 17 with windows; whichever candidate wins, the product is the oracle's;
    SAENA_NO_X_WINDOWS=1 leaves the mode out"""
    monkeypatch.setenv("SAENA_PLAN_CACHE", "off")
    entries, M = orc.laplacian3d(100)                       # 941 192 rows, 6.5 M entries
    A = orc.OracleOp(entries, M, M, orc.split_even(M, 1))
    x = inputs.v2(M)
    want = A.matvec(x)
    dx, dy = capi.DeviceVector(M, x), capi.DeviceVector(M)
    G = util.gpu_operator(A)
    G.autotune()
    v, name = G.variant()
    assert name in ("k_sellp", "k_sellp2", "k_vidx")
    assert G.x_windows() in (0,) + ROWS and (v == 17 or G.x_windows() == 0)
    G.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), want)
    monkeypatch.setenv("SAENA_NO_X_WINDOWS", "1")
    G2 = util.gpu_operator(A)
    G2.autotune()
    assert G2.x_windows() == 0
    G2.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), want)
