"""The x-window launch mode of k_vidx (variant 17 + set_x_windows(R)): a workgroup of R rows stages the windows of x its rows reach
in LDS and gathers from there.  The stored operator, the products and the sequential row sums are k_vidx's, so every fused
epilogue must be BIT-IDENTICAL to k_sellp (variant 11) -- and the product to the oracle's sequential loop -- at every R.

The named operators of tests/xwin_ref.py reach every branch of k_vidxw and of build_xwin (rows of more than 8 entries, slices of
two widths, 4 to 16 windows, several staging passes, the gap rule at its edge, ncols != nrows, the LDS cap); the geometry the
library reports for them is held to that restatement, so the kernel's paths cannot drift out from under the tests."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc
from tests import hierarchy, inputs, util
from tests import xwin_ref as X

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


def _with_values(rows, cols, vals):
    """row-major entries (columns ascending), entry k taking vals[k % len]"""
    v = np.asarray(vals, np.float64)[np.arange(len(rows)) % len(vals)]
    return orc.coo_from_arrays(np.asarray(rows, np.int32), np.asarray(cols, np.int32), v)


def _diagonals(M, offsets, vals, N=None, rows=None):
    """the diagonals at `offsets` of an M x N operator (N = M unless given) over the rows [rows[0], rows[1]) (all unless given),
    entry k taking vals[k % len]"""
    N = M if N is None else N
    r = np.arange(*(rows or (0, M)))
    rr = np.concatenate([r[(r + o >= 0) & (r + o < N)] for o in offsets])
    cc = np.concatenate([r[(r + o >= 0) & (r + o < N)] + o for o in offsets])
    order = np.lexsort((cc, rr))
    return _with_values(rr[order], cc[order], vals)


def _every_epilogue(capi, G, M, N, x, rhs, square=True):
    """the outputs of every launch form the operator can take: product, residual (plain, negated, scaled by c w), Jacobi, Chebyshev
    (step 0 and k), u -= A e"""
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
        G.residual_negative(dx, dr, dy)
        out["residual_negative"] = dy.download()
        G.residual_multiply(dx, dr, dy, capi.DeviceVector(M, inputs.v_sin(M) + 2.0), 0.37)      # (w and c of test_gpu_forms.vectors)
        out["residual_multiply"] = dy.download()
        du = capi.DeviceVector(M, x)
        G.jacobi(2, du, dr)
        out["jacobi"] = du.download()
        du = capi.DeviceVector(M, x)
        G.chebyshev(3, 1.9371, du, dr)
        out["chebyshev"] = du.download()
    return out


_SPECIALS = np.array([0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000123,
                      0xfff8000000000456, 0xffffffffffffffff, 0x3ff8000000000000], np.uint64).view(np.float64)


VALS5 = [4.0, -1.25, -0.75, 1.0 / 3.0, 2.5]
VALS256 = [1.0 + k / 1024.0 for k in range(254)] + [0.0, 5.0]     # 254 + 2 distinct values: dictionaries of about 250 entries
VALS_SPECIAL = [1.5, -2.25, 3.0] * 40 + list(_SPECIALS)           # +-0.0, +-Inf, NaNs with payloads among the values


def _special_x(n, extra):
    """+-Inf and NaN at the first and last element, at R - 1 and R for each R, and at `extra`"""
    x = inputs.v2(n).copy()
    at = [0, n - 1] + [c for R in ROWS for c in (R - 1, R)] + list(extra)
    s = [np.inf, -np.inf, np.nan, _SPECIALS[4], _SPECIALS[5]]
    x[at] = [s[k % len(s)] for k in range(len(at))]
    return x


def _case(name):
    """-> (OracleOp, M, N, square, x): built once per module.  "name.suffix": the named operator of tests/xwin_ref.py with other values"""
    if name in _CASES:
        return _CASES[name]
    x = None
    if name.startswith("poisson"):
        entries, M = orc.laplacian3d(int(name[7:]))
        A, N, square = orc.OracleOp(entries, M, M, orc.split_even(M, 1)), M, True
    elif name == "band5":
        M = N = 5000
        A, square = orc.OracleOp(_stencil_like(M, VALS5), M, M, orc.split_even(M, 1)), True
    elif name == "band256":                     # dictionaries of about 250 entries, two to four per workgroup of 512 / 1024 rows
        M = N = 3000
        A, square = orc.OracleOp(_stencil_like(M, VALS256), M, M, orc.split_even(M, 1), orc.split_even(M, 1), square=False), False
    elif name == "specials":                    # +-Inf and NaN at a dozen positions of x
        M = N = 3000
        A, square = orc.OracleOp(_stencil_like(M, VALS_SPECIAL), M, M, orc.split_even(M, 1), orc.split_even(M, 1), square=False), False
        x = inputs.v2(M).copy()
        at = [0, 1, 255, 256, 511, 512, 1023, 1024, 1500, 2047, 2998, 2999]
        x[at] = [np.inf, -np.inf, np.nan, np.inf, -np.inf, _SPECIALS[4], np.inf, _SPECIALS[5], -np.inf, np.nan, np.inf, -np.inf]
    else:
        base, _, kind = name.partition(".")
        rows, cols, M, N = X.operator(base)
        vals = {"": VALS5, "values256": VALS256, "specials": VALS_SPECIAL}[kind]
        square = M == N and kind == ""          # (a zero or an Inf on the diagonal: product and u -= A e only, as band256 and specials)
        e = _with_values(rows, cols, vals)
        A = orc.OracleOp(e, M, N, orc.split_even(M, 1)) if square else \
            orc.OracleOp(e, M, N, orc.split_even(M, 1), orc.split_even(N, 1), square=False)
        if kind == "specials":
            # wide19: the last column is read at positions 9..18 of its rows only (the second and third turn of the row loop), column
            # 2500 at every position; five: row 4000 reads column 7000 through the fifth window (offset +3000), row 10000 through the first
            x = _special_x(N, {"wide19": [2500], "five": [7000]}[base])
    if x is None:
        x = inputs.v2(N)
    _CASES[name] = (A, M, N, square, x)
    return _CASES[name]


_CASES = {}
_REF = {}


def _reference(capi, name):
    """variant 11's outputs on the case's inputs, computed once and left unchanged"""
    if name not in _REF:
        A, M, N, square, x = _case(name)
        G = util.gpu_operator(A)
        G.set_variant(11)
        assert G.variant() == (11, "k_sellp")
        _REF[name] = _every_epilogue(capi, G, M, N, x, inputs.rhs2(M), square)
        for v in _REF[name].values():
            v.setflags(write=False)
    return _REF[name]


def assert_same_bits_or_nan(a, b):
    """bit identity, except where both are NaN (payloads are not compared)"""
    both = np.isnan(a) & np.isnan(b)
    np.testing.assert_array_equal(bits(a)[~both], bits(b)[~both])


# poisson12: 1 000 rows, all offsets in one window, one partial workgroup; poisson35: 35 937 rows (no multiple of 64), n = 33 and
# n^2 = 1 089: three windows at every R, those of the first and last workgroups leave the vector at both ends
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", ["poisson12", "poisson35", "band5", "band256", "specials"])
def test_x_windows_bit_identical_to_row_patterns(capi, name, rows, monkeypatch):
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    A, M, N, square, x = _case(name)
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


# ---- the named operators of tests/xwin_ref.py: every branch of k_vidxw and build_xwin -------------------------------------------
GEOMETRY_CASES = list(X.OPERATORS) + ["steps.values256"]
_LINE = re.compile(r"x windows for the value-indexed form: workgroups of (\d+) rows, (\d+) windows, (\d+) doubles of x .* = ([0-9.]+) KiB of LDS")
_PATTERNS = re.compile(r"row patterns: (\d+) rows follow (\d+) patterns of <= (\d+) entries")


def _check_outputs(capi, G, name, out=None):
    A, M, N, square, x = _case(name)
    ref = _reference(capi, name)
    out = _every_epilogue(capi, G, M, N, x, inputs.rhs2(M), square) if out is None else out
    assert set(out) == set(ref)
    for k in ref:
        assert_same_bits(out[k], ref[k])
    np.testing.assert_array_equal(out["spmv"], A.matvec(x))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", GEOMETRY_CASES)
def test_geometries_of_the_named_operators(capi, name, rows, monkeypatch, capfd):
    """where the restatement accepts the geometry: the library reports the same windows, doubles of x and LDS, every epilogue has
    k_sellp's bits and the product the oracle's; where it refuses: the library refuses for the same reason and keeps the direct gathers"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    monkeypatch.setenv("SAENA_SETUP_TIMING", "1")
    A, M, N, square, x = _case(name)
    g = X.named_geometry(name.partition(".")[0], rows)
    G = util.gpu_operator(A)
    G.set_variant(17)
    assert G.variant() == (17, "k_vidx") and G.x_windows() == 0
    m = _PATTERNS.search(capfd.readouterr().err)
    assert m and tuple(map(int, m.groups())) == (M, g["npat"], g["W"])
    if g["verdict"] != X.OK:
        with pytest.raises(capi.SgpuError, match="x windows") as e:
            G.set_x_windows(rows)
        assert g["verdict"] in str(e.value) and re.search("SPX_MAXWIN|LDS cap", str(e.value))
        assert G.x_windows() == 0 and G.variant() == (17, "k_vidx")
        dx, dy = capi.DeviceVector(N, x), capi.DeviceVector(M)
        G.spmv(dx, dy)                                       # the direct gathers
        np.testing.assert_array_equal(dy.download(), A.matvec(x))
        if (name, rows) == ("seven", 1024):                  # after a refused R an accepted one still works
            assert X.named_geometry(name, 512)["verdict"] == X.OK
            G.set_x_windows(512)
            assert G.x_windows() == 512
            _check_outputs(capi, G, name)
        return
    G.set_x_windows(rows)
    assert G.x_windows() == rows and G.variant() == (17, "k_vidx")
    m = _LINE.search(capfd.readouterr().err)
    assert m, "no geometry line on the first build of this workgroup size"
    got = (int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4))
    print(f"{name} at {rows} rows: library {got}, restatement {X.setup_line(g)}, {g['passes']} staging passes, widths {sorted(set(g['w8']))}")
    assert got == X.setup_line(g)
    _check_outputs(capi, G, name)
    G.set_x_windows(0)                                       # and back: the direct gathers of the same operator
    assert G.x_windows() == 0
    dx, dy = capi.DeviceVector(N, x), capi.DeviceVector(M)
    G.spmv(dx, dy)
    assert_same_bits(dy.download(), _reference(capi, name)["spmv"])


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", ["wide19.specials", "five.specials"])
def test_specials_on_the_new_paths(capi, name, rows, monkeypatch):
    """+-0.0, +-Inf and NaNs among the values, +-Inf and NaN in x at the vector's ends, at R - 1 and R, and where a later turn of the
    row loop (wide19) or the fifth window (five) reads them: k_sellp's bits, NaN for NaN"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    A, M, N, square, x = _case(name)
    assert X.named_geometry(name.partition(".")[0], rows)["verdict"] == X.OK
    ref = _reference(capi, name)
    G = util.gpu_operator(A)
    G.set_variant(17)
    G.set_x_windows(rows)
    assert G.x_windows() == rows and G.variant() == (17, "k_vidx")
    out = _every_epilogue(capi, G, M, N, x, inputs.rhs2(M), square)
    assert set(out) == set(ref)
    for k in ref:
        assert_same_bits_or_nan(out[k], ref[k])
    assert np.isnan(out["spmv"]).any() and np.isinf(out["spmv"]).any()


_HALO_REF = {}


def _halo_world(capi, key, entries, M, nprocs, rows, every_rank):
    """product and one Jacobi sweep of an emulated world on variant 17 with windows of `rows` rows, held to the bits of the same world
    on variant 11 (computed once per key).  every_rank: no rank may refuse the mode; else a rank that does says so and keeps its direct
    gathers, and at least one rank runs the mode"""
    split = orc.split_nnz(entries, M, nprocs)
    A = orc.OracleOp(entries, M, M, split)
    W = util.EmulatedWorld(A)
    x, rhs = inputs.v2(M), inputs.rhs2(M)
    in_mode = []

    def run(variant):
        xs, ys, rs, us = W.slices(x, split), W.slices(np.zeros(M), split), W.slices(rhs, split), W.slices(x, split)
        W.exchange(xs); W.exchange(us)
        for r in range(nprocs):
            W.g[r].set_variant(variant); W.g[r].set_lanes_per_row(1)
            if variant == 17:
                try:
                    W.g[r].set_x_windows(rows)
                    in_mode.append(r)
                except capi.SgpuError as e:
                    assert "x windows refused" in str(e) and not every_rank, str(e)
                assert W.g[r].x_windows() == (rows if r in in_mode else 0) and W.g[r].variant() == (17, "k_vidx")
            W.g[r].spmv(xs[r], ys[r])
            W.g[r].jacobi(1, us[r], rs[r])
        return W.gather(ys), W.gather(us)

    if key not in _HALO_REF:
        _HALO_REF[key] = run(11)
    got = run(17)
    assert in_mode, "no rank ran the mode"
    assert_same_bits(got[0], _HALO_REF[key][0])
    assert_same_bits(got[1], _HALO_REF[key][1])
    return in_mode


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nprocs", [2, 3])
def test_x_windows_with_emulated_halos(capi, nprocs, rows, monkeypatch):
    """several ranks on one device: the interior launch masks the boundary rows (HALO); the window mode gives k_sellp's bits"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    entries, M = orc.laplacian3d(20)
    assert _halo_world(capi, nprocs, entries, M, nprocs, rows, True) == list(range(nprocs))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nprocs", [2, 3])
@pytest.mark.parametrize("name", ["wide19", "steps", "five"])
def test_x_windows_with_emulated_halos_on_the_named_operators(capi, name, nprocs, rows, monkeypatch):
    """rows of 19 entries, slices of two widths and five windows under the HALO instantiations, split by nnz.  Every rank of wide19
    runs the mode; elsewhere a rank may refuse it (and says so), and at least one rank runs it"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    r, c, M, _ = X.operator(name)
    in_mode = _halo_world(capi, (name, nprocs), _with_values(r, c, VALS5), M, nprocs, rows, name == "wide19")
    print(f"{name} at {nprocs} ranks, {rows} rows: ranks in the mode {in_mode}")


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


# ---- a V-cycle whose every launch form goes through the mode --------------------------------------------------------------------
_WINDOW_HIERARCHY = None


def _window_hierarchy():
    """three levels by hand: A0 is `five` made SPD (symmetric values, a dominant diagonal); the first aggregation pairs node i with
    node i + 6000 -- R0 is 6000 x 12000 with offsets {0, 6000}, P0 = R0^T has offset 0 in its rows below 6000 and -6000 in the rest:
    patterns relative to the row index, which take the mode (the transfers of a smoothed-aggregation hierarchy are rowbase and do
    not); A1 = R0 A0 P0.  A second aggregation (node i with i + 400 k) leaves 400 rows: the restriction fuses the next level's first
    sweep (RSWEEP) only where that level smooths, and the V-cycle is captured in a graph only where the coarsest level fits the
    LDS-resident solvers."""
    global _WINDOW_HIERARCHY
    if _WINDOW_HIERARCHY is None:
        n0, n1, n2 = 12000, 6000, 400

        def band(o, scale):                                   # entry (i, i + o) and its mirror image: a few distinct values
            return -scale * (1.0 + 0.125 * (np.arange(n0 - o) % 3))
        A0 = sp.diags([8.0 + 0.25 * (np.arange(n0) % 4), band(1500, 1.0), band(1500, 1.0), band(3000, 0.5), band(3000, 0.5)],
                      [0, 1500, -1500, 3000, -3000], format="csr")
        j = np.arange(n1)
        R0 = sp.csr_matrix((np.concatenate([np.ones(n1), np.full(n1, 0.75)]), (np.concatenate([j, j]), np.concatenate([j, j + n1]))), shape=(n1, n0))
        P0 = R0.T.tocsr()
        A1 = (R0 @ A0 @ P0).tocsr()
        i = np.arange(n1)
        R1 = sp.csr_matrix((np.ones(n1), (i % n2, i)), shape=(n2, n1))
        P1 = R1.T.tocsr()
        A2 = (R1 @ A1 @ P1).tocsr()
        As, Ps, Rs = [A0, A1, A2], [P0, P1], [R0, R1]
        assert abs(A0 - A0.T).max() == 0 and (2 * A0.diagonal() > abs(A0).sum(axis=1).A1).all()
        OA, OP, OR = hierarchy.oracle_hierarchy(As, Ps, Rs)
        _WINDOW_HIERARCHY = ((As, Ps, Rs), OA, OP, OR, hierarchy.eig_estimates(As))
    return _WINDOW_HIERARCHY


def test_the_hand_made_transfers_have_windows_relative_to_the_row_index():
    As, Ps, Rs = _window_hierarchy()[0]
    for S, nwin in ((As[0], 5), (Rs[0], 2), (Ps[0], 2)):
        c = S.tocoo()
        for R in ROWS:
            g = X.geometry(c.row, c.col, S.shape[0], S.shape[1], R)
            assert g["verdict"] == X.OK and g["nwin"] == nwin and g["uniform"]


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_vcycle_and_pcg_with_every_launch_form_in_the_mode(capi, smoother, monkeypatch):
    """A0 (residual, Jacobi / Chebyshev sweeps), R0 (RSWEEP: the restriction with level 1's first sweep) and P0 (u -= P e) on variant 17
    with windows: one V-cycle and one pCG solve give the bits -- and pCG the iteration count and residual history -- of the same
    hierarchy on k_sellp.  Switching level 0's mode on the live hierarchy re-captures the V-cycle's graph."""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    _, OA, OP, OR, eig = _window_hierarchy()
    n = OA[0].Mbig
    rhs = inputs.rhs2(n)

    def build(rows):
        GA = [util.gpu_operator(a) for a in OA]
        GP = [util.gpu_operator(q) for q in OP]
        GR = [util.gpu_operator(r) for r in OR]
        three = (GA[0], GP[0], GR[0])
        for G in three:                                       # (level 1 and its transfers keep the form the library gives them)
            G.set_variant(17 if rows else 11); G.set_lanes_per_row(1)
            if rows:
                G.set_x_windows(rows)
        return three, capi.Amg(GA, GP, GR, eig_max=eig, pre=2, post=2, smoother=smoother, coarse_solver="direct"), (GA, GP, GR)

    def check_forms(three, rows):
        for G in three:
            assert G.variant() == ((17, "k_vidx") if rows else (11, "k_sellp")) and G.x_windows() == rows

    def run(amg, du, dr):
        du.upload(np.zeros(n))
        before = capi.launch_count()
        amg.vcycle(du, dr)
        launches = capi.launch_count() - before
        u = du.download()
        du.upload(np.zeros(n))
        it, hist, ok = amg.solve_pCG(du, dr)
        return u, launches, (du.download(), it, hist, ok)

    three, amg, keep = build(0)
    du, dr = capi.DeviceVector(n), capi.DeviceVector(n, rhs)
    ref_u, _, ref_pcg = run(amg, du, dr)
    check_forms(three, 0)
    assert ref_pcg[3] and ref_pcg[1] > 1 and np.isfinite(ref_u).all() and np.abs(ref_u).max() > 0
    amg.destroy()

    three, amg, keep = build(512)
    du, dr = capi.DeviceVector(n), capi.DeviceVector(n, rhs)
    u, first, pcg = run(amg, du, dr)
    check_forms(three, 512)
    assert_same_bits(u, ref_u)
    assert_same_bits(pcg[0], ref_pcg[0])
    assert pcg[1] == ref_pcg[1] and pcg[3] == ref_pcg[3]
    assert_same_bits(pcg[2], ref_pcg[2])
    u, replay, _ = run(amg, du, dr)                           # the captured graph once more: one enqueue
    assert_same_bits(u, ref_u)
    assert replay < first
    # level 0 back to its direct gathers, then to other workgroup sizes, on the live hierarchy: a stale graph would replay the launches
    # of the mode it was captured with; the library drops it and captures again (as many enqueues as the first V-cycle)
    for rows in (0, 256, 1024):
        three[0].set_x_windows(rows)
        u, launches, _ = run(amg, du, dr)
        assert three[0].x_windows() == rows and three[0].variant() == (17, "k_vidx")
        assert three[1].x_windows() == 512 and three[2].x_windows() == 512
        assert_same_bits(u, ref_u)
        assert launches > replay, "the V-cycle's graph was replayed, not captured again"
    amg.destroy()


# ---- the plan cache's mode field and the development pin ------------------------------------------------------------------------
_PLAN = {}


def _plan_operator():
    """`seven` at 32 000 rows: 206 000 entries, above the autotune's floor of 200 000 -> (OracleOp, M, x, the oracle's product, geometry per R)"""
    if "op" not in _PLAN:
        M = 32000
        offsets = X.OPERATORS["seven"][2][0][0]
        e = _diagonals(M, offsets, VALS5)
        assert len(e) == 206000
        A = orc.OracleOp(e, M, M, orc.split_even(M, 1))
        x = inputs.v2(M)
        c = hierarchy.coo_to_scipy(e, M, M).tocoo()
        st = X.structure(c.row, c.col, M)
        _PLAN["op"] = (A, M, x, A.matvec(x), {R: X.geometry(c.row, c.col, M, M, R, st) for R in ROWS})
        _PLAN["entries"] = e
    return _PLAN["op"]


def _lines(path):
    return [ln for ln in open(path).read().splitlines() if ln.strip()] if path.exists() else []


def _tuned_line(capi, tmp_path_factory, monkeypatch):
    """the line the autotune writes for the operator (its key, and what the sweep chooses), found once"""
    if "line" not in _PLAN:
        path = tmp_path_factory.mktemp("plan") / "plans.tsv"
        monkeypatch.setenv("SAENA_PLAN_CACHE", str(path))
        G = util.gpu_operator(_plan_operator()[0])
        G.autotune()
        lines = _lines(path)
        assert len(lines) == 1
        _PLAN["line"] = lines[0]
    return _PLAN["line"]


def _with_plan(line, variant, lanes, xw):
    f = line.split("\t")
    f[1:4] = [str(variant), str(lanes), str(xw)]
    return "\t".join(f)


def _product(capi, G, M, x):
    dx, dy = capi.DeviceVector(M, x), capi.DeviceVector(M)
    G.spmv(dx, dy)
    return dy.download()


def _check_tuned_product(capi, G, line):
    """a sweep keeps the fastest form, and on an operator of this size that may be one that adds a row's products across lanes
    (k_csr_vector): the product of a form with the sequential row sum (the library's sequential_sum()) is the oracle's, bit for bit;
    that of any other form has the bits of the same variant and lanes set by hand on a fresh operator -- a plan never changes a
    form's result -- and meets the catalogue's contract for such forms against the oracle (tests/test_gpu_forms.py)"""
    from tests import test_gpu_forms as F
    A, M, x, want, geo = _plan_operator()
    v, lanes, xw = (int(f) for f in line.split("\t")[1:4])
    assert G.variant()[0] == v and G.x_windows() == xw and G.info()["lanes_per_row"] == lanes
    got = _product(capi, G, M, x)
    if v in (9, 11, 13, 14, 15, 17) or (lanes == 1 and v in (0, 1, 3, 4, 7, 8)):
        np.testing.assert_array_equal(got, want)
        return
    H = util.gpu_operator(A)
    H.set_variant(v); H.set_lanes_per_row(lanes)
    assert_same_bits(got, _product(capi, H, M, x))
    lim = F.TOL * F.abs_bound(_PLAN["entries"], M, x) + 2 * F.EPS * np.abs(want) + 1e-300
    assert (np.abs(got - want) <= lim).all()


def test_plan_cache_restores_the_mode(capi, tmp_path, tmp_path_factory, monkeypatch):
    """a cached plan of variant 17 with windows of 512 rows is taken as it stands: no sweep, no new line, the oracle's product; another
    workgroup size can still be built on that plan (the tables of the sizes not in use were freed, not barred)"""
    monkeypatch.delenv("SAENA_KEEP_HOST_VALUES", raising=False)
    A, M, x, want, geo = _plan_operator()
    assert geo[512]["verdict"] == X.OK and geo[256]["verdict"] == X.OK
    line = _tuned_line(capi, tmp_path_factory, monkeypatch)
    path = tmp_path / "plans.tsv"
    path.write_text(line + "\n" + _with_plan(line, 17, 1, 512) + "\n")
    monkeypatch.setenv("SAENA_PLAN_CACHE", str(path))
    G = util.gpu_operator(A)
    G.autotune()
    assert G.variant() == (17, "k_vidx") and G.x_windows() == 512
    assert len(_lines(path)) == 2
    np.testing.assert_array_equal(_product(capi, G, M, x), want)
    G.set_x_windows(256)
    assert G.x_windows() == 256 and G.variant() == (17, "k_vidx")
    np.testing.assert_array_equal(_product(capi, G, M, x), want)


@pytest.mark.parametrize("fields", [(17, 1, 384), (11, 1, 512)])
def test_plan_cache_ignores_invalid_mode_lines(capi, fields, tmp_path, tmp_path_factory, monkeypatch):
    """a size the mode does not have, or windows on another variant: not a plan.  Alone in the cache the operator is tuned afresh and a
    line is appended; behind a valid line of the same key, that line is the plan"""
    monkeypatch.delenv("SAENA_KEEP_HOST_VALUES", raising=False)
    A, M, x, want, geo = _plan_operator()
    line = _tuned_line(capi, tmp_path_factory, monkeypatch)
    path = tmp_path / "plans.tsv"
    path.write_text(_with_plan(line, *fields) + "\n")
    monkeypatch.setenv("SAENA_PLAN_CACHE", str(path))
    G = util.gpu_operator(A)
    G.autotune()
    lines = _lines(path)
    assert len(lines) == 2 and lines[1].split("\t")[0] == line.split("\t")[0]
    assert G.x_windows() == 0 or G.variant() == (17, "k_vidx")
    _check_tuned_product(capi, G, lines[1])
    path.write_text(_with_plan(line, 17, 1, 256) + "\n" + _with_plan(line, *fields) + "\n")
    G = util.gpu_operator(A)
    G.autotune()
    assert len(_lines(path)) == 2
    assert G.variant() == (17, "k_vidx") and G.x_windows() == 256
    np.testing.assert_array_equal(_product(capi, G, M, x), want)


def test_plan_cache_with_a_mode_the_operator_refuses(capi, tmp_path, tmp_path_factory, monkeypatch):
    """windows of 1024 rows exceed the LDS cap on this operator: the cached plan falls through to the sweep"""
    monkeypatch.delenv("SAENA_KEEP_HOST_VALUES", raising=False)
    A, M, x, want, geo = _plan_operator()
    assert geo[1024]["verdict"] == X.LDS_CAP
    line = _tuned_line(capi, tmp_path_factory, monkeypatch)
    path = tmp_path / "plans.tsv"
    path.write_text(line + "\n" + _with_plan(line, 17, 1, 1024) + "\n")
    monkeypatch.setenv("SAENA_PLAN_CACHE", str(path))
    G = util.gpu_operator(A)
    G.autotune()
    assert len(_lines(path)) == 3
    assert G.x_windows() in [0] + [R for R in ROWS if geo[R]["verdict"] == X.OK]
    assert G.x_windows() == 0 or G.variant() == (17, "k_vidx")
    _check_tuned_product(capi, G, _lines(path)[2])


def test_the_development_pin_of_the_mode(capi, monkeypatch):
    """SAENA_X_WINDOWS pins the mode where only the variant can be pinned: set_variant(17) turns it on where the operator takes it,
    and leaves the direct gathers -- raising nothing -- where it does not, or where the size is none of the mode's"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    A, M, N, square, x = _case("five")
    monkeypatch.setenv("SAENA_X_WINDOWS", "512")
    G = util.gpu_operator(A)
    G.set_variant(17)
    assert G.x_windows() == 512 and G.variant() == (17, "k_vidx")
    assert_same_bits(_product(capi, G, M, x), _reference(capi, "five")["spmv"])
    G.set_variant(11)
    assert G.x_windows() == 0                                 # (the pin belongs to variant 17)
    B, Mb, Nb, _, xb = _case("seventeen")
    H = util.gpu_operator(B)
    H.set_variant(17)
    assert H.x_windows() == 0 and H.variant() == (17, "k_vidx")
    np.testing.assert_array_equal(_product(capi, H, Mb, xb), B.matvec(xb))
    monkeypatch.setenv("SAENA_X_WINDOWS", "384")
    G = util.gpu_operator(A)
    G.set_variant(17)
    assert G.x_windows() == 0 and G.variant() == (17, "k_vidx")
    np.testing.assert_array_equal(_product(capi, G, M, x), A.matvec(x))
