"""The prologue of k_vidxw (variant 17 + set_x_windows(R)): the head of the window table arrives in the kernel arguments, the
dictionaries' offsets are computed where all dictionaries of the operator have one length (else read together), and every wave loads
a dictionary value and a table chunk with clamped indices before it waits.  None of that may change a bit: every case compares the
mode with k_sellp (variant 11) on the same operator, bit for bit, for the product, the residual and two Jacobi sweeps, at every
workgroup size the operator takes.  x carries one NaN and one Inf.

The operators are made for the paths of the prologue; what puts an operator on its path (the dictionaries' lengths, the table's
words, the windows, the slices' widths) is computed here from its entries and asserted, so a case cannot silently run another path."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import inputs, util
from tests import test_gpu_x_windows as XW
from tests import xwin_ref as X

pytestmark = pytest.mark.gpu

ROWS = X.ROWS
GROUP = 256                                     # rows of one dictionary


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


# ---- operators: (rows, cols, vals, M, N), row-major with columns ascending -------------------------------------------------------
def _tridiagonal(M):
    r = np.arange(M)
    rows = np.concatenate([r, r[1:], r[:-1]])
    cols = np.concatenate([r, r[1:] - 1, r[:-1] + 1])
    order = np.lexsort((cols, rows))
    return rows[order], cols[order]


def _group_values(rows, counts):
    """the entries of group g (rows [256 g, 256 g + 256)) take counts[g] distinct values in turn, no value shared between groups"""
    v = np.zeros(len(rows))
    g = rows // GROUP
    for k, n in enumerate(counts):
        at = np.flatnonzero(g == k)
        assert n <= len(at)
        v[at] = 1.0 + (k * GROUP + np.arange(len(at)) % max(n, 1)) / 4096.0
    return v


def dictionary_lengths(rows, vals, M):
    """distinct bit patterns among the values of every group of 256 rows: what build_vidx counts"""
    g = np.asarray(rows) // GROUP
    b = np.ascontiguousarray(vals, np.float64).view(np.uint64)
    return [len(np.unique(b[g == k])) for k in range((M + GROUP - 1) // GROUP)]


def _band(M, counts, keep=None):
    rows, cols = _tridiagonal(M)
    if keep is not None:
        sel = keep(rows)
        rows, cols = rows[sel], cols[sel]
    return rows, cols, _group_values(rows, counts), M, M


def _uniform(kind):
    """11 dictionaries (no multiple of 2 or 4: the last workgroup of 512 and of 1024 rows owns fewer than D) of 3 values each, the last
    group 100 rows.  planted: one more value in group 5; short: the last group holds 2"""
    M = 10 * GROUP + 100
    rows, cols, vals, M, N = _band(M, [3] * 10 + [2 if kind == "short" else 3])
    if kind == "planted":
        vals[np.flatnonzero(rows == 5 * GROUP + 77)[1]] = 7.5
    return rows, cols, vals, M, N


def _full():
    """groups 2 and 3 hold 256 distinct values each: every lane of their workgroups of 256 rows, and of the one workgroup of 512 rows
    that owns both, stages a value"""
    return _band(6 * GROUP, [2, 2, 256, 256, 2, 5])


def _empty():
    """the rows of group 3 and of the last group (6) are empty: dictionaries of no value, the last one where vdict ends"""
    return _band(7 * GROUP, [3, 3, 3, 0, 3, 3, 0], keep=lambda r: (r // GROUP != 3) & (r // GROUP != 6))


def _long_table():
    """299 patterns of 7 offsets from [-8, 8] (the diagonal among them) and the diagonal alone on the first and last 8 rows: 300
    patterns, 304 + 300 x 8 = 2704 words = 338 chunks of 16 bytes"""
    M = 3000
    rng = np.random.default_rng(8)
    others = [o for o in range(-8, 9) if o != 0]
    pats = set()
    while len(pats) < 299:
        pats.add(tuple(sorted([0] + list(rng.choice(others, 6, replace=False)))))
    pats = sorted(pats)
    rr, cc = [], []
    for r in range(M):
        offs = (0,) if r < 8 or r >= M - 8 else pats[r % 299]
        rr += [r] * len(offs); cc += [r + o for o in offs]
    rows, cols = np.asarray(rr), np.asarray(cc)
    return rows, cols, np.asarray(XW.VALS5)[np.arange(len(rows)) % 5], M, M


def _named(name):
    rows, cols, M, N = X.operator(name)
    return rows, cols, np.asarray(XW.VALS5)[np.arange(len(rows)) % 5], M, N


OPERATORS = {
    "uniform": lambda: _uniform(""), "planted": lambda: _uniform("planted"), "short": lambda: _uniform("short"),
    "full": _full, "empty": _empty, "long_table": _long_table,
    "five": lambda: _named("five"), "seven": lambda: _named("seven"), "tiny": lambda: _named("tiny"), "steps": lambda: _named("steps"),
}
_OPS, _GEOM, _REF = {}, {}, {}


def operator(name):
    """-> (rows, cols, vals, M, N, OracleOp, x), built once"""
    if name not in _OPS:
        rows, cols, vals, M, N = OPERATORS[name]()
        e = orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), vals)
        A = orc.OracleOp(e, M, N, orc.split_even(M, 1))
        x = inputs.v2(N).copy()
        x[N // 3], x[2 * N // 3 + 1] = np.nan, np.inf
        x.setflags(write=False)
        _OPS[name] = (rows, cols, vals, M, N, A, x)
    return _OPS[name]


def geometry(name, R):
    if (name, R) not in _GEOM:
        rows, cols, vals, M, N, A, x = operator(name)
        _GEOM[(name, R)] = X.geometry(rows, cols, M, N, R)
    return _GEOM[(name, R)]


def _outputs(capi, G, M, N, x):
    dx, dy, dr = capi.DeviceVector(N, x), capi.DeviceVector(M), capi.DeviceVector(M, inputs.rhs2(M))
    out = {}
    G.spmv(dx, dy)
    out["spmv"] = dy.download()
    G.residual(dx, dr, dy)
    out["residual"] = dy.download()
    du = capi.DeviceVector(M, x)
    G.jacobi(2, du, dr)
    out["jacobi"] = du.download()
    return out


def reference(capi, name):
    """k_sellp's outputs, computed once and left unchanged"""
    if name not in _REF:
        rows, cols, vals, M, N, A, x = operator(name)
        G = util.gpu_operator(A)
        G.set_variant(11)
        assert G.variant() == (11, "k_sellp")
        _REF[name] = _outputs(capi, G, M, N, x)
        for v in _REF[name].values():
            v.setflags(write=False)
    return _REF[name]


def check(capi, name, R, monkeypatch):
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    rows, cols, vals, M, N, A, x = operator(name)
    assert geometry(name, R)["verdict"] == X.OK
    ref = reference(capi, name)
    G = util.gpu_operator(A)
    G.set_variant(17)
    G.set_x_windows(R)
    assert G.x_windows() == R and G.variant() == (17, "k_vidx")
    out = _outputs(capi, G, M, N, x)
    for k in ref:
        XW.assert_same_bits_or_nan(out[k], ref[k])
    assert np.isnan(out["spmv"]).any() and np.isinf(out["spmv"]).any()
    reached = np.zeros(M, bool)                               # the NaN and the Inf reach the rows that hold their columns, no other
    reached[rows[np.isin(cols, np.flatnonzero(~np.isfinite(x)))]] = True
    np.testing.assert_array_equal(~np.isfinite(out["spmv"]), reached)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(out["spmv"][~reached], A.matvec(x)[~reached])


# ---- the dictionaries' offsets: computed (one length) or read (lengths differ) ------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name", ["uniform", "planted", "short"])
def test_dictionaries_of_one_length_and_of_differing_lengths(capi, name, R, monkeypatch):
    rows, cols, vals, M, N, A, x = operator(name)
    lens = dictionary_lengths(rows, vals, M)
    assert len(lens) == 11 and len(lens) % 2 and len(lens) % 4
    assert lens == {"uniform": [3] * 11, "planted": [3] * 5 + [4] + [3] * 5, "short": [3] * 10 + [2]}[name]
    assert geometry(name, R)["uniform"]                      # (the slices: one width, so a.uw)
    check(capi, name, R, monkeypatch)


@pytest.mark.parametrize("R", ROWS)
def test_a_full_dictionary_in_every_lane(capi, R, monkeypatch):
    rows, cols, vals, M, N, A, x = operator("full")
    assert dictionary_lengths(rows, vals, M) == [2, 2, 256, 256, 2, 5]
    check(capi, "full", R, monkeypatch)


@pytest.mark.parametrize("R", ROWS)
def test_empty_dictionaries_in_the_middle_and_at_the_end(capi, R, monkeypatch):
    """the library accepts the operator (sgpu_op_create and build_vidx refuse nothing here): the workgroup of the trailing 256 empty
    rows begins its dictionary where vdict ends, and its lanes read the one element vdict is padded by"""
    rows, cols, vals, M, N, A, x = operator("empty")
    assert dictionary_lengths(rows, vals, M) == [3, 3, 3, 0, 3, 3, 0]
    assert not geometry("empty", R)["uniform"] and 0 in geometry("empty", R)["w8"]
    check(capi, "empty", R, monkeypatch)


@pytest.mark.parametrize("R", ROWS)
def test_a_table_of_more_chunks_than_a_workgroup_of_256_rows_has_lanes(capi, R, monkeypatch):
    g = geometry("long_table", R)
    assert (g["npat"], g["W"], g["words"]) == (300, 7, 2704) and g["words"] // 8 == 338
    assert (338 > R) == (R == 256)                           # the chunk loaded at the top and the loop at 256 rows, the chunk alone beyond
    check(capi, "long_table", R, monkeypatch)


# ---- the head in the arguments, the tail from the window table ----------------------------------------------------------------------
@pytest.mark.parametrize("name,R", [(n, R) for n in ("five", "seven") for R in ROWS if X.named_geometry(n, R)["verdict"] == X.OK])
def test_fewer_and_more_than_four_windows(capi, name, R, monkeypatch):
    g = geometry(name, R)
    assert g["nwin"] == {"five": 5, "seven": 7}[name]
    check(capi, name, R, monkeypatch)


def test_both_sides_of_four_windows_ran():
    ran = [(n, R) for n in ("five", "seven") for R in ROWS if X.named_geometry(n, R)["verdict"] == X.OK]
    assert ("five", 256) in ran and ("seven", 512) in ran and X.named_geometry("wide19", 256)["nwin"] < 4


# ---- waves without a slice, slices of differing widths -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "steps"])
def test_dead_waves_and_slice_pointers_at_1024_rows(capi, name, monkeypatch):
    """tiny: one slice, fifteen waves of its workgroup without one; steps: 94 slices of two widths (the slice pointers are read), the
    last workgroup's waves from slice 94 on are dead and read slice 0's pointers"""
    g = geometry(name, 1024)
    ns = len(g["w8"])
    assert ns % 16 and g["uniform"] == (name == "tiny")
    check(capi, name, 1024, monkeypatch)


# ---- one HALO instantiation -------------------------------------------------------------------------------------------------------
def test_the_interior_launch_of_an_emulated_world(capi, monkeypatch):
    """wide19 split over two ranks on one device: the interior launch (HALO) masks the boundary rows; k_sellp's bits"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    r, c, M, _ = X.operator("wide19")
    assert XW._halo_world(capi, ("prologue", "wide19"), XW._with_values(r, c, XW.VALS5), M, 2, 256, True) == [0, 1]
