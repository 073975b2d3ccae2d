"""k_vidxw_fast, the common path of k_vidxw (variant 17 + set_x_windows(R)) as a kernel of its own: saena_amd/csrc/vw_fast.h says which
operator x R and which launch take it, and whether dictionaries of at most two values stay in scalar registers.  None of that may
change a bit: every case compares the product, the residual and two Jacobi sweeps with k_sellp (variant 11) on the same operator, bit
for bit, at R = 256 and 512 -- in the style and with the helpers of tests/test_gpu_vidxw_staging.py.

Which kernel an operator takes is computed here from its entries (the rule restated: one slice width, one dictionary length, one to
four trips, a table of at most R chunks; at most two values per dictionary -> scalar registers) and asserted twice: from the line the
library prints behind its x-window line (SAENA_SETUP_TIMING) and from sgpu_op_get_x_window_kernel before and after the launches.  So a
case cannot silently take the other kernel."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import inputs, util
from tests import test_gpu_vidxw_staging as ST
from tests import test_gpu_x_windows as XW
from tests import xwin_ref as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (256, 512)
GENERAL, LDS_DICT, SCALAR_DICT = 0, 1, 2
_KERNEL = re.compile(r"x windows at (\d+) rows: (?:the common-path kernel is taken, dictionaries of (\d+) values in (scalar registers|LDS), (\d+) bytes of LDS"
                     r"|the general kernel is kept \((.*)\))")
NOT_256_512, WIDTHS, DICT_LENGTHS, TRIPS, SWITCHED_OFF = ("workgroups of neither 256 nor 512 rows", "slices of differing widths", "dictionaries of differing lengths",
                                                          "not staged window by window in one to four trips", "SAENA_VIDXW_FAST=0")
NAN_PAYLOAD = np.array([0x7ff8000000abc123], np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


# ---- operators ------------------------------------------------------------------------------------------------------------------------
def two_diagonals(R, value_of):
    """the diagonals {0, 1} of 3 R + 17 rows, the value of an entry given by value_of(row, 0 | 1) -> arrays"""
    rows, cols, _, M, N = ST.band(1, R)
    return rows, cols, value_of(rows, cols - rows), M, N


def by_group(a, b):
    """a, b alternating along the entries of a group of 256 rows, the groups beginning with a and with b in turn: the first value a
    group sees -- its code 0 -- differs from its neighbours'"""
    return lambda r, d: np.where((r + d + r // 256) % 2 == 0, a, b)


DICTIONARIES = {
    "one value": lambda R: two_diagonals(R, lambda r, d: np.full(len(r), 2.5)),
    "two values": lambda R: two_diagonals(R, by_group(4.0, -1.25)),
    # the second group of 256 rows holds 4.0 alone: the dictionaries' lengths differ
    "two values, one group with one": lambda R: two_diagonals(R, lambda r, d: np.where(r // 256 == 1, 4.0, by_group(4.0, -1.25)(r, d))),
    "three values": lambda R: two_diagonals(R, lambda r, d: np.asarray([4.0, -1.25, 1.0 / 3.0])[(2 * r + d) % 3]),
    # (the library, like the reference, refuses a zero on the diagonal: the signed zeros come without the diagonal's contract -- no
    # inverse diagonal, so product and residual only; Inf and the NaN stay off the diagonal or have an inverse)
    "signed zeros": lambda R: two_diagonals(R, by_group(-0.0, 0.0)),
    "infinities": lambda R: two_diagonals(R, lambda r, d: np.where(d == 0, np.inf, -np.inf)),
    "a NaN with a payload": lambda R: two_diagonals(R, lambda r, d: np.where(d == 0, 1.5, NAN_PAYLOAD)),
}
NO_DIAGONAL = ("signed zeros",)
_OPS, _REF = {}, {}


def make(key):
    """("dict", name, R): the operators above, with a finite x; ("named", name): tests/xwin_ref.py's; else tests/test_gpu_vidxw_staging.py's"""
    if key[0] not in ("dict", "named"):
        return ST.make(key)
    if key not in _OPS:
        rows, cols, vals, M, N = DICTIONARIES[key[1]](key[2]) if key[0] == "dict" else ST.named(key[1])
        e = orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), np.ascontiguousarray(vals, np.float64))
        A = orc.OracleOp(e, M, N, orc.split_even(M, 1)) if key[1] not in NO_DIAGONAL else \
            orc.OracleOp(e, M, N, orc.split_even(M, 1), orc.split_even(N, 1), square=False)
        x = inputs.v2(N).copy()
        if key[0] == "named":
            x[N // 3], x[2 * N // 3 + 1] = np.nan, np.inf
        x.setflags(write=False)
        _OPS[key] = (rows, cols, vals, M, N, A, x)
    return _OPS[key]


def reference(capi, key, x=None, rhs=None, tag=None, u0=None):
    """k_sellp's outputs, computed once per (operator, inputs) and left unchanged"""
    if key[0] not in ("dict", "named"):
        return ST.reference(capi, key, x, rhs, tag, u0)
    if (key, tag) not in _REF:
        rows, cols, vals, M, N, A, x0 = make(key)
        G = util.gpu_operator(A)
        G.set_variant(11)
        assert G.variant() == (11, "k_sellp")
        _REF[(key, tag)] = outputs(capi, key, G, M, N, x0 if x is None else x, rhs, u0)
        for v in _REF[(key, tag)].values():
            v.setflags(write=False)
    return _REF[(key, tag)]


def outputs(capi, key, G, M, N, x, rhs=None, u0=None):
    """tests/test_gpu_vidxw_staging.py's: product, residual, two Jacobi sweeps; an operator without an inverse diagonal: no sweeps"""
    if key[0] != "dict" or key[1] not in NO_DIAGONAL:
        return ST.outputs(capi, G, M, N, x, rhs, u0)
    dx, dy, dr = capi.DeviceVector(N, x), capi.DeviceVector(M), capi.DeviceVector(M, inputs.rhs2(M) if rhs is None else rhs)
    out = {}
    G.spmv(dx, dy)
    out["spmv"] = dy.download()
    G.residual(dx, dr, dy)
    out["residual"] = dy.download()
    return out


# ---- the rule, restated from the operator's entries -------------------------------------------------------------------------------------
def expected(key, R, env_off=False):
    """-> (kind, the clause that refuses or None, LDS bytes of the lean kernel or None, values per dictionary or 0)"""
    rows, cols, vals, M, N, A, x = make(key)
    g = X.geometry(rows, cols, M, N, R)
    assert g["verdict"] == X.OK
    order = np.lexsort((cols, rows))
    pat = np.ascontiguousarray(np.asarray(vals, np.float64)[order]).view(np.uint64)
    grp = np.asarray(rows)[order] // 256
    sizes = {len(set(pat[grp == b].tolist())) for b in range((M + 255) // 256)}
    vd_u = sizes.pop() if len(sizes) == 1 else 0
    ntrip = sum(-(-(R + hi - lo) // R) for lo, hi in g["windows"]) if g["nwin"] <= 4 and g["S"] <= 4 * R else 0
    clause = (NOT_256_512 if R not in (256, 512) else WIDTHS if not g["uniform"] else DICT_LENGTHS if vd_u == 0 else TRIPS if not 1 <= ntrip <= 4 else None)
    assert g["words"] // 8 <= R                                   # (no operator here has a table of more than R chunks: tests/test_vw_fast_header.py holds that clause)
    if clause is None and env_off:
        clause = SWITCHED_OFF
    if clause is not None:
        return GENERAL, clause, None, vd_u
    kind = SCALAR_DICT if vd_u <= 2 else LDS_DICT
    return kind, None, g["lds"] - (R // 256 * X.VI_MAX * 8 if kind == SCALAR_DICT else 0), vd_u


def in_mode(capi, key, R, monkeypatch, capfd, want, env_off=False):
    """the operator on variant 17 with windows of R rows; the library's two lines and its getter say which kernel it takes"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    monkeypatch.setenv("SAENA_SETUP_TIMING", "1")
    if env_off:
        monkeypatch.setenv("SAENA_VIDXW_FAST", "0")
    else:
        monkeypatch.delenv("SAENA_VIDXW_FAST", raising=False)
    kind, clause, lds, vd_u = expected(key, R, env_off)
    assert (kind, clause) == want, (kind, clause, vd_u)
    rows, cols, vals, M, N, A, x = make(key)
    G = util.gpu_operator(A)
    G.set_variant(17)
    assert G.x_window_kernel() == GENERAL                     # (the mode is off)
    capfd.readouterr()
    G.set_x_windows(R)
    err = capfd.readouterr().err
    assert G.x_windows() == R and G.variant() == (17, "k_vidx")
    staged, m = ST._STAGED.search(err), _KERNEL.search(err)
    assert staged and m and int(staged.group(1)) == int(m.group(1)) == R and staged.end() < m.start(), err[-1500:]
    if kind == GENERAL:
        assert m.group(5) == clause, m.groups()
    else:
        assert (int(m.group(2)), m.group(3), int(m.group(4))) == (vd_u, "scalar registers" if kind == SCALAR_DICT else "LDS", lds), m.groups()
    assert G.x_window_kernel() == kind
    return G


def check(capi, key, R, monkeypatch, capfd, want, env_off=False, same=XW.assert_same_bits_or_nan):
    rows, cols, vals, M, N, A, x = make(key)
    ref = reference(capi, key)
    G = in_mode(capi, key, R, monkeypatch, capfd, want, env_off)
    out = outputs(capi, key, G, M, N, x)
    assert G.x_window_kernel() == want[0]                     # what the last launch (a Jacobi sweep) ran
    assert set(out) == set(ref) and (M != N or set(out) == {"spmv", "residual", "jacobi"} or key[1] in NO_DIAGONAL)
    for k in ref:
        same(out[k], ref[k])
    return out


# ---- which kernel is taken ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
def test_switched_off_by_the_environment_the_general_kernel_gives_the_same_bits(capi, R, monkeypatch, capfd):
    """both paths in one process: the environment is read per operator"""
    key = ("band", 65, R)
    off = check(capi, key, R, monkeypatch, capfd, (GENERAL, SWITCHED_OFF), env_off=True)
    on = check(capi, key, R, monkeypatch, capfd, (LDS_DICT, None))
    for k in on:
        XW.assert_same_bits_or_nan(on[k], off[k])


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("key,clause", [(("named", "steps"), WIDTHS), (("five",), TRIPS), (("six",), TRIPS)])
def test_slice_pointers_flat_staging_and_six_trips_keep_the_general_kernel(capi, key, clause, R, monkeypatch, capfd):
    check(capi, key, R, monkeypatch, capfd, (GENERAL, clause))


def test_1024_rows_keep_the_general_kernel(capi, monkeypatch, capfd):
    check(capi, ("band", 65, 256), 1024, monkeypatch, capfd, (GENERAL, NOT_256_512))


def test_a_halo_launch_of_an_eligible_operator_keeps_the_general_kernel(capi, monkeypatch):
    """the diagonals {-65, 0, 65} of 5000 rows split over two ranks on one device (the emulated halo of the x-window tests): both ranks
    have a halo and an eligible local part; the interior launch masks the boundary rows and runs k_vidxw; k_sellp's bits"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    monkeypatch.delenv("SAENA_VIDXW_FAST", raising=False)
    rows, cols, vals, M, N = ST.diagonals(5000, [-65, 0, 65])
    e = orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), vals)
    split = orc.split_nnz(e, M, 2)
    W = util.EmulatedWorld(orc.OracleOp(e, M, M, split))
    x, rhs = inputs.v2(M), inputs.rhs2(M)
    ran = []

    def run(variant):
        xs, ys, rs, us = W.slices(x, split), W.slices(np.zeros(M), split), W.slices(rhs, split), W.slices(x, split)
        W.exchange(xs); W.exchange(us)
        for r in range(2):
            W.g[r].set_variant(variant); W.g[r].set_lanes_per_row(1)
            if variant == 17:
                W.g[r].set_x_windows(256)
                assert W.g[r].x_window_kernel() == LDS_DICT       # what a launch without a halo would run
            W.g[r].spmv(xs[r], ys[r])
            if variant == 17:
                ran.append(W.g[r].x_window_kernel())
            W.g[r].jacobi(1, us[r], rs[r])
            if variant == 17:
                ran.append(W.g[r].x_window_kernel())
        return W.gather(ys), W.gather(us)

    ref, got = run(11), run(17)
    assert ran == [GENERAL] * 4
    XW.assert_same_bits(got[0], ref[0])
    XW.assert_same_bits(got[1], ref[1])


# ---- the dictionaries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name,want", [("one value", (SCALAR_DICT, None)), ("two values", (SCALAR_DICT, None)), ("two values, one group with one", (GENERAL, DICT_LENGTHS)),
                                       ("three values", (LDS_DICT, None)), ("signed zeros", (SCALAR_DICT, None)), ("infinities", (SCALAR_DICT, None)),
                                       ("a NaN with a payload", (SCALAR_DICT, None))])
def test_dictionaries_of_one_two_and_three_values(capi, name, want, R, monkeypatch, capfd):
    """x is finite: every bit is compared, those of the NaNs included -- a decoded value is the stored bit pattern"""
    key = ("dict", name, R)
    rows, cols, vals, M, N, A, x = make(key)
    first = np.ascontiguousarray(vals[np.searchsorted(rows, np.arange(0, M, 256))], np.float64).view(np.uint64)
    if name in ("two values", "signed zeros"):
        assert first[0] != first[1]                               # code 0 of neighbouring dictionaries: different values
    out = check(capi, key, R, monkeypatch, capfd, want, same=XW.assert_same_bits)
    if name == "signed zeros":
        assert (out["spmv"] == 0).all()                           # (a sum begins at +0.0, so the zeros' signs show in the residual alone)
    if name == "a NaN with a payload":
        assert np.isnan(out["spmv"][:-1]).all()                   # (every row but the last holds the NaN)


@pytest.mark.parametrize("R", ROWS)
def test_the_five_values_of_the_staging_tests_take_the_lds_dictionary(capi, R, monkeypatch, capfd):
    assert expected(("band", 1, R), R)[3] == len(XW.VALS5) == 5
    check(capi, ("band", 1, R), R, monkeypatch, capfd, (LDS_DICT, None))


# ---- the geometries -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("k", ["0", "1", "63", "64", "65", "R-1", "R"])
def test_one_window_of_every_size_up_to_two_trips(capi, k, R, monkeypatch, capfd):
    """M = 3 R + 17: a partial last workgroup with spare waves; one trip (k = 0) or two"""
    kk = {"R-1": R - 1, "R": R}.get(k) if k.startswith("R") else int(k)
    assert make(("band", kk, R))[3] % R == 17
    check(capi, ("band", kk, R), R, monkeypatch, capfd, (LDS_DICT, None))


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("key", [("ends",), ("tall",), ("flat",), ("four",), ("named", "tiny"), ("holes",), ("len3",), ("len8",), ("len9",), ("len16",)])
def test_windows_and_pattern_lengths(capi, key, R, monkeypatch, capfd):
    """windows that leave x at both ends, fewer and more columns than rows, four windows, one partial slice, lmin = 0, and one body of
    the row loop each: lengths 3, 8, 5 ... 9 and 8 ... 16 (the last two: two turns of the loop)"""
    check(capi, key, R, monkeypatch, capfd, (LDS_DICT, None))


@pytest.mark.parametrize("R", ROWS)
def test_specials_where_only_padded_positions_read(capi, R, monkeypatch, capfd):
    """tests/test_gpu_vidxw_staging.py's case on the lean kernel: NaN and +-Inf in columns that only padded positions read change no
    product, no residual, and no Jacobi sweep that begins at a finite u"""
    key = ("pad",)
    rows, cols, vals, M, N, A, x0 = make(key)
    only_padded = np.arange(N) % 20 == 7
    assert not np.isin(cols, np.flatnonzero(only_padded)).any() and np.bincount(rows, minlength=M).min() == 0
    plain = inputs.v2(N).copy()
    plain[only_padded] = 0.0
    special = plain.copy()
    special[only_padded] = np.resize([np.nan, np.inf, -np.inf], int(only_padded.sum()))
    ref = reference(capi, key, plain, tag="plain", u0=plain)
    G = in_mode(capi, key, R, monkeypatch, capfd, (LDS_DICT, None))
    for x in (plain, special):
        out = ST.outputs(capi, G, M, N, x, u0=plain)
        assert set(out) == {"spmv", "residual", "jacobi"} and G.x_window_kernel() == LDS_DICT
        for k in ref:
            XW.assert_same_bits(out[k], ref[k])
    assert all(np.isfinite(v).all() for v in ref.values())


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("dictionary", ["LDS", "scalar registers"])
def test_a_zero_row_keeps_its_sign(capi, dictionary, R, monkeypatch, capfd):
    """x = -0.0 over a stretch of rows, their right-hand side 0: every product there is a zero with a sign; k_sellp's bits, and a
    minus survives the Jacobi update"""
    key, want = (("band", 1, R), (LDS_DICT, None)) if dictionary == "LDS" else (("dict", "two values", R), (SCALAR_DICT, None))
    rows, cols, vals, M, N, A, x0 = make(key)
    x, rhs = inputs.v2(N).copy(), inputs.rhs2(M).copy()
    x[100:160], rhs[100:160] = -0.0, 0.0
    ref = reference(capi, key, x, rhs, tag="zeros")
    G = in_mode(capi, key, R, monkeypatch, capfd, want)
    out = ST.outputs(capi, G, M, N, x, rhs)
    for k in ref:
        XW.assert_same_bits(out[k], ref[k])
    assert (out["spmv"][100:158] == 0).all() and (out["jacobi"][100:158] == 0).all() and np.signbit(out["jacobi"][100:158]).any()


# ---- one non-temporal instantiation per dictionary treatment -------------------------------------------------------------------------------
def nt_hashes(capi):
    out = {}
    for key, R, kind in ((("band", 65, 256), 256, LDS_DICT), (("dict", "two values", 512), 512, SCALAR_DICT)):
        rows, cols, vals, M, N, A, x = make(key)
        G = util.gpu_operator(A)
        G.set_variant(17)
        G.set_x_windows(R)
        for k, a in ST.outputs(capi, G, M, N, x).items():
            out[f"{key[0]}/{R}/{k}"] = hashlib.sha256(XW.bits(a).tobytes()).hexdigest()
        out[f"{key[0]}/{R}/kernel"] = [G.x_window_kernel(), kind]
    return out


NT_WORKER = """
import json, sys
sys.path.insert(0, %(root)r)
from saena_amd import capi
from tests import test_gpu_vidxw_fast as T
capi.init(0)
print("RESULT " + json.dumps(T.nt_hashes(capi)))
"""


def test_the_non_temporal_instantiations_give_the_same_bits(capi, monkeypatch):
    """SAENA_SELLP_NT is read once per process: a child process with SAENA_SELLP_NT=1 runs k_vidxw_fast<NT> on operators far below the
    size where it switches on"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    monkeypatch.delenv("SAENA_VIDXW_FAST", raising=False)
    here = nt_hashes(capi)
    env = dict(os.environ, SAENA_SELLP_NT="1", SAENA_KEEP_HOST_VALUES="1")
    out = subprocess.run([sys.executable, "-c", NT_WORKER % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(here) == 8 and all(v[0] == v[1] for k, v in here.items() if k.endswith("kernel"))
    assert child == here, sorted(k for k in here if child.get(k) != here[k])
