"""How k_vidxw (variant 17 + set_x_windows(R)) brings its windows of x into LDS -- window by window through range-checked buffer loads
(saena_amd/csrc/xwin_stage.h), or flat where the rule refuses -- and how its row loop treats positions below the shortest and beyond
the longest pattern.  None of that may change a bit: every case compares the mode with k_sellp (variant 11) on the same operator, bit
for bit, for the product, the residual and two Jacobi sweeps, at R = 256, 512 and 1024.

The operators are a few thousand rows at most and made for one path each; what puts an operator on its path (its windows, their sizes,
the trips, the pattern lengths) is computed here from its entries and asserted, and the library's own line says which staging it took,
so a case cannot silently run another path."""
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
from tests import test_gpu_x_windows as XW
from tests import xwin_ref as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = X.ROWS
_STAGED = re.compile(r"x windows for the value-indexed form: workgroups of (\d+) rows, .*; staged (window by window|flat) \((\d+) trips\)")


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


# ---- operators: diagonals at fixed offsets of an M x N operator, some rows left empty -> (rows, cols, vals, M, N) ---------------------
def diagonals(M, offsets, N=None, empty=None, second=None):
    """the diagonals at `offsets`; second: the offsets of the rows from M / 2 on, where they differ"""
    N = M if N is None else N
    rr, cc = [], []
    for offs, lo, hi in ((offsets, 0, M),) if second is None else ((offsets, 0, M // 2), (second, M // 2, M)):
        r = np.arange(lo, hi)
        if empty is not None:
            r = r[r % empty[0] != empty[1]]
        rr += [r[(r + o >= 0) & (r + o < N)] for o in offs]
        cc += [r[(r + o >= 0) & (r + o < N)] + o for o in offs]
    rr, cc = np.concatenate(rr), np.concatenate(cc)
    order = np.lexsort((cc, rr))
    rows, cols = rr[order], cc[order]
    return rows, cols, np.asarray(XW.VALS5)[np.arange(len(rows)) % 5], M, N


def band(k, R):
    """two offsets {0, k}: one window of R + k doubles; M = 3 R + 17: a partial last workgroup, and (k no multiple of 64) a last trip
    that fills part of a wave"""
    return diagonals(3 * R + 17, sorted({0, k}))


def named(name):
    rows, cols, M, N = X.operator(name)
    return rows, cols, np.asarray(XW.VALS5)[np.arange(len(rows)) % 5], M, N


OPERATORS = {
    "ends": lambda: diagonals(4000, [-1500, 0, 1500]),                                    # three windows that leave x at both ends
    "six": lambda: diagonals(5000, [-2000, -1999, 0, 1, 2000, 2001]),                     # three windows of R + 1: six trips
    "tall": lambda: named("tall"), "flat": lambda: named("flat"), "four": lambda: named("four"), "five": lambda: named("five"),
    "len8": lambda: diagonals(3000, range(0, 8), second=range(-7, 1)),                    # every row 8 entries: lmin = lmax = 8
    "len9": lambda: diagonals(3000, range(-4, 5)),                                        # 5 ... 9 entries: a second trip of one position
    "len16": lambda: diagonals(3000, range(-8, 8)),                                       # 8 ... 16: a full second trip
    "len3": lambda: diagonals(3000, [0, 1, 2], second=[-2, -1, 0]),                       # lmin = lmax = 3
    "holes": lambda: diagonals(3000, [-1, 0, 1], empty=(20, 7)),                          # lmin = 0
    "pad": lambda: diagonals(3000, [0, 20], empty=(20, 7)),                               # columns that only padded positions read
}
_OPS, _REF = {}, {}


def make(key):
    if key not in _OPS:
        rows, cols, vals, M, N = band(*key[1:]) if key[0] == "band" else OPERATORS[key[0]]()
        e = orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), vals)
        A = orc.OracleOp(e, M, N, orc.split_even(M, 1)) if M == N else orc.OracleOp(e, M, N, orc.split_even(M, 1), orc.split_even(N, 1), square=False)
        x = inputs.v2(N).copy()
        x[N // 3], x[2 * N // 3 + 1] = np.nan, np.inf
        x.setflags(write=False)
        _OPS[key] = (rows, cols, vals, M, N, A, x)
    return _OPS[key]


def outputs(capi, G, M, N, x, rhs=None, u0=None):
    dx, dy = capi.DeviceVector(N, x), capi.DeviceVector(M)
    out = {}
    G.spmv(dx, dy)
    out["spmv"] = dy.download()
    if M == N:
        dr = capi.DeviceVector(M, inputs.rhs2(M) if rhs is None else rhs)
        G.residual(dx, dr, dy)
        out["residual"] = dy.download()
        du = capi.DeviceVector(M, x if u0 is None else u0)
        G.jacobi(2, du, dr)
        out["jacobi"] = du.download()
    return out


def reference(capi, key, x=None, rhs=None, tag=None, u0=None):
    """k_sellp's outputs, computed once per (operator, inputs) and left unchanged"""
    if (key, tag) not in _REF:
        rows, cols, vals, M, N, A, x0 = make(key)
        G = util.gpu_operator(A)
        G.set_variant(11)
        assert G.variant() == (11, "k_sellp")
        _REF[(key, tag)] = outputs(capi, G, M, N, x0 if x is None else x, rhs, u0)
        for v in _REF[(key, tag)].values():
            v.setflags(write=False)
    return _REF[(key, tag)]


def in_mode(capi, key, R, monkeypatch, capfd, staged, trips=None):
    """the operator on variant 17 with windows of R rows, on the staging the case is written for"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    monkeypatch.setenv("SAENA_SETUP_TIMING", "1")
    rows, cols, vals, M, N, A, x = make(key)
    g = X.geometry(rows, cols, M, N, R)
    assert g["verdict"] == X.OK
    want_trips = sum(-(-(R + hi - lo) // R) for lo, hi in g["windows"]) if g["nwin"] <= 4 and g["S"] <= 4 * R else 0
    assert (want_trips > 0) == (staged == "window by window") and (trips is None or want_trips == trips), (g["windows"], want_trips)
    G = util.gpu_operator(A)
    G.set_variant(17)
    capfd.readouterr()
    G.set_x_windows(R)
    assert G.x_windows() == R and G.variant() == (17, "k_vidx")
    m = _STAGED.search(capfd.readouterr().err)
    assert m and (int(m.group(1)), m.group(2), int(m.group(3))) == (R, staged, want_trips), m and m.groups()
    return G, g


def check(capi, key, R, monkeypatch, capfd, staged="window by window", trips=None):
    rows, cols, vals, M, N, A, x = make(key)
    ref = reference(capi, key)
    G, g = in_mode(capi, key, R, monkeypatch, capfd, staged, trips)
    out = outputs(capi, G, M, N, x)
    assert set(out) == set(ref)
    for k in ref:
        XW.assert_same_bits_or_nan(out[k], ref[k])
    reached = np.zeros(M, bool)                               # the NaN and the Inf reach the rows that hold their columns, no other
    reached[rows[np.isin(cols, np.flatnonzero(~np.isfinite(x)))]] = True
    assert reached.any()
    np.testing.assert_array_equal(~np.isfinite(out["spmv"]), reached)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(out["spmv"][~reached], A.matvec(x)[~reached])
    return g


# ---- A: the windows, trip by trip ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("k", ["0", "1", "63", "64", "65", "R-1", "R"])
def test_one_window_of_every_size_up_to_two_trips(capi, k, R, monkeypatch, capfd):
    kk = {"R-1": R - 1, "R": R}.get(k) if k.startswith("R") else int(k)
    g = check(capi, ("band", kk, R), R, monkeypatch, capfd, trips=1 if kk == 0 else 2)
    assert g["windows"] == [(0, kk)] and g["S"] == R + kk and make(("band", kk, R))[3] % R == 17


@pytest.mark.parametrize("R", ROWS)
def test_windows_that_leave_the_vector_at_both_ends(capi, R, monkeypatch, capfd):
    g = check(capi, ("ends",), R, monkeypatch, capfd, trips=3)
    assert g["windows"] == [(-1500, -1500), (0, 0), (1500, 1500)] and g["clamped"]


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name", ["tall", "flat"])
def test_fewer_and_more_columns_than_rows(capi, name, R, monkeypatch, capfd):
    g = check(capi, (name,), R, monkeypatch, capfd)
    assert make((name,))[3] != make((name,))[4] and g["clamped"]


@pytest.mark.parametrize("R", ROWS)
def test_four_windows_are_staged_one_by_one_and_five_flat(capi, R, monkeypatch, capfd):
    assert check(capi, ("four",), R, monkeypatch, capfd, trips=4)["S"] == 4 * R
    assert check(capi, ("five",), R, monkeypatch, capfd, staged="flat")["nwin"] == 5


@pytest.mark.parametrize("R", ROWS)
def test_six_trips(capi, R, monkeypatch, capfd):
    assert check(capi, ("six",), R, monkeypatch, capfd, trips=6)["S"] == 3 * R + 3


# ---- B: the shortest and the longest pattern -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name,lmin,lmax", [("len3", 3, 3), ("len8", 8, 8), ("len9", 5, 9), ("len16", 8, 16), ("holes", 0, 3)])
def test_pattern_lengths_at_every_branch_of_the_row_loop(capi, name, lmin, lmax, R, monkeypatch, capfd):
    rows, cols, vals, M, N, A, x = make((name,))
    lens = np.bincount(rows, minlength=M)
    assert (lens.min(), lens.max()) == (lmin, lmax)
    check(capi, (name,), R, monkeypatch, capfd)


@pytest.mark.parametrize("R", ROWS)
def test_specials_where_only_padded_positions_read(capi, R, monkeypatch, capfd):
    """offsets {0, 20}, the rows r = 7 (mod 20) empty: no entry holds a column c = 7 (mod 20), but the empty row c reads it at every
    padded position (its pattern repeats position 0 of the first window, which is its own column).  NaN and +-Inf there change no
    product and no residual, and no Jacobi sweep that begins at a finite u"""
    key = ("pad",)
    rows, cols, vals, M, N, A, x0 = make(key)
    only_padded = np.arange(N) % 20 == 7
    assert not np.isin(cols, np.flatnonzero(only_padded)).any() and np.bincount(rows, minlength=M).min() == 0
    plain = inputs.v2(N).copy()
    plain[only_padded] = 0.0
    special = plain.copy()
    special[only_padded] = np.resize([np.nan, np.inf, -np.inf], int(only_padded.sum()))
    ref = reference(capi, key, plain, tag="plain", u0=plain)
    G, g = in_mode(capi, key, R, monkeypatch, capfd, "window by window")
    for x in (plain, special):                                # (the sweeps begin at the plain vector: u is an operand of its own)
        out = outputs(capi, G, M, N, x, u0=plain)
        assert set(out) == {"spmv", "residual", "jacobi"}
        for k in ref:
            XW.assert_same_bits(out[k], ref[k])
    assert all(np.isfinite(v).all() for v in ref.values())


@pytest.mark.parametrize("R", ROWS)
def test_a_zero_row_keeps_its_sign(capi, R, monkeypatch, capfd):
    """x = -0.0 over a stretch of rows, their right-hand side 0: every product there is a zero with a sign, the Jacobi update of such a
    row is -0.0 - (+-0.0): k_sellp's bits, and a minus survives"""
    key = ("band", 1, R)
    rows, cols, vals, M, N, A, x0 = make(key)
    x, rhs = inputs.v2(N).copy(), inputs.rhs2(M).copy()
    x[100:160], rhs[100:160] = -0.0, 0.0
    ref = reference(capi, key, x, rhs, tag="zeros")
    G, g = in_mode(capi, key, R, monkeypatch, capfd, "window by window")
    out = outputs(capi, G, M, N, x, rhs)
    for k in ref:
        XW.assert_same_bits(out[k], ref[k])
    # (rows 100 ... 157: their columns are zeros in both sweeps; a row whose scaled diagonal is positive ends at -0.0 - (+0.0))
    assert (out["spmv"][100:158] == 0).all() and (out["jacobi"][100:158] == 0).all() and np.signbit(out["jacobi"][100:158]).any()


# ---- one HALO and one non-temporal instantiation ---------------------------------------------------------------------------------------
def test_the_interior_launch_of_an_emulated_world(capi, monkeypatch):
    """the diagonals {0, 65} of 5000 rows split over two ranks on one device: the interior launch (HALO) masks the boundary rows; k_sellp's bits"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    rows, cols, vals, M, N = diagonals(5000, [0, 65])
    e = orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), vals)
    assert XW._halo_world(capi, ("staging", "band65"), e, M, 2, 256, False)


def nt_hashes(capi):
    out = {}
    for key, R in ((("band", 65, 256), 256), (("six",), 512)):
        rows, cols, vals, M, N, A, x = make(key)
        G = util.gpu_operator(A)
        G.set_variant(17)
        G.set_x_windows(R)
        for k, a in outputs(capi, G, M, N, x).items():
            out[f"{key[0]}/{R}/{k}"] = hashlib.sha256(XW.bits(a).tobytes()).hexdigest()
    return out


NT_WORKER = """
import json, sys
sys.path.insert(0, %(root)r)
from saena_amd import capi
from tests import test_gpu_vidxw_staging as T
capi.init(0)
print("RESULT " + json.dumps(T.nt_hashes(capi)))
"""


def test_the_non_temporal_instantiation_gives_the_same_bits(capi, monkeypatch):
    """SAENA_SELLP_NT is read once per process: a child process with SAENA_SELLP_NT=1 runs k_vidxw<NT> on operators far below the
    size where it switches on"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    here = nt_hashes(capi)
    env = dict(os.environ, SAENA_SELLP_NT="1", SAENA_KEEP_HOST_VALUES="1")
    out = subprocess.run([sys.executable, "-c", NT_WORKER % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(here) == 6 and child == here, sorted(k for k in here if child.get(k) != here[k])
