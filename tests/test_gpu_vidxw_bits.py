"""The bit codes of k_vidxw_fast (saena_amd/csrc/vw_fast.h): where the dictionaries of an operator hold at most two values the lean
kernel of the x-window mode (variant 17 + set_x_windows(R)) streams one bit per entry instead of an 8-bit code.  Product order and
operands are unchanged, so every case holds the product, the residual and two Jacobi sweeps to k_sellp (variant 11) bit for bit and to
a plain fp64 row loop (numpy, one position at a time in column order; the sweeps: the oracle's), at R = 256 and 512, on operators of
3 R + 17 rows -- a partial workgroup, a partial slice, spare waves -- unless a case says otherwise.

Which kernel and which code format an operator takes is restated here from its entries and asserted from the line the library prints
behind its x-window lines (SAENA_SETUP_TIMING: the format and both byte counts) and from sgpu_op_get_x_window_code_width before and
after the launches, so no case can silently run on the other format."""
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
_WIDTH = re.compile(r"x windows at (\d+) rows: codes of (?:1 bit per entry, (\d+) bytes packed from (\d+) bytes of 8-bit codes"
                    r"|8 bits per entry \((.*)\), (\d+) bytes, 1-bit codes would take (\d+))")
NOT_SCALAR, SWITCHED_OFF = "the dictionaries are in LDS", "SAENA_VIDXW_BITS=0"
NAN_PAYLOAD = np.array([0x7ff8000000abc123], np.uint64).view(np.float64)[0]
A_, B_ = 4.0, -1.25


# ---- operators: (rows, cols, vals, M, N), row-major with columns ascending; pos: an entry's position in its row ------------------------
def entries(M, offsets, value_of, N=None, empty=None):
    rows, cols, _, M, N = ST.diagonals(M, sorted(offsets), N=N, empty=empty)
    first = np.searchsorted(rows, rows)                               # (rows ascending: where each entry's row begins)
    pos = np.arange(len(rows)) - first
    return rows, cols, np.ascontiguousarray(value_of(rows, pos, cols), np.float64), M, N


def parity(a, b):
    """a, b by the parity of row + position: neighbouring lanes, neighbouring positions and -- a slice has 64 rows, its rows begin at
    position 0 -- the same lane of neighbouring turns carry different codes; code 0 of a group is its first row's first value"""
    return lambda r, p, c: np.where((r + p) % 2 == 0, a, b)


SEVEN = (-300, -20, -1, 0, 1, 20, 300)                                # 7-point-like: rows of 4 ... 7 entries
WIDE = tuple(range(-9, 10))                                           # tests/xwin_ref.py's wide19: rows of up to 19 entries, three turns


def turn_marks(r, p, c):
    """positions 7 / 8 and 15 / 16 differ (the byte order across turns) and a turn's eight bits 0 1 1 0 1 0 0 0 (+ the turn) read the
    same in no other bit order; the diagonal stays non-zero"""
    return np.where((p // 8 + np.isin(p % 8, (1, 2, 4))) % 2 == 0, A_, B_)


def per_group(r, p, c):
    """two values that differ from one group of 256 rows to the next: at R = 512 two dictionaries per workgroup"""
    g = r // 256
    return np.where((r + p) % 2 == 0, 1.0 + g, -0.5 - 0.25 * g)


OPERATORS = {
    "seven": lambda R: entries(3 * R + 17, SEVEN, parity(A_, B_)),
    "wide19": lambda R: entries(3 * R + 17, WIDE, turn_marks),
    "one value": lambda R: entries(3 * R + 17, SEVEN, lambda r, p, c: np.full(len(r), 2.5)),
    "per group": lambda R: entries(3 * R + 17, SEVEN, per_group),
    # (the library, like the reference, refuses a zero on the diagonal: the signed zeros come without the diagonal's contract)
    "signed zeros": lambda R: entries(3 * R + 17, (0, 1), parity(0.0, -0.0)),
    # rows r = 7 (mod 40) are empty, so the columns c = 7 (mod 40) are read by padded positions alone (one row in 40: with the partial
    # last slice the operator stays within the padding the sliced-ELLPACK values accept)
    "nan dictionary": lambda R: entries(3 * R + 17, (-40, 0), lambda r, p, c: np.where(c == r, 1.5, NAN_PAYLOAD), empty=(40, 7)),
    "inf dictionary": lambda R: entries(3 * R + 17, (-40, 0), lambda r, p, c: np.where(c == r, np.inf, -np.inf), empty=(40, 7)),
    "whole slices": lambda R: entries(64 * 5, SEVEN, parity(A_, B_)),                     # M = 64 k: 320 rows, two workgroups at 256 (one slice in the last), one at 512
    "whole workgroups": lambda R: entries(3 * R, SEVEN, parity(A_, B_)),
    # (64 stored positions for one entry: the sliced-ELLPACK values under every row-pattern form refuse that much padding unless
    # SAENA_SELL_PAD, read once per process, allows it -- this operator runs in a child process)
    "one row": lambda R: entries(1, (0,), lambda r, p, c: np.full(len(r), 3.0)),
    "three values": lambda R: entries(3 * R + 17, SEVEN, lambda r, p, c: np.asarray([A_, B_, 1.0 / 3.0])[(r + p) % 3]),
}
NO_DIAGONAL = ("signed zeros",)
_OPS, _REF = {}, {}


def make(name, R):
    if (name, R) not in _OPS:
        rows, cols, vals, M, N = OPERATORS[name](R)
        e = orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), vals)
        A = orc.OracleOp(e, M, N, orc.split_even(M, 1)) if name not in NO_DIAGONAL else \
            orc.OracleOp(e, M, N, orc.split_even(M, 1), orc.split_even(N, 1), square=False)
        x = inputs.v2(N).copy()
        if name.endswith("dictionary"):
            only_padded = np.arange(N) % 40 == 7
            assert not np.isin(cols, np.flatnonzero(only_padded)).any() and np.bincount(rows, minlength=M).min() == 0
            x[only_padded] = np.resize([np.nan, np.inf, -np.inf], int(only_padded.sum()))
        x.setflags(write=False)
        _OPS[(name, R)] = (rows, cols, vals, M, N, A, x)
    return _OPS[(name, R)]


def outputs(capi, name, G, M, N, x):
    """product, residual and two Jacobi sweeps (tests/test_gpu_vidxw_staging.py's); without an inverse diagonal: no sweeps"""
    if name not in NO_DIAGONAL:
        return ST.outputs(capi, G, M, N, x)
    dx, dy, dr = capi.DeviceVector(N, x), capi.DeviceVector(M), capi.DeviceVector(M, inputs.rhs2(M))
    out = {}
    G.spmv(dx, dy)
    out["spmv"] = dy.download()
    G.residual(dx, dr, dy)
    out["residual"] = dy.download()
    return out


def row_loop(rows, cols, vals, M, x):
    """the plain fp64 row loop: a row's products added one after the other in column order, the sum beginning at +0.0"""
    first = np.searchsorted(rows, np.arange(M))
    n = np.bincount(rows, minlength=M)
    y = np.zeros(M)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(n.max()) if M else 0):
            has = np.flatnonzero(n > j)
            y[has] = y[has] + vals[first[has] + j] * x[cols[first[has] + j]]
    return y


def reference(capi, name, R):
    """k_sellp's outputs and the row loop's, computed once per operator and left unchanged"""
    if (name, R) not in _REF:
        rows, cols, vals, M, N, A, x = make(name, R)
        G = util.gpu_operator(A)
        G.set_variant(11)
        assert G.variant() == (11, "k_sellp")
        sellp = outputs(capi, name, G, M, N, x)
        y = row_loop(rows, cols, vals, M, x)
        with np.errstate(invalid="ignore", over="ignore"):
            loop = {"spmv": y, "residual": y - inputs.rhs2(M)}
            if "jacobi" in sellp:
                loop["jacobi"] = A.jacobi(2, x, inputs.rhs2(M))
        for v in list(sellp.values()) + list(loop.values()):
            v.setflags(write=False)
        _REF[(name, R)] = (sellp, loop)
    return _REF[(name, R)]


# ---- the rule, restated from the operator's entries -------------------------------------------------------------------------------------
def expected(name, R):
    """-> (kernel, values per dictionary, slices, positions per slice)"""
    rows, cols, vals, M, N, A, x = make(name, R)
    g = X.geometry(rows, cols, M, N, R)
    assert g["verdict"] == X.OK and g["uniform"] and g["words"] // 8 <= R
    pat = np.ascontiguousarray(vals, np.float64).view(np.uint64)
    sizes = {len(set(pat[rows // 256 == b].tolist())) for b in range((M + 255) // 256)}
    assert len(sizes) == 1                                            # one dictionary length
    vd_u = sizes.pop()
    ntrip = sum(-(-(R + hi - lo) // R) for lo, hi in g["windows"]) if g["nwin"] <= 4 and g["S"] <= 4 * R else 0
    assert 1 <= ntrip <= 4
    return (SCALAR_DICT if vd_u <= 2 else LDS_DICT), vd_u, (M + 63) // 64, int(g["w8"][0])


def in_mode(capi, name, R, monkeypatch, capfd, width, why=None):
    """the operator on variant 17 with windows of R rows; the library's line and its getter name the code format"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    monkeypatch.setenv("SAENA_SETUP_TIMING", "1")
    monkeypatch.delenv("SAENA_VIDXW_FAST", raising=False)
    if why == SWITCHED_OFF:
        monkeypatch.setenv("SAENA_VIDXW_BITS", "0")
    else:
        monkeypatch.delenv("SAENA_VIDXW_BITS", raising=False)
    kernel, vd_u, ns, uw = expected(name, R)
    assert width == (1 if kernel == SCALAR_DICT and why != SWITCHED_OFF else 8)
    rows, cols, vals, M, N, A, x = make(name, R)
    G = util.gpu_operator(A)
    G.set_variant(17)
    assert G.x_window_code_width() == 8                               # (the mode is off: k_vidx reads the 8-bit codes)
    capfd.readouterr()
    G.set_x_windows(R)
    err = capfd.readouterr().err
    assert G.x_windows() == R and G.variant() == (17, "k_vidx") and G.x_window_kernel() == kernel
    m = _WIDTH.search(err)
    assert m and int(m.group(1)) == R, err[-1500:]
    if width == 1:
        assert (int(m.group(2)), int(m.group(3))) == (ns * 8 * uw, ns * 64 * uw), m.groups()
    else:
        assert (m.group(4), int(m.group(5)), int(m.group(6))) == (why, ns * 64 * uw, ns * 8 * uw), m.groups()
    assert G.x_window_code_width() == width
    return G


def check(capi, name, R, monkeypatch, capfd, width=1, why=None):
    rows, cols, vals, M, N, A, x = make(name, R)
    sellp, loop = reference(capi, name, R)
    G = in_mode(capi, name, R, monkeypatch, capfd, width, why)
    out = outputs(capi, name, G, M, N, x)
    assert G.x_window_code_width() == width and G.x_window_kernel() == expected(name, R)[0]      # what the last launch ran and read
    assert set(out) == set(sellp) == set(loop) and ("jacobi" in out or name in NO_DIAGONAL)
    for k in out:
        XW.assert_same_bits_or_nan(out[k], sellp[k])
        XW.assert_same_bits_or_nan(out[k], loop[k])
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(loop[k]))
    return out


# ---- 1, 2: the strides of lane, turn and slice; the bit order in a byte and the byte order across turns ---------------------------------
@pytest.mark.parametrize("R", ROWS)
def test_seven_point_like_rows_with_the_value_by_parity(capi, R, monkeypatch, capfd):
    rows, cols, vals, M, N, A, x = make("seven", R)
    n = np.bincount(rows, minlength=M)
    assert (n.min(), n.max()) == (4, 7) and M % R == 17
    out = check(capi, "seven", R, monkeypatch, capfd)
    assert np.isfinite(out["spmv"]).all()


@pytest.mark.parametrize("R", ROWS)
def test_three_turns_with_marks_at_the_turns_edges(capi, R, monkeypatch, capfd):
    rows, cols, vals, M, N, A, x = make("wide19", R)
    assert expected("wide19", R)[3] == 24 and np.bincount(rows).max() == 19
    long_row = vals[rows == 100]
    assert long_row[7] != long_row[8] and long_row[15] != long_row[16] and list(long_row[:8] == B_) == [False, True, True, False, True, False, False, False]
    check(capi, "wide19", R, monkeypatch, capfd)


# ---- 3, 4, 5: the dictionaries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
def test_dictionaries_of_one_value_every_bit_zero(capi, R, monkeypatch, capfd):
    assert expected("one value", R)[:2] == (SCALAR_DICT, 1)
    check(capi, "one value", R, monkeypatch, capfd)


@pytest.mark.parametrize("R", ROWS)
def test_dictionaries_that_differ_from_group_to_group(capi, R, monkeypatch, capfd):
    rows, cols, vals, M, N, A, x = make("per group", R)
    assert len(set(vals.tolist())) == 2 * ((M + 255) // 256) and expected("per group", R)[:2] == (SCALAR_DICT, 2)
    check(capi, "per group", R, monkeypatch, capfd)


@pytest.mark.parametrize("R", ROWS)
def test_signed_zeros(capi, R, monkeypatch, capfd):
    out = check(capi, "signed zeros", R, monkeypatch, capfd)
    assert (out["spmv"] == 0).all() and set(out) == {"spmv", "residual"}


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name", ["nan dictionary", "inf dictionary"])
def test_special_values_in_the_dictionary_and_specials_in_x_where_only_padded_positions_read(capi, name, R, monkeypatch, capfd):
    rows, cols, vals, M, N, A, x = make(name, R)
    assert (~np.isfinite(x)).sum() >= M // 40 and (~np.isfinite(vals)).any()
    out = check(capi, name, R, monkeypatch, capfd)
    empty = np.bincount(rows, minlength=M) == 0
    assert empty.sum() >= M // 40 and (XW.bits(out["spmv"][empty]) == 0).all()      # an empty row: +0.0 whatever its padded positions read
    if name == "nan dictionary":
        assert np.isnan(out["spmv"][40:][~empty[40:]]).all()                       # (every row that reaches column r - 40 holds the NaN)


# ---- 6: M = 64 k, M = 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name", ["whole slices", "whole workgroups"])
def test_whole_slices_and_whole_workgroups(capi, name, R, monkeypatch, capfd):
    M = make(name, R)[3]
    assert M == {"whole slices": 320, "whole workgroups": 3 * R}[name]
    check(capi, name, R, monkeypatch, capfd)


def one_row(capi):
    """M = 1 at both R against k_sellp and the row loop, in a process whose SAENA_SELL_PAD admits the operator -> what ran"""
    ran = []
    for R in ROWS:
        rows, cols, vals, M, N, A, x = make("one row", R)
        sellp, loop = reference(capi, "one row", R)
        G = util.gpu_operator(A)
        G.set_variant(17)
        G.set_x_windows(R)
        out = ST.outputs(capi, G, M, N, x)
        assert M == 1 and set(out) == set(sellp) == set(loop) == {"spmv", "residual", "jacobi"}
        for k in out:
            XW.assert_same_bits(out[k], sellp[k])
            XW.assert_same_bits(out[k], loop[k])
        ran.append([R, G.x_window_kernel(), G.x_window_code_width()])
    return ran


ONE_ROW_WORKER = """
import json, sys
sys.path.insert(0, %(root)r)
from saena_amd import capi
from tests import test_gpu_vidxw_bits as T
capi.init(0)
print("RESULT " + json.dumps(T.one_row(capi)))
"""


def test_one_row(capi):
    env = dict(os.environ, SAENA_KEEP_HOST_VALUES="1", SAENA_SETUP_TIMING="1", SAENA_SELL_PAD="64")
    env.pop("SAENA_VIDXW_BITS", None)
    env.pop("SAENA_VIDXW_FAST", None)
    out = subprocess.run([sys.executable, "-c", ONE_ROW_WORKER % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    ran = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert ran == [[R, SCALAR_DICT, 1] for R in ROWS]
    lines = [(int(m.group(1)), m.group(2), m.group(3)) for m in _WIDTH.finditer(out.stderr)]
    assert lines == [(R, "64", "512") for R in ROWS], out.stderr[-3000:]          # one slice of eight positions: 64 bytes of bits for 512 of codes


# ---- 8: three values keep the 8-bit codes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
def test_three_values_in_a_group_run_the_lds_dictionary_on_8_bit_codes(capi, R, monkeypatch, capfd):
    assert expected("three values", R)[:2] == (LDS_DICT, 3)
    check(capi, "three values", R, monkeypatch, capfd, width=8, why=NOT_SCALAR)


# ---- 7, 9: one non-temporal instantiation; the switch ---------------------------------------------------------------------------------------
def hashes(capi, width):
    out = {}
    for name, R in (("seven", 256), ("wide19", 512), ("per group", 512)):
        rows, cols, vals, M, N, A, x = make(name, R)
        G = util.gpu_operator(A)
        G.set_variant(17)
        G.set_x_windows(R)
        for k, a in ST.outputs(capi, G, M, N, x).items():
            out[f"{name}/{R}/{k}"] = hashlib.sha256(XW.bits(a).tobytes()).hexdigest()
        out[f"{name}/{R}/kernel and width"] = [G.x_window_kernel(), G.x_window_code_width(), SCALAR_DICT, width]
    return out


WORKER = """
import json, sys
sys.path.insert(0, %(root)r)
from saena_amd import capi
from tests import test_gpu_vidxw_bits as T
capi.init(0)
print("RESULT " + json.dumps(T.hashes(capi, %(width)d)))
"""


def in_child(env, width):
    out = subprocess.run([sys.executable, "-c", WORKER % dict(root=ROOT, width=width)], env=dict(os.environ, SAENA_KEEP_HOST_VALUES="1", **env),
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


_HERE = {}


def here(capi, monkeypatch):
    """this process's hashes on the bit codes, computed once"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    monkeypatch.delenv("SAENA_VIDXW_BITS", raising=False)
    monkeypatch.delenv("SAENA_VIDXW_FAST", raising=False)
    if not _HERE:
        _HERE.update(hashes(capi, 1))
    assert len(_HERE) == 12 and all(v[:2] == v[2:] for k, v in _HERE.items() if k.endswith("width"))
    return _HERE


def strip(h):
    return {k: v for k, v in h.items() if not k.endswith("width")}


def test_the_non_temporal_instantiation_gives_the_same_bits(capi, monkeypatch):
    """SAENA_SELLP_NT is read once per process: a child process with SAENA_SELLP_NT=1 runs k_vidxw_fast<NT, SD, BITS> on operators far
    below the size where it switches on"""
    mine = here(capi, monkeypatch)
    child = in_child({"SAENA_SELLP_NT": "1"}, 1)
    assert child == mine, sorted(k for k in mine if child.get(k) != mine[k])


def test_switched_off_in_a_child_process_the_8_bit_codes_give_the_same_bits(capi, monkeypatch):
    mine = here(capi, monkeypatch)
    child = in_child({"SAENA_VIDXW_BITS": "0"}, 8)
    assert all(v[:2] == v[2:] == [SCALAR_DICT, 8] for k, v in child.items() if k.endswith("width"))
    assert strip(child) == strip(mine), sorted(k for k in strip(mine) if child.get(k) != mine[k])


@pytest.mark.parametrize("R", ROWS)
def test_switched_off_per_operator_in_this_process(capi, R, monkeypatch, capfd):
    """the environment is read when the windows are built: one process runs both formats"""
    off = check(capi, "seven", R, monkeypatch, capfd, width=8, why=SWITCHED_OFF)
    on = check(capi, "seven", R, monkeypatch, capfd)
    for k in on:
        XW.assert_same_bits(on[k], off[k])


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c
