"""The mask rows of k_vidxw_fast (saena_amd/csrc/vw_masks.h): where the dictionaries stay in scalar registers, no pattern is longer
than eight positions and every pattern is an ordered subset of the longest one, the lean kernel of the x-window mode reads a slice of
64 rows as sixteen 64-bit lane masks in scalar registers -- no pattern id, no code, no table.  Products and their order are unchanged,
so every case holds the product, the residual and two Jacobi sweeps to k_sellp (variant 11) bit for bit and to a plain fp64 row loop
(tests/test_gpu_vidxw_bits.py's), at R = 256 and 512, on operators of 3 R + 17 rows unless a case says otherwise.

Which row format an operator takes is asserted from the line the library prints behind its x-window lines (SAENA_SETUP_TIMING) and
from sgpu_op_get_x_window_row_format before and after the launches, so no case can silently run on the other format."""
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
from tests import test_gpu_vidxw_bits as B
from tests import test_gpu_vidxw_staging as ST
from tests import test_gpu_x_windows as XW

pytestmark = pytest.mark.gpu

ROOT = B.ROOT
ROWS = B.ROWS
TABLE, MASKS = 0, 1
_ROWS = re.compile(r"x windows at (\d+) rows: (?:rows as lane masks, (\d+) bytes in (\d+) records of (\d+) slots|rows through the table \((.*)\))")
TURNS, NOT_SUBSEQUENCE, SWITCHED_OFF = "a pattern of more than eight positions", "a pattern is no ordered subset of the longest pattern", "SAENA_VIDXW_MASKS=0"
A_, B_ = B.A_, B.B_
EIGHT = (-300, -20, -1, 0, 1, 20, 21, 300)                          # (three windows in four trips at R = 256, as SEVEN has)
NINE = tuple(range(-4, 5))


def by_slot(r, p, c):
    """the diagonal one value, every other slot the other: a slice's value masks are all-or-nothing"""
    return np.where(c == r, A_, B_)


def halves(M):
    """rows of the first half hold columns r, r + 300, those of the second r - 300, r: no pattern holds all three slots"""
    rows, cols, _, M, N = ST.diagonals(M, [0, 300], second=[-300, 0])
    return rows, cols, np.where(cols == rows, A_, B_).astype(np.float64), M, N


def last_slice_empty(R):
    """3 R + 128 rows of which the last 64 hold nothing: a whole slice of empty rows -- the last one, so that the slices keep one
    width, behind a slice with rows, so that the last dictionary keeps its two values"""
    rows, cols, vals, M, N = B.entries(3 * R + 128, B.SEVEN, B.parity(A_, B_))
    keep = rows < 3 * R + 64
    return rows[keep], cols[keep], vals[keep], M, N


OPERATORS = {
    "by slot": lambda R: B.entries(3 * R + 17, B.SEVEN, by_slot),
    "eight slots": lambda R: B.entries(3 * R + 17, EIGHT, B.parity(A_, B_)),
    "one slot": lambda R: B.entries(3 * R + 17, (0,), lambda r, p, c: np.where(r % 2 == 0, A_, B_)),
    "last slice empty": last_slice_empty,
    # M = 64 k: thirteen slices, a last workgroup of one slice at R = 256 and of five at 512 (the 320 rows of the bit codes' case hold
    # no row with all seven slots)
    "thirteen slices": lambda R: B.entries(64 * 13, B.SEVEN, B.parity(A_, B_)),
    "nine positions": lambda R: B.entries(3 * R + 17, NINE, B.parity(A_, B_)),
    "no complete pattern": lambda R: halves(3 * R + 17),
}
_OPS, _REF = {}, {}


def make(name, R):
    if name in B.OPERATORS:
        return B.make(name, R)
    if (name, R) not in _OPS:
        rows, cols, vals, M, N = OPERATORS[name](R)
        e = orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), vals)
        A = orc.OracleOp(e, M, N, orc.split_even(M, 1))
        x = inputs.v2(N).copy()
        x.setflags(write=False)
        _OPS[(name, R)] = (rows, cols, vals, M, N, A, x)
    return _OPS[(name, R)]


def reference(capi, name, R):
    """k_sellp's outputs and the row loop's, computed once per operator and left unchanged"""
    if name in B.OPERATORS:
        return B.reference(capi, name, R)
    if (name, R) not in _REF:
        rows, cols, vals, M, N, A, x = make(name, R)
        G = util.gpu_operator(A)
        G.set_variant(11)
        assert G.variant() == (11, "k_sellp")
        sellp = ST.outputs(capi, G, M, N, x)
        y = B.row_loop(rows, cols, vals, M, x)
        loop = {"spmv": y, "residual": y - inputs.rhs2(M), "jacobi": A.jacobi(2, x, inputs.rhs2(M))}
        for v in list(sellp.values()) + list(loop.values()):
            v.setflags(write=False)
        _REF[(name, R)] = (sellp, loop)
    return _REF[(name, R)]


def in_mode(capi, name, R, monkeypatch, capfd, fmt, why=None):
    """the operator on variant 17 with windows of R rows; the library's line and its getter name the row format"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    monkeypatch.setenv("SAENA_SETUP_TIMING", "1")
    for v in ("SAENA_VIDXW_FAST", "SAENA_VIDXW_BITS", "SAENA_VIDXW_MASKS"):
        monkeypatch.delenv(v, raising=False)
    if why == SWITCHED_OFF:
        monkeypatch.setenv("SAENA_VIDXW_MASKS", "0")
    rows, cols, vals, M, N, A, x = make(name, R)
    G = util.gpu_operator(A)
    G.set_variant(17)
    assert G.x_window_row_format() == TABLE                           # (the mode is off)
    capfd.readouterr()
    G.set_x_windows(R)
    err = capfd.readouterr().err
    assert G.x_windows() == R and G.variant() == (17, "k_vidx") and G.x_window_kernel() == B.SCALAR_DICT
    m = _ROWS.search(err)
    assert m and int(m.group(1)) == R, err[-1500:]
    ns = (M + 63) // 64
    if fmt == MASKS:
        lmax = int(np.bincount(rows, minlength=M).max())
        assert (int(m.group(2)), int(m.group(3)), int(m.group(4))) == (128 * ns, ns, lmax), m.groups()
    else:
        assert m.group(5) == why, m.groups()
    assert G.x_window_row_format() == fmt and G.x_window_code_width() == 1      # a mask launch reports the bit codes' width
    return G


def check(capi, name, R, monkeypatch, capfd, fmt=MASKS, why=None):
    rows, cols, vals, M, N, A, x = make(name, R)
    sellp, loop = reference(capi, name, R)
    G = in_mode(capi, name, R, monkeypatch, capfd, fmt, why)
    out = B.outputs(capi, name, G, M, N, x)
    assert G.x_window_row_format() == fmt and G.x_window_kernel() == B.SCALAR_DICT and G.x_window_code_width() == 1      # what the last launch ran and read
    assert set(out) == set(sellp) == set(loop) and ("jacobi" in out or name in B.NO_DIAGONAL)
    for k in out:
        XW.assert_same_bits_or_nan(out[k], sellp[k])
        XW.assert_same_bits_or_nan(out[k], loop[k])
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(loop[k]))
    return out


def slices_of(rows, M, nslot):
    """-> per slice: rows that hold all nslot slots, rows that hold none"""
    n = np.bincount(rows, minlength=(M + 63) // 64 * 64).reshape(-1, 64)
    return (n == nslot).sum(axis=1), (n == 0).sum(axis=1)


# ---- full, partial and empty presence masks; partial and uniform value masks -----------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name", ["seven", "by slot"])
def test_seven_point_like_rows_whose_end_rows_lack_slots(capi, name, R, monkeypatch, capfd):
    """"seven": the value by the parity of row + position (partial value masks); "by slot": uniform ones.  The first and the last 300
    rows lack slots, those between hold all seven, the last slice has 17 rows: full, partial and (spare lanes) empty presence bits"""
    rows, cols, vals, M, N, A, x = make(name, R)
    full, none = slices_of(rows, M, 7)
    assert (full == 64).any() and ((full > 0) & (full < 64)).any() and (full == 0).any() and none[-1] == 64 - 17 and M % R == 17
    out = check(capi, name, R, monkeypatch, capfd)
    assert np.isfinite(out["spmv"]).all()


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name", ["eight slots", "one slot", "one value", "per group"])
def test_eight_slots_one_slot_and_the_dictionaries(capi, name, R, monkeypatch, capfd):
    rows, cols, vals, M, N, A, x = make(name, R)
    assert int(np.bincount(rows).max()) == {"eight slots": 8, "one slot": 1}.get(name, 7)
    check(capi, name, R, monkeypatch, capfd)


@pytest.mark.parametrize("R", ROWS)
def test_a_whole_slice_of_empty_rows_and_the_sign_of_a_zero_row(capi, R, monkeypatch, capfd):
    rows, cols, vals, M, N, A, x = make("last slice empty", R)
    assert M == 3 * R + 128 and slices_of(rows, M, 7)[1][-1] == 64
    out = check(capi, "last slice empty", R, monkeypatch, capfd)
    assert (XW.bits(out["spmv"][3 * R + 64:]) == 0).all()             # +0.0, not -0.0, whatever the absent slots read


@pytest.mark.parametrize("R", ROWS)
def test_signed_zeros(capi, R, monkeypatch, capfd):
    out = check(capi, "signed zeros", R, monkeypatch, capfd)
    assert (out["spmv"] == 0).all() and set(out) == {"spmv", "residual"}


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name", ["nan dictionary", "inf dictionary"])
def test_special_dictionary_values_and_specials_in_x_where_only_absent_slots_read(capi, name, R, monkeypatch, capfd):
    rows, cols, vals, M, N, A, x = make(name, R)
    assert (~np.isfinite(x)).sum() >= M // 40 and (~np.isfinite(vals)).any()
    out = check(capi, name, R, monkeypatch, capfd)
    empty = np.bincount(rows, minlength=M) == 0
    assert empty.sum() >= M // 40 and (XW.bits(out["spmv"][empty]) == 0).all()      # an empty row: +0.0 whatever its absent slots read


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name", ["thirteen slices", "whole workgroups"])
def test_whole_slices_and_whole_workgroups(capi, name, R, monkeypatch, capfd):
    assert make(name, R)[3] == {"thirteen slices": 832, "whole workgroups": 3 * R}[name]
    check(capi, name, R, monkeypatch, capfd)


# ---- the refusals that still run, and the switch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("name,why", [("nine positions", TURNS), ("no complete pattern", NOT_SUBSEQUENCE)])
def test_refused_operators_run_through_the_table_and_give_the_same_bits(capi, name, why, R, monkeypatch, capfd):
    rows, cols, vals, M, N, A, x = make(name, R)
    assert int(np.bincount(rows).max()) == (9 if name == "nine positions" else 2)
    check(capi, name, R, monkeypatch, capfd, fmt=TABLE, why=why)


@pytest.mark.parametrize("R", ROWS)
def test_switched_off_per_operator_in_this_process(capi, R, monkeypatch, capfd):
    """the environment is read when the windows are built: one process runs both formats"""
    off = check(capi, "seven", R, monkeypatch, capfd, fmt=TABLE, why=SWITCHED_OFF)
    on = check(capi, "seven", R, monkeypatch, capfd)
    for k in on:
        XW.assert_same_bits(on[k], off[k])


# ---- child processes: M = 1, one non-temporal instantiation, the switch --------------------------------------------------------------------
def one_row(capi):
    ran = B.one_row(capi)                                             # (holds M = 1 at both R to k_sellp and the row loop)
    fmt = []
    for R in ROWS:
        rows, cols, vals, M, N, A, x = B.make("one row", R)
        G = util.gpu_operator(A)
        G.set_variant(17)
        G.set_x_windows(R)
        ST.outputs(capi, G, M, N, x)
        fmt.append([R, G.x_window_row_format()])
    return ran, fmt


def hashes(capi, fmt):
    out = {}
    for name, R in (("seven", 256), ("by slot", 512), ("eight slots", 512)):
        rows, cols, vals, M, N, A, x = make(name, R)
        G = util.gpu_operator(A)
        G.set_variant(17)
        G.set_x_windows(R)
        for k, a in ST.outputs(capi, G, M, N, x).items():
            out[f"{name}/{R}/{k}"] = hashlib.sha256(XW.bits(a).tobytes()).hexdigest()
        out[f"{name}/{R}/format"] = [G.x_window_kernel(), G.x_window_row_format(), B.SCALAR_DICT, fmt]
    return out


WORKER = """
import json, sys
sys.path.insert(0, %(root)r)
from saena_amd import capi
from tests import test_gpu_vidxw_masks as T
capi.init(0)
print("RESULT " + json.dumps(T.%(call)s))
"""


def in_child(env, call):
    full = dict(os.environ, SAENA_KEEP_HOST_VALUES="1", SAENA_SETUP_TIMING="1")
    for v in ("SAENA_VIDXW_FAST", "SAENA_VIDXW_BITS", "SAENA_VIDXW_MASKS"):
        full.pop(v, None)
    full.update(env)
    out = subprocess.run([sys.executable, "-c", WORKER % dict(root=ROOT, call=call)], env=full, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]), out.stderr


def test_one_row(capi):
    (ran, fmt), err = in_child({"SAENA_SELL_PAD": "64"}, "one_row(capi)")
    assert ran == [[R, B.SCALAR_DICT, 1] for R in ROWS] and fmt == [[R, MASKS] for R in ROWS]
    lines = [(int(m.group(1)), m.group(2), m.group(3), m.group(4)) for m in _ROWS.finditer(err)]
    assert lines == [(R, "128", "1", "1") for _ in range(2) for R in ROWS], err[-3000:]      # one record of one slot, built twice per R


_HERE = {}


def here(capi, monkeypatch):
    """this process's hashes on the mask rows, computed once"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    for v in ("SAENA_VIDXW_FAST", "SAENA_VIDXW_BITS", "SAENA_VIDXW_MASKS"):
        monkeypatch.delenv(v, raising=False)
    if not _HERE:
        _HERE.update(hashes(capi, MASKS))
    assert len(_HERE) == 12 and all(v[:2] == v[2:] for k, v in _HERE.items() if k.endswith("format"))
    return _HERE


def strip(h):
    return {k: v for k, v in h.items() if not k.endswith("format")}


def test_the_non_temporal_instantiation_gives_the_same_bits(capi, monkeypatch):
    """SAENA_SELLP_NT is read once per process: a child process with SAENA_SELLP_NT=1 runs k_vidxw_fast<NT, SD, BITS, MASKS> on
    operators far below the size where it switches on"""
    mine = here(capi, monkeypatch)
    child, _ = in_child({"SAENA_SELLP_NT": "1"}, "hashes(capi, %d)" % MASKS)
    assert child == mine, sorted(k for k in mine if child.get(k) != mine[k])


def test_switched_off_in_a_child_process_the_table_rows_give_the_same_bits(capi, monkeypatch):
    mine = here(capi, monkeypatch)
    child, _ = in_child({"SAENA_VIDXW_MASKS": "0"}, "hashes(capi, %d)" % TABLE)
    assert all(v[:2] == v[2:] == [B.SCALAR_DICT, TABLE] for k, v in child.items() if k.endswith("format"))
    assert strip(child) == strip(mine), sorted(k for k in strip(mine) if child.get(k) != mine[k])


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c
