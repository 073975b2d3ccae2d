"""A plain numpy restatement of the geometry the library decides for the x-window launch mode of k_vidx (variant 17 +
set_x_windows(R)): what build_sell_values, build_sellp_mode(rowbase = false), build_vidx and build_xwin compute on the host, from the
operator's structure alone.  The GPU tests hold the library's reported geometry to it, and tests/test_xwin_ref.py pins it for the named
operators below, so a test written for one path of the kernel cannot silently run another.

The named operators are diagonals at fixed offsets (optionally over a row range, with some rows left empty): the structure only -- the
tests attach the values."""
import numpy as np

ROWS = (256, 512, 1024)
SP_MAX_TABLE = 4096                     # ints of ONE pattern table (more: per-workgroup tables, which the mode refuses)
SELL_PAD = 1.12                         # padding of the slices of 64 rows the pattern forms accept
SPX_MAXWIN = 16
VW_MAX_LDS = 64 * 1024
VI_MAX = 256                            # distinct values of a dictionary (one per 256 rows), 8 B each

OK = "ok"
TOO_MANY_WINDOWS = "more windows than SPX_MAXWIN"
LDS_CAP = "exceed the LDS cap"


def structure(rows, cols, M):
    """what does not depend on R, from one pass over the rows: -> dict
      lens      row lengths
      patterns  [(offsets relative to the row index, columns ascending)], in order of first appearance (build_sellp_mode)
      npat, W   their count and the longest row (at least 1)
      one_table npat * (W + 1) <= SP_MAX_TABLE
      padding   stored positions of the slices of 64 rows / entries (build_sell_values)
      w8        the slices' widths in groups of 8 positions, per slice (build_vidx)
      uniform   all slices one width (a narrower LAST slice is padded up): the kernel then reads a.uw, else a.vcptr
      offsets   the sorted distinct offsets of all patterns"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    lens = np.bincount(rows, minlength=M)
    rp = np.concatenate([[0], np.cumsum(lens)])
    rel = cols - rows
    ids, patterns = {}, []
    for r in range(M):
        key = tuple(rel[rp[r]:rp[r + 1]].tolist())
        if key not in ids:
            ids[key] = len(patterns)
            patterns.append(key)
    W = max(1, int(lens.max()) if M else 1)
    ns = (M + 63) // 64
    widths = [int(lens[s * 64:min(M, s * 64 + 64)].max()) for s in range(ns)]
    w8 = [(w + 7) & ~7 for w in widths]
    uniform = w8[0] > 0 and all(w == w8[0] or (s == ns - 1 and w < w8[0]) for s, w in enumerate(w8))
    return dict(lens=lens, patterns=patterns, npat=len(patterns), W=W, one_table=len(patterns) * (W + 1) <= SP_MAX_TABLE,
                padding=64.0 * sum(widths) / max(1, len(rows)), w8=w8, uniform=uniform,
                offsets=sorted({o for p in patterns for o in p}), nnz=len(rows))


def windows(offsets, R):
    """build_xwin's clusters: a gap of MORE than R columns between neighbouring offsets begins a new window -> [(omin, omax)]"""
    out = []
    for i, o in enumerate(offsets):
        if i == 0 or o - offsets[i - 1] > R:
            out.append([o, o])
        else:
            out[-1][1] = o
    return [tuple(w) for w in out]


def geometry(rows, cols, M, N, R, st=None):
    """-> dict: structure()'s fields (pass `st` to reuse them across R) and, for workgroups of R rows,
      windows   [(omin, omax)]; nwin their count
      S         doubles of x a workgroup stages: sum of R + omax - omin
      passes    staging passes of 4 R elements: ceil(S / 4R)
      lds       bytes: windows (+ the spare slot, rounded to 16 B), R / 256 dictionaries, the table as 16-bit words
      clamped   some window of some workgroup leaves [0, N): the kernel clamps against the COLUMN count
      verdict   OK, or the reason build_xwin gives"""
    st = structure(rows, cols, M) if st is None else st
    g = dict(st)
    assert st["one_table"] and st["padding"] <= SELL_PAD and st["offsets"], "not an operator of the value-indexed form"
    win = windows(st["offsets"], R)
    S = sum(R + hi - lo for lo, hi in win)
    wp, lp = (st["W"] + 7) & ~7, (st["npat"] + 7) & ~7
    words = lp + st["npat"] * wp
    lds = ((S + 2) & ~1) * 8 + (R // 256) * VI_MAX * 8 + 2 * words
    last_r0 = (M - 1) // R * R
    g.update(R=R, windows=win, nwin=len(win), S=S, passes=-(-S // (4 * R)), words=words, lds=lds,
             clamped=win[0][0] < 0 or last_r0 + R + win[-1][1] > N,
             verdict=TOO_MANY_WINDOWS if len(win) > SPX_MAXWIN else LDS_CAP if lds > VW_MAX_LDS else OK)
    return g


def setup_line(g):
    """the fields of the library's line "x windows for the value-indexed form: workgroups of R rows, n windows, S doubles of x ... = K
    KiB of LDS" (SAENA_SETUP_TIMING=1) -> (R, n, S, "K")"""
    return g["R"], g["nwin"], g["S"], "%.1f" % (g["lds"] / 1024.0)


# ---- the named operators: name -> (M, N, [(offsets, first row, end row)], empty rows or None)
def _spec(M, offsets, N=None, pieces=None, empty=None):
    return M, M if N is None else N, pieces if pieces is not None else [(list(offsets), 0, M)], empty


OPERATORS = {
    "wide19": _spec(5000, range(-9, 10)),                                   # rows of 19 entries: three turns of the row loop
    "steps": _spec(6000, None, pieces=[(list(range(-2, 3)), 0, 3000), (list(range(-6, 7)), 3000, 6000)]),      # slices of two widths
    "four": _spec(12000, [-3000, -1500, 0, 1500]),                          # the fourth window's register slot
    "five": _spec(12000, [-3000, -1500, 0, 1500, 3000]),                    # one window from the table's loop, two staging passes
    "seven": _spec(12000, [-4500, -3000, -1500, 0, 1500, 3000, 4500]),      # the LDS cap at 1024 rows
    "sixteen": _spec(20000, [1100 * k for k in range(-8, 8)]),              # the most windows, four staging passes
    "seventeen": _spec(20000, [1100 * k for k in range(-8, 9)]),            # one window too many at every R
    "comb": _spec(8000, [200 * k for k in range(-5, 6)]),                   # one wide window: three staging passes at 256 rows
    "gaps": _spec(6000, [-1025, -513, -257, 0, 256, 512, 1024]),            # gaps of exactly R (merge) and R + 1 (split)
    "tall": _spec(3700, [-700, -350, 0], N=3000),                           # fewer columns than rows
    "flat": _spec(3000, [0, 350, 700], N=3700),                             # more columns than rows
    "holes": _spec(4000, [-1, 0, 1], empty=(20, 7)),                        # rows r % 20 == 7 hold no entry
    "tiny": _spec(60, [-1, 0, 1]),                                          # one partial slice, waves without a slice
}
_COO, _STRUCT, _GEOM = {}, {}, {}


def operator(name):
    """-> (rows, cols, M, N), row-major with columns ascending"""
    if name not in _COO:
        M, N, pieces, empty = OPERATORS[name]
        rr, cc = [], []
        for offsets, lo, hi in pieces:
            r = np.arange(lo, hi)
            if empty is not None:
                r = r[r % empty[0] != empty[1]]
            for o in offsets:
                k = r[(r + o >= 0) & (r + o < N)]
                rr.append(k); cc.append(k + o)
        rows, cols = np.concatenate(rr), np.concatenate(cc)
        order = np.lexsort((cols, rows))
        _COO[name] = (rows[order].astype(np.int32), cols[order].astype(np.int32), M, N)
        for a in _COO[name][:2]:
            a.setflags(write=False)
    return _COO[name]


def named_structure(name):
    if name not in _STRUCT:
        rows, cols, M, N = operator(name)
        _STRUCT[name] = structure(rows, cols, M)
    return _STRUCT[name]


def named_geometry(name, R):
    """geometry() of a named operator, computed once"""
    if (name, R) not in _GEOM:
        rows, cols, M, N = operator(name)
        _GEOM[(name, R)] = geometry(rows, cols, M, N, R, named_structure(name))
    return _GEOM[(name, R)]
