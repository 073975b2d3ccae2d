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


# ---- the plans of saena_amd/csrc/xwin_plan.h, restated: what build_xwin uploads and keeps, what build_sellpx uploads ----
INT32_MAX = 2 ** 31 - 1
SPX_ROWS, SPX_LDS_BYTES = 512, 80 * 1024
DESC_COLS = 1 << 28                     # xwin_stage.h: columns whose byte offsets stay below 2^31
# build_xwin's refusals, in the order it checks them
PATTERN_LENGTH, NO_ENTRIES = "a pattern longer than the table's width", "no entries"
POSITIONS_16, COLUMNS_32, SLICE_WIDTH = "LDS positions beyond 16 bits", "column arithmetic beyond 32 bits", "slices wider than the table"
LDS_CAP_TEXT = "windows, dictionaries and table exceed the LDS cap"
# vw_fast.h's clauses
FAST_TAKEN, FAST_ROWS, FAST_WIDTHS, FAST_DICTS, FAST_TRIPS, FAST_TABLE, FAST_OFF = range(7)


def layout(win, R):
    """windows one after the other -> ([base], [size], S)"""
    size = [R + hi - lo for lo, hi in win]
    base = [sum(size[:c]) for c in range(len(win))]
    return base, size, sum(size)


def position(win, base, o):
    """the LDS position of offset o for a workgroup's first row: inside the one window that holds it"""
    (c,) = [c for c, (lo, hi) in enumerate(win) if lo <= o <= hi]
    return base[c] + o - win[c][0]


def fast_rule(R, uw, vd_u, ntrip, n8):
    return (FAST_ROWS if R not in (256, 512) else FAST_WIDTHS if uw == 0 else FAST_DICTS if vd_u == 0 else FAST_TRIPS if not 1 <= ntrip <= 4
            else FAST_TABLE if n8 > R else FAST_TAKEN)


def vidxw_plan(patterns, W, M, N, R, uw, dict_lengths, fast_off=False):
    """build_xwin's plan for the patterns (offset tuples, in table order) of a table W wide; uw: the slices' common width or 0;
    dict_lengths: values per dictionary, one per 256 rows -> dict(verdict=...) and, where the verdict is OK,
      nwin S lp wp words lds lmin lmax vd_u; win: the window list as uploaded; table: the 16-bit words; ntrip, trips (six of them);
      fast_clause fast_kind fast_lds"""
    if any(len(p) > W for p in patterns):
        return dict(verdict=PATTERN_LENGTH)
    offsets = sorted({o for p in patterns for o in p})
    if not offsets:
        return dict(verdict=NO_ENTRIES)
    win = windows(offsets, R)
    if len(win) > SPX_MAXWIN:
        return dict(verdict=TOO_MANY_WINDOWS)
    base, size, S = layout(win, R)
    if S > 65536:
        return dict(verdict=POSITIONS_16)
    if M + R + S + max(abs(offsets[0]), abs(offsets[-1])) > INT32_MAX - 8:
        return dict(verdict=COLUMNS_32)
    npat, wp, lp = len(patterns), (W + 7) & ~7, (len(patterns) + 7) & ~7
    if uw > wp:
        return dict(verdict=SLICE_WIDTH)
    words = lp + npat * wp
    lds = ((S + 2) & ~1) * 8 + (R // 256) * VI_MAX * 8 + 2 * words
    if lds > VW_MAX_LDS:
        return dict(verdict=LDS_CAP_TEXT)
    table = np.zeros(words, np.int64)
    for i, p in enumerate(patterns):
        table[i] = len(p)
        at = [8 * position(win, base, o) for o in p] or [0]
        table[lp + i * wp:lp + (i + 1) * wp] = at + [at[-1]] * (wp - len(at))
    wlist = [len(win), S] + [v for c in range(len(win)) for v in (base[c], win[c][0] - base[c])] + [INT32_MAX] * (2 * max(0, 4 - len(win)))
    vd_u = dict_lengths[0] if len(set(dict_lengths)) == 1 else 0
    per_window = 1 <= len(win) <= 4 and S <= 4 * R and N < DESC_COLS and win[0][0] >= -DESC_COLS and M + win[-1][1] + 2 * R <= DESC_COLS
    trips = [(base[c] + i0, win[c][0] + i0, min(R, size[c] - i0)) for c in range(len(win)) for i0 in range(0, size[c], R)] if per_window else []
    if len(trips) > 6:
        trips = []
    ntrip = len(trips)
    clause = fast_rule(R, uw, vd_u, ntrip, words // 8)
    if clause == FAST_TAKEN and fast_off:
        clause = FAST_OFF
    kind = 0 if clause != FAST_TAKEN else 2 if vd_u <= 2 else 1
    return dict(verdict=OK, windows=win, nwin=len(win), S=S, lp=lp, wp=wp, words=words, lds=lds, lmin=min(map(len, patterns)), lmax=max(map(len, patterns)),
                vd_u=vd_u, win=wlist, table=table, ntrip=ntrip, trips=trips + [(0, 0, 0)] * (6 - ntrip), fast_clause=clause, fast_kind=kind,
                fast_lds=0 if kind == 0 else 8 * ((S + 2) & ~1) + (0 if kind == 2 else R // 256 * VI_MAX * 8) + 2 * words)


# build_sellpx's refusals, in the order it checks them (it reports none: the codes of xwin_plan.h's SpxRefusal)
SPX_OK, SPX_NO_ENTRIES, SPX_WINDOW_COUNT, SPX_POSITIONS_16, SPX_WINDOWS_LDS, SPX_TABLE = range(6)


def sellpx_plan(patterns, ids, M):
    """build_sellpx's plan: patterns as offset tuples, ids: the rows' pattern ids -> dict(verdict=code) and, where accepted, nwin S
    max_words, win (count, then omin / base / size each), wgptr, pat (workgroup-local ids), tab (without its 8 words of padding)"""
    offsets = sorted({o for p in patterns for o in p})
    if not offsets:
        return dict(verdict=SPX_NO_ENTRIES)
    win = windows(offsets, SPX_ROWS)
    if len(win) > SPX_MAXWIN:
        return dict(verdict=SPX_WINDOW_COUNT)
    base, size, S = layout(win, SPX_ROWS)
    if S > 65535:
        return dict(verdict=SPX_POSITIONS_16)
    if 8 * S >= SPX_LDS_BYTES:
        return dict(verdict=SPX_WINDOWS_LDS)
    room = (SPX_LDS_BYTES - 8 * S) // 2
    tab, wgptr, pat, max_words = [], [0], [], 0
    for r0 in range(0, M, SPX_ROWS):
        used = []
        for i in ids[r0:r0 + SPX_ROWS]:
            if i not in used:
                used.append(i)
            pat.append(used.index(i))
        used = used or [0]
        body = [[len(patterns[i])] + ([position(win, base, o) for o in patterns[i]] or [0]) for i in used]
        words = (len(used) + sum(map(len, body)) + 3) // 4 * 4
        max_words = max(max_words, words)
        if words > room or words > 65535 or len(tab) + words > INT32_MAX - 8:
            return dict(verdict=SPX_TABLE)
        starts = [len(used) + sum(map(len, body[:k])) for k in range(len(used))]
        flat = starts + [v for b in body for v in b]
        tab += flat + [0] * (words - len(flat))
        wgptr.append(len(tab))
    return dict(verdict=SPX_OK, windows=win, nwin=len(win), S=S, max_words=max_words, win=[len(win)] + [v for c in range(len(win)) for v in (win[c][0], base[c], size[c])],
                wgptr=wgptr, pat=pat, tab=tab)


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
