"""Operators that sit exactly on, and one step past, the eligibility limits of the SpMV forms (include/saena_gpu.h, variants 0..17),
the limits restated in numpy, and a plain reference of the product.  No GPU here: tests/test_form_limits.py holds the generators to
the restated limits, tests/test_gpu_form_limits.py holds the library to both.

A form's builder says "this operator fits my 16-bit codes, my LDS table, my windows"; the plan-time autotune then picks among the
forms by timing alone.  Every case below is a pair (at, past): `at` is the last operator the limit admits, `past` differs from it by one
entry, row, pattern, segment, window or template.  The restated limits are written from the builders' comments and the refusal
messages of sgpu_op_set_variant ("The limits of the forms"), not from the builders' code.

Operators are CSR arrays with ascending, distinct columns per row, deterministic, no files."""
from collections import namedtuple

import numpy as np

# ---- the numbers the forms document --------------------------------------------------------------------------------------------
TILE = (2048, 4096)            # products a row block stages in LDS: 16 KiB / 32 KiB plan
BLOCK_ROWS = (256, 512)        # rows per row block of the two plans
CC_SEGMENTS = 256              # 16-bit column codes: at most 256 segments of 256 columns per row block (8+8 bits, the finest split)
ONE_TABLE = 4096               # ints of ONE pattern table of fixed width (k_sellp, k_sellp2, k_vidx)
GROUP_TABLE, GROUP_ROWS = 8192, 1024     # ints of the table of a group of 1024 rows (k_sellp<wide>)
PATTERNS = 65535               # 16-bit pattern ids
SPX_WINDOWS, SPX_ROWS, SPX_LDS = 16, 512, 80 * 1024      # k_sellpx: windows of x, rows per workgroup, LDS for windows + table
XL_MAX, XL_MAXT, NCU = 20224, 8, 256     # x-in-LDS: doubles of x per window, windows per chunk, chunks (one per CU of an MI355X)
RT_BYTES = 32768               # k_rowt: bytes of LDS for the templates
DENSE_ROWS = 8192
SELL_PAD, SORTED_PAD, SELLX_PAD = 112, 105, 125          # stored / actual entries, in per cent

Op = namedtuple("Op", "rp col val M N square")
# one forced form on a pair: names[verdict] is the kernel name expected for an operator of that verdict, None = refused;
# printed: the numbers the refusal message must carry; tile: as in tests/test_gpu_forms.py (rows of at most `tile` entries are sequential)
Run = namedtuple("Run", "variant lanes cls env tile names printed", defaults=((),))
# plan: verdict -> what the x-in-LDS plan must say (sgpu_debug_block_plan, big = 2): (windows, columns per window, sums in LDS)
Case = namedtuple("Case", "key at past predicate verdicts runs plan", defaults=(None,))
SEQ, TREE = "sequential", "tree"
KEEP = {"SAENA_KEEP_HOST_VALUES": "1"}


def _values(rows, cols):
    """seven distinct values: every form that codes values (k_vidx: 256 per 256 rows) takes them"""
    return 0.5 + ((3 * rows + 5 * cols) % 7) * 0.25


def make_op(lens, cols, N, square=False, val=None):
    lens = np.asarray(lens, np.int64)
    M = lens.size
    rp = np.concatenate([[0], np.cumsum(lens)])
    cols = np.asarray(cols, np.int64)
    assert cols.size == rp[-1] and cols.min() >= 0 and cols.max() < N
    rows = np.repeat(np.arange(M), lens)
    step = np.diff(cols)
    same_row = rows[1:] == rows[:-1]
    assert np.all(step[same_row] > 0), "columns ascend within a row"
    val = _values(rows, cols) if val is None else np.asarray(val, np.float64)
    return Op(rp.astype(np.int32), cols.astype(np.int32), val, M, int(N), square)


def rows_of(op):
    return np.repeat(np.arange(op.M), np.diff(op.rp))


def from_offsets(offsets_per_row, N):
    """row r holds the columns r + offsets_per_row[r]"""
    lens = [len(o) for o in offsets_per_row]
    cols = np.concatenate([r + np.asarray(o, np.int64) for r, o in enumerate(offsets_per_row)])
    return make_op(lens, cols, N)


def seq_matvec(rp, col, val, x):
    """the reference's local loop: sum += val[rp + j] * x[col[rp + j]] for j < len, fp64, in stored order (vectorised over the rows)"""
    rp = np.asarray(rp, np.int64)
    lens = np.diff(rp)
    y = np.zeros(lens.size)
    x = np.asarray(x, np.float64)
    for j in range(int(lens.max()) if lens.size else 0):
        m = lens > j
        k = rp[:-1][m] + j
        y[m] = y[m] + val[k] * x[col[k]]
    return y


# ---- restated cuts and limits --------------------------------------------------------------------------------------------------
def plan_blocks(rp, cap, maxrows):
    """the row-block plan: consecutive rows while the block holds <= cap products and <= maxrows rows; a longer row alone"""
    M = len(rp) - 1
    blk, r = [0], 0
    while r < M:
        start = r
        while r < M and r - start < maxrows and rp[r + 1] - rp[start] <= cap:
            r += 1
        if r == start:
            r += 1
        blk.append(r)
    return blk


def tile_verdict(op, k):
    """the column-major form of plan k: every row block's entries fit the tile (and no block is empty)"""
    blk = plan_blocks(op.rp, TILE[k], BLOCK_ROWS[k])
    n = np.diff(np.asarray(op.rp, np.int64)[blk])
    return "served" if n.max() <= TILE[k] and n.min() > 0 else "refused"


def cc16_verdict(op, k=0):
    """the split of the 16-bit codes: the largest offset width of 12..8 bits at which every row block touches at most 2^(16 - bits)
    segments"""
    blk = plan_blocks(op.rp, TILE[k], BLOCK_ROWS[k])
    for ob in range(12, 7, -1):
        if all(np.unique(op.col[op.rp[a]:op.rp[b]] >> ob).size <= 1 << (16 - ob) for a, b in zip(blk[:-1], blk[1:])):
            return f"served:{16 - ob}+{ob}"
    return "refused"


def patterns(op, rowbase=False):
    """-> (ids per row, list of patterns) in order of first appearance; a pattern is the row's columns relative to the row index
    (rowbase: to the row's first column)"""
    lens = np.diff(op.rp)
    if op.M > 4096 and lens.min() == lens.max():                # (rows of one length, many of them: the same sets, ids in sorted order)
        c = op.col.astype(np.int64).reshape(op.M, -1)
        rel = c - (c[:, :1] if rowbase else np.arange(op.M)[:, None])
        rel -= rel.min()
        base = int(rel.max()) + 1
        assert base ** rel.shape[1] < 2 ** 62
        uniq, ids = np.unique(rel @ base ** np.arange(rel.shape[1]), return_inverse=True)      # (a row's offsets as one number)
        return ids.ravel(), [int(lens[0])] * len(uniq)
    seen, ids, pats = {}, np.zeros(op.M, np.int64), []
    for r in range(op.M):
        c = op.col[op.rp[r]:op.rp[r + 1]].astype(np.int64)
        key = (c - (c[0] if rowbase and c.size else 0 if rowbase else r)).tobytes()
        if key not in seen:
            seen[key] = len(pats)
            pats.append(c.size)
        ids[r] = seen[key]
    return ids, pats


def sell_padding_ok(op, limit=SELL_PAD):
    lens = np.diff(op.rp).astype(np.int64)
    pad = np.concatenate([lens, np.zeros(-op.M % 64, np.int64)]).reshape(-1, 64)
    return 100 * int(pad.max(axis=1).sum()) * 64 <= limit * int(lens.sum())


def sellp_verdict(op):
    """row patterns: ONE table of npat x (W + 1) ints while that is at most 4096; else a table per group of 1024 rows of at most 8192 ints
    (a start per pattern, length + offsets per pattern, one spare int); at most 65 535 patterns; in either mode of what the
    offsets are relative to"""
    if not sell_padding_ok(op):
        return "refused"
    W = int(np.diff(op.rp).max())
    if W + 3 > GROUP_TABLE:
        return "refused"
    for rowbase in (False, True):
        ids, pats = patterns(op, rowbase)
        if len(pats) > PATTERNS:
            continue
        if len(pats) * (W + 1) <= ONE_TABLE:
            return "served:one"
        ok = True
        for g in range(0, op.M, GROUP_ROWS):
            used = np.unique(ids[g:g + GROUP_ROWS])
            ok = ok and used.size + 1 + sum(1 + pats[i] for i in used) <= GROUP_TABLE
        if ok:
            return "served:wide"
    return "refused"


def sellpx_verdict(op):
    """x in LDS for the row patterns: the offsets of all patterns cluster into windows (a gap of more than 512 columns separates two),
    at most 16 of them; a workgroup of 512 rows holds 512 + (omax - omin) doubles per window and its table (a start per pattern, length +
    positions per pattern, 16-bit words in fours) in 80 KiB"""
    ids, pats = patterns(op)
    rows = rows_of(op)
    offs = np.unique(op.col.astype(np.int64) - rows)
    cut = np.flatnonzero(np.diff(offs) > SPX_ROWS)
    nwin = cut.size + 1
    if nwin > SPX_WINDOWS:
        return "refused"
    lo, hi = offs[np.concatenate([[0], cut + 1])], offs[np.concatenate([cut, [offs.size - 1]])]
    S = int((SPX_ROWS + hi - lo).sum())
    for g in range(0, op.M, SPX_ROWS):
        used = np.unique(ids[g:g + SPX_ROWS])
        words = -(-(used.size + sum(1 + max(pats[i], 1) for i in used)) // 4) * 4
        if S * 8 + words * 2 > SPX_LDS:
            return "refused"
    return "served"


def xlds_chunks(op):
    """one nnz-balanced row chunk per CU: chunk b starts at the first row whose prefix reaches b / nb of the entries"""
    nb = min(NCU, op.M)
    nnz = int(op.rp[-1])
    cut = [0] + [min(op.M, int(np.searchsorted(op.rp, nnz * b // nb))) for b in range(1, nb)] + [op.M]
    return np.maximum.accumulate(cut)


def xlds_verdict(op, global_acc=False):
    """x in LDS: every chunk's columns reach over at most 8 windows of 20 224; where the chunks are short, over 8 windows shortened by
    the chunk's rows (in 64s), the partial sums then live in LDS behind the window"""
    blk = xlds_chunks(op)
    span, rows = 0, 0
    for a, b in zip(blk[:-1], blk[1:]):
        if b > a and op.rp[b] > op.rp[a]:
            c = op.col[op.rp[a]:op.rp[b]]
            span = max(span, int(c.max()) - int(c.min()))
        rows = max(rows, int(b - a))
    if span // XL_MAX + 1 > XL_MAXT:
        return "refused"
    if span >= XL_MAX and rows <= XL_MAX // 4 and not global_acc and span // (XL_MAX - -(-rows // 64) * 64) + 1 <= XL_MAXT:
        return "served:lds"
    return "served:global" if span >= XL_MAX else "served:one window"


def sellx_stored(op, win):
    """sliced ELLPACK inside the (chunk, window) blocks: a row's piece per window of its chunk (every row has one, maybe empty, in the
    chunk's last window), the pieces of a block sorted by length, 64 to a slice, a slice as wide as its longest piece made even"""
    blk = xlds_chunks(op)
    stored = 0
    for a, b in zip(blk[:-1], blk[1:]):
        if b == a:
            continue
        c = op.col[op.rp[a]:op.rp[b]].astype(np.int64)
        T = (int(c.max()) - int(c.min())) // win + 1 if c.size else 1
        w = np.minimum((c - (c.min() if c.size else 0)) // win, T - 1)
        k = np.repeat(np.arange(b - a), np.diff(op.rp[a:b + 1]))
        counts = np.bincount(k * T + w, minlength=(b - a) * T).reshape(b - a, T)
        for t in range(T):
            pieces = np.sort(counts[:, t] if t == T - 1 else counts[counts[:, t] > 0, t])[::-1]
            stored += int(((pieces[::64] + 1) // 2 * 2).sum()) * 64
    return stored


def sellx_verdict(op, global_acc=False):
    """on top of the x-in-LDS plan: at most 25 % more stored than entries"""
    v = xlds_verdict(op, global_acc)
    if v == "refused":
        return v
    rows = int(np.diff(xlds_chunks(op)).max())
    win = XL_MAX - -(-rows // 64) * 64 if v == "served:lds" else XL_MAX
    return v if 100 * sellx_stored(op, win) <= SELLX_PAD * int(op.rp[-1]) else "refused"


def templates(op):
    seen = set()
    for r in range(op.M):
        a, b = op.rp[r], op.rp[r + 1]
        seen.add((op.col[a:b].astype(np.int64) - r).tobytes() + op.val[a:b].tobytes())
    return len(seen)


def rowt_verdict(op):
    """row templates: (length, relative columns, values) of every distinct row, (W + 1) ints and W doubles each, in 32 768 bytes"""
    W = int(np.diff(op.rp).max())
    return "served" if templates(op) * ((W + 1) * 4 + W * 8) <= RT_BYTES else "refused"


def sell_verdict(op, sorted_rows=False):
    """sliced ELLPACK: slices of 64 rows pad to at most 12 % more than the entries; opt-in, the rows sorted by length (longest first,
    rows of one length in their order) in windows of 2048 rows pad to at most 5 %"""
    if sell_padding_ok(op):
        return "served:plain"
    lens = np.diff(op.rp).astype(np.int64)
    if not sorted_rows or lens.sum() < 4 * op.M:
        return "refused"
    tot = 0
    for w in range(0, op.M, 2048):
        s = np.sort(lens[w:w + 2048])[::-1]
        tot += int(s[::64].sum()) * 64
    return "served:sorted" if 100 * tot <= SORTED_PAD * int(lens.sum()) else "refused"


def pair_verdict(op):
    """two positions per 16-byte load from 16 entries per row on"""
    return "served:pair" if int(op.rp[-1]) >= 16 * op.M else "served:single"


def dense_verdict(op):
    return "served" if op.M <= DENSE_ROWS and op.M * op.N <= DENSE_ROWS * DENSE_ROWS else "refused"


# ---- the generators ------------------------------------------------------------------------------------------------------------
def _long_rows(longs, M=600, N=8192, seed=3):
    """short rows of 3..9 entries, and one row of each length in `longs` spread over the operator"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(3, 10, size=M)
    at = np.linspace(40, M - 40, len(longs)).astype(int)
    lens[at] = longs
    cols = np.concatenate([np.sort(np.random.default_rng([seed, r]).choice(N, size=k, replace=False)) for r, k in enumerate(lens)])
    return make_op(lens, cols, N)


def case_tile():
    """#1: rows of 2047 .. 4097 entries among short rows: every tile form takes the operator, rows of at most the tile are
    sequential at one lane per row.  (the pair is the same operator twice: nothing is refused here, the edges are the rows)"""
    op = _long_rows([2047, 2048, 2049, 4095, 4096, 4097])
    names = {0: "k_csr_stream<16KiB>", 1: "k_csr_stream<32KiB>", 3: "k_csr_cc16<16KiB*", 4: "k_csr_cc16<32KiB*"}
    runs = [Run(v, 1, SEQ, {}, TILE[v in (1, 4)], {"served": n}) for v, n in names.items()]
    return Case("tile", op, op, lambda o: "served", ("served", "served"), runs)


def case_cm(k):
    """#1: the column-major form of plan k takes rows of exactly the tile and refuses a row of one entry more"""
    t = TILE[k]
    at, past = _long_rows([t - 1, t, t]), _long_rows([t - 1, t, t + 1])
    run = Run(7 + k, 1, SEQ, KEEP, t, {"served": f"k_csr_cm<{16 << k}KiB*", "refused": None})
    return Case(f"cm{16 << k}", at, past, lambda o: tile_verdict(o, k), ("served", "refused"), [run])


def case_cc16():
    """#2: 512 rows of 8 entries, N = 2^17: row r and row r + 256 sit in the 256-column segment 2 r, so each row block of either plan
    touches exactly 256 segments of 256 columns (and 256 of 512: only the 8+8 split fits); past: the last entry of row 255 moves to
    segment 511, the 257th"""
    M, N = 512, 1 << 17
    r = np.arange(M) % 256
    cols = (512 * r)[:, None] + 31 * np.arange(8)[None, :]
    past = cols.copy()
    past[255, 7] = 511 * 256
    ops = [make_op(np.full(M, 8), c.ravel(), N) for c in (cols, past)]
    runs = [Run(3 + k, 1, SEQ, env, TILE[k], {"served:8+8": f"k_csr_cc16<{16 << k}KiB,8+8>", "refused": None}, (256, 256))
            for k in (0, 1) for env in ({}, {"SAENA_HOST_CC16": "1"})]
    return Case("cc16", ops[0], ops[1], cc16_verdict, ("served:8+8", "refused"), runs)


def _pattern_offsets(p, n=7):
    """pattern p of n entries: offset 0, then 4 j + (digit j of p in base 4): distinct for p < 4^(n-1), the same pattern whether taken
    relative to the row index or to the row's first column"""
    return [0] + [4 * j + (p >> (2 * (j - 1))) % 4 for j in range(1, n)]


def _pattern_op(M, pats, N=None):
    """row r follows pats[r % len(pats)]"""
    span = max(max(p) for p in pats)
    return from_offsets([pats[r % len(pats)] for r in range(M)], N or M + span + 1)


def case_one_table():
    """#3: 512 patterns of 7 entries are 4096 ints at width 8: ONE table; 513 go to the tables per 1024 rows.  k_vidx needs the one
    table"""
    ops = [_pattern_op(2048, [_pattern_offsets(p) for p in range(n)]) for n in (512, 513)]
    runs = [Run(11, 1, SEQ, {}, 0, {"served:one": "k_sellp", "served:wide": "k_sellp<wide>"}),
            Run(14, 1, SEQ, {}, 0, {"served:one": "k_sellp2", "served:wide": "k_sellp2<wide>"}),
            Run(17, 1, SEQ, {}, 0, {"served:one": "k_vidx", "served:wide": None}, (256, 256))]
    return Case("one_table", ops[0], ops[1], sellp_verdict, ("served:one", "served:wide"), runs)


def case_group_table():
    """#4: one group of 1024 rows following 903 patterns of 7 entries and 8 of 6: 911 starts + 903 x 8 + 8 x 7 + 1 spare = 8192 ints;
    904 and 7 make 8193.  The patterns start at offset 0, so they are as many relative to the rows' first columns"""
    def op(n7, n6):
        return _pattern_op(1024, [_pattern_offsets(p) for p in range(n7)] + [_pattern_offsets(2048 + p, 6) for p in range(n6)])
    run = Run(11, 1, SEQ, {}, 0, {"served:wide": "k_sellp<wide>", "refused": None}, (GROUP_TABLE, GROUP_ROWS))
    return Case("group_table", op(903, 8), op(904, 7), sellp_verdict, ("served:wide", "refused"), [run])


def case_longest_row():
    """#4: 64 rows of one pattern of W entries: start + length + W offsets + spare = W + 3 ints: W = 8189 fills the group's table"""
    ops = [_pattern_op(64, [list(range(W))]) for W in (8189, 8190)]
    run = Run(11, 1, SEQ, {}, 0, {"served:wide": "k_sellp<wide>", "refused": None}, (GROUP_TABLE, GROUP_ROWS))
    return Case("longest_row", ops[0], ops[1], sellp_verdict, ("served:wide", "refused"), [run])


def case_pattern_ids():
    """#5: 530 000 rows of two entries, row r holding columns r and r + 1 + (r mod n): n = 65 535 patterns get 16-bit ids, 65 536 do not,
    relative to the row index or to the first column alike.  Large enough that an eighth of the entries admits the patterns' table
    (3 x 65 536 ints) and that the patterns are found on several threads and merged: 1 and 16 threads give the same ids"""
    M = 530000
    r = np.arange(M)
    ops = [make_op(np.full(M, 2), np.stack([r, r + 1 + r % n], 1).ravel(), M + 65537) for n in (PATTERNS, PATTERNS + 1)]
    runs = [Run(11, 1, SEQ, {"SAENA_SETUP_THREADS": t}, 0, {"served:wide": "k_sellp<wide>", "refused": None}, (GROUP_TABLE, GROUP_ROWS))
            for t in ("1", "16")]
    return Case("pattern_ids", ops[0], ops[1], sellp_verdict, ("served:wide", "refused"), runs)


def case_sellpx_windows():
    """#6: one pattern of 16 / 17 entries 1000 columns apart: 16 / 17 windows of 512 doubles"""
    ops = [_pattern_op(1024, [[1000 * k for k in range(n)]], 1024 + 16001) for n in (16, 17)]
    run = Run(15, 1, SEQ, {}, 0, {"served": "k_sellpx", "refused": None}, (SPX_WINDOWS, SPX_LDS // 1024))
    return Case("sellpx_windows", ops[0], ops[1], sellpx_verdict, ("served", "refused"), [run])


def case_sellpx_s():
    """#6: 20 workgroups of 512 rows of ONE entry, workgroup g at offset 512 g, the last at `span`: one window of 512 + span doubles and
    the smallest table there is (1 start + 1 length + 1 position -> 4 words = 8 bytes): S = 10 239 leaves exactly those 8 bytes,
    S = 10 240 is the 80 KiB"""
    M = 20 * 512
    g = np.arange(M) // 512
    ops = [make_op(np.ones(M, int), np.arange(M) + np.where(g < 19, 512 * g, span), M + 9729) for span in (9727, 9728)]
    run = Run(15, 1, SEQ, {}, 0, {"served": "k_sellpx", "refused": None}, (SPX_WINDOWS, SPX_LDS // 1024))
    return Case("sellpx_s", ops[0], ops[1], sellpx_verdict, ("served", "refused"), [run])


def case_sellpx_lds():
    """#6: one window: 20 entries 512 columns apart but the last, which sits `span` columns from the first.  The workgroup's table is
    1 start + 1 length + 20 positions = 22 -> 24 words = 48 bytes, so the window may hold (81920 - 48) / 8 = 10234 doubles = 512 + 9722:
    windows + table end exactly at the 80 KiB"""
    ops = [_pattern_op(1024, [[512 * k for k in range(19)] + [span]]) for span in (9722, 9723)]
    run = Run(15, 1, SEQ, {}, 0, {"served": "k_sellpx", "refused": None}, (SPX_WINDOWS, SPX_LDS // 1024))
    return Case("sellpx_lds", ops[0], ops[1], sellpx_verdict, ("served", "refused"), [run])


def _xlds_op(last, win):
    """16 384 rows of 16 entries: 256 chunks of 64 rows (k_sellx slices a chunk's pieces 64 at a time).  Row 0 holds the first column, both sides of every window edge w x win and
    `last`; row 1 holds the last column of window 8 (8 win - 1); the others stay around the diagonal"""
    M = 16384
    row0 = [0] + [w * win - d for w in range(1, 8) for d in (1, 0)] + [last]
    row1 = list(range(1, 16)) + [8 * win - 1]
    cols = [row0, row1] + [list(range(r, r + 16)) for r in range(2, M)]
    return make_op(np.full(M, 16), np.concatenate(cols), 8 * XL_MAX + 1)


def case_xlds(acc):
    """#7: chunk 0 reaches the last column of window 8 / the first of window 9.  "lds": windows of 20 224 - 64 with the partial sums
    behind them; one column more and the form keeps them in global memory under full windows.  "global": full windows; one column
    more than 8 x 20 224 is refused"""
    win = XL_MAX - 64 if acc == "lds" else XL_MAX
    at, past = _xlds_op(8 * win - 2, win), _xlds_op(8 * win, win)
    env = {} if acc == "lds" else {"SAENA_XLDS_GLOBAL_ACC": "1"}
    names = {"served:lds": "k_csr_xlds", "served:global": "k_csr_xlds", "refused": None}
    runs = [Run(10, 8, TREE, env, 0, names, (XL_MAXT * XL_MAX,)),
            Run(16, 8, TREE, env, 0, {k: v and "k_csr_xldsr" for k, v in names.items()}, (XL_MAXT * XL_MAX,)),
            Run(12, 1, TREE, dict(KEEP, **env), 0, {k: v and "k_sellx" for k, v in names.items()}, (XL_MAXT, 25))]
    verdicts = ("served:lds", "served:global") if acc == "lds" else ("served:global", "refused")
    plan = {"served:lds": (XL_MAXT, XL_MAX - 64, 1), "served:global": (XL_MAXT, XL_MAX, 0)}
    return Case(f"xlds_{acc}", at, past, lambda o: sellx_verdict(o, acc == "global"), verdicts, runs, plan)


def case_sellx():
    """#9: 256 chunks of 64 rows, 32 of 20 entries and 32 of 12 around the diagonal: one slice of width 20 per chunk stores 327 680;
    262 144 entries pad exactly 25 %, one entry fewer (off the last row) pads more"""
    lens = np.tile(np.repeat([20, 12], 32), 256)
    ops = []
    for cut in (0, 1):
        k = lens.copy()
        k[-1] -= cut
        ops.append(from_offsets([list(range(n)) for n in k], lens.size + 20))
    run = Run(12, 1, TREE, KEEP, 0, {"served:one window": "k_sellx", "refused": None}, (XL_MAXT, 25))
    return Case("sellx", ops[0], ops[1], sellx_verdict, ("served:one window", "refused"), [run], {"served:one window": (1, XL_MAX, 0)})


def case_rowt():
    """#8: templates of 6 entries are 7 ints + 6 doubles = 76 bytes: 431 fill 32 756 of the 32 768 bytes (431 x 7 ints: an odd count
    in front of the doubles), 432 do not fit.  The templates differ in their values alone"""
    def op(n, M=3017):
        o = _pattern_op(M, [list(range(6))])
        t = rows_of(o) % n
        return o._replace(val=1.0 + t / 1024.0 + (o.col - rows_of(o)) / 8.0)
    run = Run(13, 1, SEQ, KEEP, 0, {"served": "k_rowt", "refused": None}, (RT_BYTES,))
    return Case("rowt", op(431), op(432), rowt_verdict, ("served", "refused"), [run])


def _band(lens, width):
    """square: row r holds len consecutive columns from min(r, M - len) on, the diagonal among them"""
    M = len(lens)
    cols = np.concatenate([min(r, M - k) + np.arange(k) for r, k in enumerate(lens)])
    return make_op(lens, cols, M, square=True)


def _trimmed(lens, eligible, nnz):
    """take entries off the eligible rows in turn until `nnz` are left"""
    lens = np.array(lens, np.int64)
    cut = int(lens.sum()) - nnz
    lens[eligible] -= cut // eligible.size
    lens[eligible[:cut % eligible.size]] -= 1
    assert lens.sum() == nnz and lens.min() > 0
    return lens


def case_sell():
    """#9: four slices whose first row has 25 entries store 6400: 5715 entries pad 11.99 %, 5714 pad 12.01 %"""
    eligible = np.flatnonzero(np.arange(256) % 64)
    ops = [_band(_trimmed(np.full(256, 25), eligible, nnz), 25) for nnz in (5715, 5714)]
    run = Run(9, 1, SEQ, {}, 0, {"served:plain": "k_sell", "refused": None})
    return Case("sell", ops[0], ops[1], sell_verdict, ("served:plain", "refused"), [run])


def case_sell_sorted():
    """#9: every fourth row has 40 entries, the others 20 or fewer: plain slices store 10 240; sorted, one slice of 40 and three of 20
    store 6400: 6096 entries pad 4.99 %, 6095 pad 5.004 %"""
    lens = np.where(np.arange(256) % 4 == 0, 40, 20)
    eligible = np.flatnonzero(np.arange(256) % 4)[-63:]                # 129 of the 192 short rows keep 20: the sorted slices' first rows
    ops = [_band(_trimmed(lens, eligible, nnz), 40) for nnz in (6096, 6095)]
    run = Run(9, 1, SEQ, {"SAENA_SELL_SORTED": "1"}, 0, {"served:sorted": "k_sell<sorted>", "refused": None})
    return Case("sell_sorted", ops[0], ops[1], lambda o: sell_verdict(o, True), ("served:sorted", "refused"), [run])


def case_pair():
    """#10: 256 rows of 16 entries, and the same with one entry fewer: the pair and the single-position instantiations"""
    lens = np.full(256, 16)
    ops = [_band(lens, 16), _band(_trimmed(lens, np.array([100]), 16 * 256 - 1), 16)]
    names = {"served:pair": "k_sell", "served:single": "k_sell"}
    runs = [Run(9, 1, SEQ, {}, 0, names), Run(11, 1, SEQ, {}, 0, {k: "k_sellp" for k in names})]
    return Case("pair", ops[0], ops[1], pair_verdict, ("served:pair", "served:single"), runs)


def case_dense():
    """#11: 8192 x 64 is served, 8193 x 64 is refused"""
    def op(M):
        return make_op(np.full(M, 3), (np.arange(M)[:, None] * 5 % 40 + np.array([0, 7, 23])[None, :]).ravel(), 64)
    run = Run(5, 1, TREE, {}, 0, {"served": "k_dense_rows", "refused": None}, (DENSE_ROWS,))
    return Case("dense", op(8192), op(8193), dense_verdict, ("served", "refused"), [run])


GENERATORS = {
    "tile": case_tile, "cm16": lambda: case_cm(0), "cm32": lambda: case_cm(1), "cc16": case_cc16, "one_table": case_one_table,
    "group_table": case_group_table, "longest_row": case_longest_row, "pattern_ids": case_pattern_ids,
    "sellpx_windows": case_sellpx_windows, "sellpx_lds": case_sellpx_lds, "sellpx_s": case_sellpx_s, "sellx": case_sellx,
    "xlds_lds": lambda: case_xlds("lds"), "xlds_global": lambda: case_xlds("global"), "rowt": case_rowt, "sell": case_sell,
    "sell_sorted": case_sell_sorted, "pair": case_pair, "dense": case_dense,
}
_CASES = {}


def case(key):
    if key not in _CASES:
        _CASES[key] = GENERATORS[key]()
    return _CASES[key]


def coo(op):
    """the operator as the oracle's entries"""
    from oracle import oracle as orc
    return orc.coo_from_arrays(rows_of(op).astype(np.int32), op.col, op.val)


def oracle_op(op, entries=None):
    from oracle import oracle as orc
    entries = coo(op) if entries is None else entries
    if op.square:
        return orc.OracleOp(entries, op.M, op.M, orc.split_even(op.M, 1))
    return orc.OracleOp(entries, op.M, op.N, orc.split_even(op.M, 1), orc.split_even(op.N, 1), square=False)
