"""saena_amd/csrc/xwin_plan.h (the windows of x in LDS, the plans build_xwin and build_sellpx upload, the slice widths of build_vidx)
as a stand-alone host program: the header has no HIP in it, so g++ -std=c++17 compiles and runs it here.

Every field of both plans is held to tests/xwin_ref.py's numpy restatement on the named operators, at R = 256, 512 and 1024 and with
dictionaries of one common length and of differing lengths; the tables are held by round trip -- every entry maps back, through the
window list the kernel is given, to the offset the pattern had; and every refusal clause is reached on both sides of its edge.  The
pins of tests/test_xwin_ref.py must come out of the header unchanged.  tools/sanitize_xwin_plan.cpp runs the edge cases under
AddressSanitizer and UndefinedBehaviorSanitizer.

Two clauses of build_sellpx have no reachable refusing side: a workgroup's table of more than 65535 words (the room left in
SPX_LDS_BYTES is at most 40960 words, so `room` refuses first) and tables beyond INT32_MAX - 8 words in all (4 GiB of input)."""
import os
import subprocess

import numpy as np
import pytest

from tests import xwin_ref as X
from tests.test_xwin_ref import TABLE as PINS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1

PROGRAM = r"""
#include "xwin_plan.h"
#include <cstdio>
#include <cstring>
using namespace xwplan;

static_assert(sk::VI_MAX == vwfast::VI_MAX && sk::NXCD == vwfast::NXCD, "one definition");
static_assert(sizeof(sk::VwHead) == (16 + 3 * xwstage::MAX_TRIPS) * sizeof(int), "the head as the kernels' second parameter");

static bool ints(std::vector<int> &v) { for (int &x : v) if (std::scanf("%d", &x) != 1) return false; return true; }
template <class V> static void line(const char *name, const V &v) { std::printf("%s", name); for (auto x : v) std::printf(" %d", (int)x); std::printf("\n"); }

// per case of stdin, by its first word:
//   windows gap rows n, n offsets, q, q offsets -> "windows nwin S", nwin x "w omin omax base", q x "at window position"
//   vidxw npat W M ncols R uw fast_off nd, npat x (W + 1) ints, nd dictionary starts
//       -> "refusal code text" and, accepted, "head ...", "hwin ...", "trips ...", "scal wp lds fast_clause fast_kind fast_lds", "win ...", "tab ..."
//   spx npat M, npat x (length, offsets), M pattern ids
//       -> "refusal code" and, accepted, "spx nwin S max_words", "win ...", "wgptr ...", "pat ...", "tab ..."
//   slices M, M + 1 row pointers -> "slices ok uw tot", "ptr ..."
int main() {
    char word[16];
    while (std::scanf("%15s", word) == 1) {
        if (!std::strcmp(word, "windows")) {
            int gap, rows, n, q;
            if (std::scanf("%d %d %d", &gap, &rows, &n) != 3) return 1;
            std::vector<int> offs(n);
            if (!ints(offs) || std::scanf("%d", &q) != 1) return 1;
            std::vector<int> ask(q);
            if (!ints(ask)) return 1;
            const Windows w = cluster(offs, gap, rows);
            std::printf("windows %d %lld\n", w.nwin(), (long long)w.S);
            for (int c = 0; c < w.nwin(); ++c) std::printf("w %d %d %d\n", w.omin[c], w.omax[c], w.base[c]);
            for (int o : ask) std::printf("at %d %d\n", w.window(o), w.position(o));
        } else if (!std::strcmp(word, "vidxw")) {
            int npat, W, M, ncols, R, uw, off, nd;
            if (std::scanf("%d %d %d %d %d %d %d %d", &npat, &W, &M, &ncols, &R, &uw, &off, &nd) != 8) return 1;
            std::vector<int> tab((size_t)npat * (W + 1)), dptr(nd);
            if (!ints(tab) || !ints(dptr)) return 1;
            const VwPlan p = plan_vidxw(tab.data(), npat, W, M, ncols, R, uw, dptr.data(), off != 0);
            std::printf("refusal %d %s\n", p.refusal, refusal_text(p.refusal));
            if (p.refusal) continue;
            const sk::VwHead &h = p.s.head;
            std::printf("head %d %d %d %d %d %d %d %d\n", h.nwin, h.S, h.lp, h.tn, h.vd_u, h.lmin, h.lmax, h.ntrip);
            line("hwin", std::vector<int>(h.win, h.win + 8));
            std::printf("trips");
            for (const xwstage::Trip &t : h.trip) std::printf(" %d %d %d", t.lds, t.col, t.cnt);
            std::printf("\nscal %d %d %d %d %d\n", p.s.wp, p.s.lds, p.s.fast_clause, p.s.fast_kind, p.s.fast_lds);
            line("win", p.win);
            line("tab", p.tab);
        } else if (!std::strcmp(word, "spx")) {
            int npat, M;
            if (std::scanf("%d %d", &npat, &M) != 2) return 1;
            std::vector<int> pstart, ptab;
            for (int i = 0; i < npat; ++i) {
                std::vector<int> len(1);
                if (!ints(len)) return 1;
                std::vector<int> o(len[0]);
                if (!ints(o)) return 1;
                pstart.push_back((int)ptab.size());
                ptab.push_back(len[0]);
                ptab.insert(ptab.end(), o.begin(), o.end());
            }
            std::vector<int> ids(M);
            if (!ints(ids)) return 1;
            const SpxPlan p = plan_sellpx(pstart, ptab, std::vector<unsigned short>(ids.begin(), ids.end()), M);
            std::printf("refusal %d\n", p.refusal);
            if (p.refusal) continue;
            std::printf("spx %d %lld %lld\n", p.nwin, (long long)p.S, (long long)p.max_words);
            line("win", p.win);
            line("wgptr", p.wgptr);
            line("pat", p.pat);
            line("tab", p.tab);
        } else if (!std::strcmp(word, "slices")) {
            int M;
            if (std::scanf("%d", &M) != 1) return 1;
            std::vector<int> rp((size_t)M + 1);
            if (!ints(rp)) return 1;
            const SliceWidths s = slice_widths(rp.data(), M);
            std::printf("slices %d %d %lld\n", s.ok ? 1 : 0, s.uw, (long long)s.tot);
            line("ptr", s.ptr);
        } else return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("xwin_plan_check")
    src, out = str(d / "xwin_plan_check.cpp"), str(d / "xwin_plan_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "saena_amd", "csrc"), src, "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    return out


def run(exe, cases):
    r = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.splitlines()]


def ask_vidxw(patterns, W, M, N, R, uw, dict_lengths, fast_off=False):
    """the case's text: the table as build_sellp lays it out (length, offsets, zeros up to W) and the dictionaries' starts"""
    rows = []
    for p in patterns:
        rows += [len(p)] + list(p)[:W] + [0] * (W - len(p))
    dptr = np.concatenate([[0], np.cumsum(dict_lengths)])
    return f"vidxw {len(patterns)} {W} {M} {N} {R} {uw} {int(fast_off)} {len(dptr)} " + " ".join(map(str, rows)) + " " + " ".join(map(str, dptr))


def read_vidxw(out):
    """the program's lines of one case, consumed from the front of `out` -> dict"""
    w = out.pop(0)
    assert w[0] == "refusal"
    got = dict(refusal=int(w[1]), text=" ".join(w[2:]))
    if got["refusal"] == 0:
        for name in ("head", "hwin", "trips", "scal", "win", "tab"):
            w = out.pop(0)
            assert w[0] == name
            got[name] = [int(x) for x in w[1:]]
    return got


def hold_vidxw(got, want, patterns, R, key):
    """every field the issue lists against the restatement, then the table by round trip"""
    if want["verdict"] != X.OK:
        assert got["refusal"] != 0 and got["text"] == want["verdict"], key
        return
    assert got["refusal"] == 0 and got["text"] == "accepted", (key, got["text"])
    assert got["head"] == [want[k] for k in ("nwin", "S", "lp", "words", "vd_u", "lmin", "lmax", "ntrip")], key
    assert got["scal"] == [want[k] for k in ("wp", "lds", "fast_clause", "fast_kind", "fast_lds")], key
    assert got["win"] == want["win"] and got["hwin"] == want["win"][2:10], key
    assert len(got["win"]) == 2 + 2 * max(4, want["nwin"]) and all(v == INT32_MAX for v in got["win"][2 + 2 * want["nwin"]:]), key
    assert got["trips"] == [v for t in want["trips"] for v in t], key
    tab = np.array(got["tab"])
    assert len(tab) == want["words"] and (tab == want["table"]).all(), key
    # round trip, from the program's own window list: (base, omin - base) per window, a window ending where the next begins
    nwin, S, lp, wp = want["nwin"], want["S"], want["lp"], want["wp"]
    base = got["win"][2:2 + 2 * nwin:2] + [S]
    shift = got["win"][3:3 + 2 * nwin:2]
    assert list(tab[:len(patterns)]) == [len(p) for p in patterns] and not tab[len(patterns):lp].any(), key
    assert (tab[lp:] % 8 == 0).all() and tab[lp:].max() < 65536 and (tab[lp:] // 8 < S).all(), key
    for i, p in enumerate(patterns):
        at = tab[lp + i * wp:lp + (i + 1) * wp] // 8
        for j, o in enumerate(p):
            holds = [c for c in range(nwin) if base[c] <= at[j] < base[c + 1]]
            assert len(holds) == 1 and at[j] + shift[holds[0]] == o, (key, i, j)
        assert (at[len(p):] == (at[len(p) - 1] if p else 0)).all(), (key, i)


def dictionaries(M, same):
    n = ((M + 63) // 64 + 3) // 4
    return [3] * n if same or n == 1 else [3] * (n - 1) + [2]


# ---- the windows ----------------------------------------------------------------------------------------------------------------------
def test_one_clustering_one_lookup(exe):
    offs = [-1025, -513, -257, 0, 256, 512, 1024]
    out = run(exe, [f"windows {gap} {rows} {len(offs)} " + " ".join(map(str, offs)) + f" {len(offs)} " + " ".join(map(str, offs)) for gap, rows in ((256, 256), (512, 512), (512, 256))])
    for gap, rows in ((256, 256), (512, 512), (512, 256)):
        win = X.windows(offs, gap)
        base, _, S = X.layout(win, rows)
        assert out.pop(0) == ["windows", str(len(win)), str(S)]
        for c, (lo, hi) in enumerate(win):
            assert [int(x) for x in out.pop(0)[1:]] == [lo, hi, base[c]]
        for o in offs:
            c = [c for c, (lo, hi) in enumerate(win) if lo <= o <= hi][0]
            assert [int(x) for x in out.pop(0)[1:]] == [c, X.position(win, base, o)]
    assert not out


# ---- the k_vidxw plan on the named operators ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", [True, False], ids=["one dictionary length", "differing lengths"])
def test_the_vidxw_plan_of_every_named_operator(exe, same):
    cases, keys = [], []
    for name in sorted(X.OPERATORS):
        st = X.named_structure(name)
        _, _, M, N = X.operator(name)
        uw = st["w8"][0] if st["uniform"] else 0
        for R in X.ROWS:
            cases.append(ask_vidxw(st["patterns"], st["W"], M, N, R, uw, dictionaries(M, same)))
            keys.append((name, R, st, M, N, uw))
    out = run(exe, cases)
    clauses = set()
    for name, R, st, M, N, uw in keys:
        got = read_vidxw(out)
        want = X.vidxw_plan(st["patterns"], st["W"], M, N, R, uw, dictionaries(M, same))
        hold_vidxw(got, want, st["patterns"], R, (name, R, same))
        # ... and the pins of tests/test_xwin_ref.py, through geometry()
        g, pin = X.named_geometry(name, R), PINS[name][2][X.ROWS.index(R)]
        if isinstance(pin, str):
            assert got["refusal"] != 0 and pin in got["text"], (name, R)
        else:
            assert (got["head"][0], got["head"][1], -(-got["head"][1] // (4 * R))) == pin and got["scal"][1] == g["lds"] and got["head"][3] == g["words"], (name, R)
            assert X.setup_line(g) == (R, got["head"][0], got["head"][1], "%.1f" % (got["scal"][1] / 1024.0)), (name, R)
            clauses.add(got["scal"][2])
            assert (got["head"][7] == 0) == (want["nwin"] > 4 or want["S"] > 4 * R), (name, R)      # flat staging where the rule refuses
    assert not out
    # the dictionaries' clause stands before the trips'; tiny has one dictionary, whose length is common whatever it is
    assert clauses == ({X.FAST_TAKEN, X.FAST_ROWS, X.FAST_WIDTHS, X.FAST_TRIPS} if same else {X.FAST_TAKEN, X.FAST_ROWS, X.FAST_WIDTHS, X.FAST_DICTS})


def test_the_fast_kernel_switched_off(exe):
    st, M = X.named_structure("four"), 12000
    out = run(exe, [ask_vidxw(st["patterns"], st["W"], M, M, 256, 8, [2] * 47, off) for off in (False, True)])
    on, off = read_vidxw(out), read_vidxw(out)
    assert on["scal"][2:] == [X.FAST_TAKEN, 2, X.vidxw_plan(st["patterns"], st["W"], M, M, 256, 8, [2] * 47)["fast_lds"]]
    assert off["scal"][2:] == [X.FAST_OFF, 0, 0] and off["tab"] == on["tab"] and off["head"] == on["head"]


# ---- every refusal clause of the k_vidxw plan, on both sides of its edge -----------------------------------------------------------------
def one_window(S, R):
    """a pattern whose two offsets span one window of S doubles"""
    return [(0, S - R)] if S - R <= R else [tuple(range(0, S - R, R)) + (S - R,)]


VIDXW_EDGES = {
    # name: (patterns, W, M, N, R, uw, verdict)
    "a pattern as long as the table is wide": ([(0, 1, 2)], 3, 300, 300, 256, 8, X.OK),
    "a pattern longer than W": ([(0, 1, 2, 3)], 3, 300, 300, 256, 8, X.PATTERN_LENGTH),
    "one entry": ([(), (5,)], 1, 300, 300, 256, 8, X.OK),
    "no entries": ([(), ()], 1, 300, 300, 256, 8, X.NO_ENTRIES),
    "sixteen windows": ([tuple(1100 * k for k in range(16))], 16, 300, 20000, 256, 16, X.OK),
    "seventeen windows": ([tuple(1100 * k for k in range(17))], 17, 300, 20000, 256, 24, X.TOO_MANY_WINDOWS),
    "S of 65536: positions fit, the LDS does not": (one_window(65536, 256), 257, 300, 70000, 256, 8, X.LDS_CAP_TEXT),
    "S of 65537": (one_window(65537, 256), 257, 300, 70000, 256, 8, X.POSITIONS_16),
    "the LDS cap to the byte": (one_window(7925, 256), 31, 300, 9000, 256, 8, X.OK),                 # 7926 * 8 + 2048 + 2 * (8 + 32)
    "the smallest step beyond it: two more doubles of x": (one_window(7926, 256), 31, 300, 9000, 256, 8, X.LDS_CAP_TEXT),
    "... or eight more table words": (one_window(7925, 256), 33, 300, 9000, 256, 8, X.LDS_CAP_TEXT),
    "slices as wide as the table": ([(0, 1)], 8, 300, 300, 256, 8, X.OK),
    "slices wider than the table": ([(0, 1)], 8, 300, 300, 256, 16, X.SLICE_WIDTH),
    "an offset at the 32-bit edge": ([(0,), (INT32_MAX - 8 - 1000 - 256 - 512,)], 1, 1000, 1000, 256, 8, X.OK),
    "... and one beyond": ([(0,), (INT32_MAX - 8 - 1000 - 256 - 512 + 1,)], 1, 1000, 1000, 256, 8, X.COLUMNS_32),
    "... on the negative side": ([(-(INT32_MAX - 8 - 1000 - 256 - 512 + 1),), (0,)], 1, 1000, 1000, 256, 8, X.COLUMNS_32),
}


def test_every_refusal_of_the_vidxw_plan_at_its_edge(exe):
    names = sorted(VIDXW_EDGES)
    out = run(exe, [ask_vidxw(p, W, M, N, R, uw, dictionaries(M, True)) for p, W, M, N, R, uw, _ in (VIDXW_EDGES[n] for n in names)])
    seen = set()
    for n in names:
        p, W, M, N, R, uw, verdict = VIDXW_EDGES[n]
        want = X.vidxw_plan(p, W, M, N, R, uw, dictionaries(M, True))
        assert want["verdict"] == verdict, n                                     # the restatement agrees with the table
        hold_vidxw(read_vidxw(out), want, p, R, n)
        seen.add(verdict)
    assert not out
    assert seen == {X.OK, X.PATTERN_LENGTH, X.NO_ENTRIES, X.TOO_MANY_WINDOWS, X.POSITIONS_16, X.COLUMNS_32, X.SLICE_WIDTH, X.LDS_CAP_TEXT}
    assert X.vidxw_plan(*VIDXW_EDGES["the LDS cap to the byte"][:6], [3, 3])["lds"] == X.VW_MAX_LDS


# ---- the k_sellpx plan ------------------------------------------------------------------------------------------------------------------
def ask_spx(patterns, ids, M):
    return f"spx {len(patterns)} {M} " + " ".join(" ".join(map(str, (len(p),) + tuple(p))) for p in patterns) + " " + " ".join(map(str, ids))


def read_spx(out):
    w = out.pop(0)
    assert w[0] == "refusal"
    got = dict(refusal=int(w[1]))
    if got["refusal"] == 0:
        for name in ("spx", "win", "wgptr", "pat", "tab"):
            w = out.pop(0)
            assert w[0] == name
            got[name] = [int(x) for x in w[1:]]
    return got


def hold_spx(got, want, patterns, ids, M, key):
    assert got["refusal"] == want["verdict"], key
    if want["verdict"] != X.SPX_OK:
        return
    assert got["spx"] == [want["nwin"], want["S"], want["max_words"]] and got["win"] == want["win"], key
    assert got["wgptr"] == want["wgptr"] and got["pat"] == want["pat"] and got["tab"] == want["tab"] + [0] * 8, key
    nwin, tab, wgptr = got["win"][0], got["tab"], got["wgptr"]
    omin, base, size = got["win"][1::3], got["win"][2::3], got["win"][3::3]
    assert wgptr[0] == 0 and all(b >= a and (b - a) % 4 == 0 for a, b in zip(wgptr, wgptr[1:])) and len(tab) == wgptr[-1] + 8, key
    for g in range(len(wgptr) - 1):
        t = tab[wgptr[g]:wgptr[g + 1]]
        rows = range(g * X.SPX_ROWS, min(M, (g + 1) * X.SPX_ROWS))
        for r in rows:                                                           # id -> start -> length -> positions -> the row's offsets
            at = t[got["pat"][r]]
            p = patterns[ids[r]]
            assert t[at] == len(p), (key, r)
            for j, o in enumerate(p):
                holds = [c for c in range(nwin) if base[c] <= t[at + 1 + j] < base[c] + size[c]]
                assert len(holds) == 1 and t[at + 1 + j] - base[holds[0]] + omin[holds[0]] == o, (key, r, j)
        stored = len({ids[r] for r in rows}) or 1                                 # a workgroup stores the patterns of its own rows, no others
        assert t[0] == stored and max(got["pat"][r] for r in rows) == stored - 1, (key, g)
        assert sum(1 + max(1, t[t[k]]) for k in range(stored)) + stored <= len(t) < sum(1 + max(1, t[t[k]]) for k in range(stored)) + stored + 4, (key, g)


def pattern_ids(name):
    st = X.named_structure(name)
    rows, cols, M, _ = X.operator(name)
    index = {p: i for i, p in enumerate(st["patterns"])}
    rp = np.concatenate([[0], np.cumsum(st["lens"])])
    rel = (cols.astype(np.int64) - rows).tolist()
    return st["patterns"], [index[tuple(rel[rp[r]:rp[r + 1]])] for r in range(M)], M


def test_the_sellpx_plan_of_every_named_operator(exe):
    names = sorted(X.OPERATORS)
    data = {n: pattern_ids(n) for n in names}
    out = run(exe, [ask_spx(*data[n]) for n in names])
    verdicts = {}
    for n in names:
        patterns, ids, M = data[n]
        want = X.sellpx_plan(patterns, ids, M)
        hold_spx(read_spx(out), want, patterns, ids, M, n)
        verdicts[n] = want["verdict"]
    assert not out
    # (sixteen: 16 windows of 512 doubles, 64 of the 80 KiB)
    assert verdicts.pop("seventeen") == X.SPX_WINDOW_COUNT and set(verdicts.values()) == {X.SPX_OK}


def _dense(S):
    """the offsets of one window of S doubles at the gap rule of SPX_ROWS"""
    return tuple(range(0, S - 512, 512)) + (S - 512,)


SPX_EDGES = {
    # name: (patterns, ids, M, verdict)
    "no entries": ([()], [0] * 10, 10, X.SPX_NO_ENTRIES),
    "sixteen windows": ([tuple(1100 * k for k in range(16))], [0] * 10, 10, X.SPX_OK),
    "seventeen windows": ([tuple(1100 * k for k in range(17))], [0] * 10, 10, X.SPX_WINDOW_COUNT),
    "S of 65535: positions fit, the LDS does not": ([_dense(65535)], [0] * 10, 10, X.SPX_WINDOWS_LDS),
    "S of 65536": ([_dense(65536)], [0] * 10, 10, X.SPX_POSITIONS_16),
    # the room for a workgroup's table, to the word: S = 10239 leaves (81920 - 81912) / 2 = 4 words; the second pattern, which no row
    # follows, only keeps the window in one piece
    "windows one double short of the LDS, a table that fills the room": ([(0, 9727), _dense(10239)[1:-1]], [0] * 10, 10, X.SPX_OK),
    "... and a table one entry larger": ([(0, 512, 9727), _dense(10239)[2:-1]], [0] * 10, 10, X.SPX_TABLE),
    "windows that fill the LDS": ([_dense(10240)], [0] * 10, 10, X.SPX_WINDOWS_LDS),
    "a workgroup of empty rows stores one pattern": ([(0, 1), ()], [0] * 512 + [1] * 100, 612, X.SPX_OK),
    "no row at all": ([(0, 1)], [], 0, X.SPX_OK),
}


def test_every_refusal_of_the_sellpx_plan_at_its_edge(exe):
    names = sorted(SPX_EDGES)
    out = run(exe, [ask_spx(*SPX_EDGES[n][:3]) for n in names])
    seen = set()
    for n in names:
        patterns, ids, M, verdict = SPX_EDGES[n]
        want = X.sellpx_plan(patterns, ids, M)
        assert want["verdict"] == verdict, n
        hold_spx(read_spx(out), want, patterns, ids, M, n)
        seen.add(verdict)
    assert not out and seen == set(range(6))
    fits = X.sellpx_plan(*SPX_EDGES["windows one double short of the LDS, a table that fills the room"][:3])
    assert fits["S"] == 10239 and fits["max_words"] == 4 == (X.SPX_LDS_BYTES - 8 * fits["S"]) // 2


# ---- the slice widths -------------------------------------------------------------------------------------------------------------------
def test_the_slice_widths_of_every_named_operator(exe):
    names = sorted(X.OPERATORS)
    out = run(exe, [f"slices {len(X.named_structure(n)['lens'])} " + " ".join(map(str, np.concatenate([[0], np.cumsum(X.named_structure(n)["lens"])]))) for n in names])
    for n in names:
        st = X.named_structure(n)
        head, ptr = out.pop(0), [int(x) for x in out.pop(0)[1:]]
        assert [b - a for a, b in zip(ptr, ptr[1:])] == [64 * w for w in st["w8"]] and ptr[0] == 0, n
        assert [int(x) for x in head[1:]] == [1, st["w8"][0] if st["uniform"] else 0, 64 * len(st["w8"]) * st["w8"][0] if st["uniform"] else ptr[-1]], n
        assert set(st["w8"]) == PINS[n][0] and st["uniform"] == PINS[n][1], n
    assert not out


def test_slice_widths_at_their_edges(exe):
    """a narrower last slice is padded up, a wider one is not uniform; empty first slices have no common width; 32-bit code positions"""
    big = (INT32_MAX - 1024) // 64 & ~7
    cases = {"narrow last": ([9] * 64 + [3], 16), "wide last": ([3] * 64 + [9], 0), "narrow middle": ([9] * 64 + [3] * 64 + [9], 0), "empty": ([0] * 70, 0),
             "the largest slice": ([big], big), "one group of positions more": ([big + 1], None), "two slices beyond": ([big // 2 + 8] * 65, None)}
    names = sorted(cases)
    out = run(exe, [f"slices {len(cases[n][0])} " + " ".join(map(str, np.concatenate([[0], np.cumsum(cases[n][0], dtype=np.int64)]))) for n in names])
    for n in names:
        lens, uw = cases[n]
        head = [int(x) for x in out.pop(0)[1:]]
        out.pop(0)
        w8 = [(max(lens[s:s + 64]) + 7) & ~7 for s in range(0, len(lens), 64)]
        assert head[:2] == ([0, 0] if uw is None else [1, uw]), n
        if uw is not None:
            assert head[2] == (64 * len(w8) * uw if uw else 64 * sum(w8)), n


# ---- the sanitizers ---------------------------------------------------------------------------------------------------------------------
def test_the_plans_under_the_sanitizers(tmp_path):
    """a stand-alone program with the sanitizer runtimes linked in statically: it runs in whatever environment the suite runs in"""
    exe = str(tmp_path / "sanitize_xwin_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tools", "sanitize_xwin_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
