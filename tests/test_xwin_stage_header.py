"""saena_amd/csrc/xwin_stage.h (how k_vidxw stages its windows of x one by one: the rule that picks this staging, and the map
(lane, trip) -> (LDS slot, column - r0)) as a stand-alone host program: the header has no HIP in it, so g++ -std=c++17 compiles and
runs it here.

For every named operator of tests/xwin_ref.py that the x-window mode accepts, at every workgroup size, the rule is held to its plain
restatement below, and where it says "window by window" the map is walked lane by lane: every LDS slot 0 ... S - 1 is written exactly
once, with the column the window holds there; a lane past its window's size writes the spare slot S and nothing else; the byte offset a
lane hands the buffer load is inside the descriptor (below 8 ncols, as an unsigned number) exactly where its column is inside x, in the
first and in the last workgroup."""
import os
import subprocess

import pytest

from tests import xwin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC_COLS = 1 << 28
MAX_TRIPS = 6

PROGRAM = r"""
#include "xwin_stage.h"
#include <cstdio>
#include <vector>
using namespace xwstage;

// per line of stdin: R ncols nrows r0 nwin, then nwin x (base omin size)
//   -> "rule <0|1> ntrip <n>", and where the rule holds, per trip "trip lds col cnt" and per lane "l slot column offset"
int main() {
    static_assert(per_window(4, 1024, 256, 100, 100, -3, 3) && !per_window(5, 1024, 256, 100, 100, -3, 3), "usable in constant expressions");
    long long R, ncols, nrows, r0;
    int nwin;
    while (std::scanf("%lld %lld %lld %lld %d", &R, &ncols, &nrows, &r0, &nwin) == 5) {
        std::vector<int> base(nwin), omin(nwin), size(nwin);
        long long S = 0;
        for (int c = 0; c < nwin; ++c) { if (std::scanf("%d %d %d", &base[c], &omin[c], &size[c]) != 3) return 1; S += size[c]; }
        const bool rule = per_window(nwin, S, (int)R, ncols, nrows, omin.front(), omin.back() + size.back() - R);
        Trip t[MAX_TRIPS];
        const int n = rule ? trips(nwin, base.data(), omin.data(), size.data(), (int)R, t) : 0;
        std::printf("rule %d ntrip %d\n", rule ? 1 : 0, n);
        if (!rule) continue;
        for (int u = 0; u < MAX_TRIPS; ++u) {
            std::printf("trip %d %d %d\n", t[u].lds, t[u].col, t[u].cnt);
            for (int l = 0; l < R; ++l) {
                std::printf("l %d %d %u\n", slot(t[u], l, (int)S), column(t[u], l), byte_offset((int)r0, t[u], l));
            }
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("xwin_stage_check")
    src, out = str(d / "xwin_stage_check.cpp"), str(d / "xwin_stage_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "saena_amd", "csrc"), src, "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    return out


def run(exe, cases):
    """cases: (R, ncols, nrows, r0, [(base, omin, size)]) -> per case (rule, ntrip, [(lds, col, cnt)], [[(slot, column, offset) per lane] per trip])"""
    text = "".join(f"{R} {ncols} {nrows} {r0} {len(win)} " + " ".join(f"{b} {o} {s}" for b, o, s in win) + "\n" for R, ncols, nrows, r0, win in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "rule":
            out.append((w[1] == "1", int(w[3]), [], []))
        elif w[0] == "trip":
            out[-1][2].append(tuple(int(x) for x in w[1:]))
            out[-1][3].append([])
        else:
            out[-1][3][-1].append(tuple(int(x) for x in w[1:]))
    assert len(out) == len(cases)
    return out


def layout(g):
    """the windows of a geometry as build_xwin lays them out: [(LDS base, omin, size)]"""
    win, base = [], 0
    for lo, hi in g["windows"]:
        win.append((base, lo, g["R"] + hi - lo))
        base += win[-1][2]
    assert base == g["S"]
    return win


def rule(nwin, S, R, ncols, nrows, omin_first, omax_last):
    """the staging is window by window where: at most four windows, at most 4 R doubles, and every column a lane can ask for -- from the
    first window's start in the first workgroup to a whole trip behind the last window's end in the last -- has a byte offset of
    magnitude below 2^31, as has the end of x"""
    return 1 <= nwin <= 4 and S <= 4 * R and ncols < DESC_COLS and omin_first >= -DESC_COLS and nrows + omax_last + 2 * R <= DESC_COLS


ACCEPTED = [(name, R) for name in sorted(xwin_ref.OPERATORS) for R in xwin_ref.ROWS if xwin_ref.named_geometry(name, R)["verdict"] == xwin_ref.OK]


def test_the_named_operators_reach_both_stagings():
    paths = {(name, R): (g["nwin"] <= 4 and g["S"] <= 4 * R) for name, R in ACCEPTED for g in [xwin_ref.named_geometry(name, R)]}
    assert len(ACCEPTED) >= 30 and any(paths.values()) and not all(paths.values())
    assert paths[("four", 256)] and not paths[("five", 256)] and not paths[("comb", 256)] and paths[("tall", 512)] and paths[("flat", 1024)]
    # (none of them needs more than four trips: test_the_rule_at_its_edges builds the layout that needs six)


def test_every_slot_once_with_its_column_and_the_rest_to_the_spare_slot(exe):
    cases, geoms = [], []
    for name, R in ACCEPTED:
        g = xwin_ref.named_geometry(name, R)
        _, _, M, N = xwin_ref.operator(name)
        for r0 in (0, (M - 1) // R * R):                       # the first and the last workgroup
            cases.append((R, N, M, r0, layout(g)))
            geoms.append((name, g, M, N, r0))
    for (name, g, M, N, r0), (ok, ntrip, trips, lanes) in zip(geoms, run(exe, cases)):
        R, S, win = g["R"], g["S"], layout(g)
        key = (name, R, r0)
        assert ok == rule(g["nwin"], S, R, N, M, win[0][1], g["windows"][-1][1]) == (g["nwin"] <= 4 and S <= 4 * R), key
        if not ok:
            assert ntrip == 0, key
            continue
        assert ntrip == sum(-(-s // R) for _, _, s in win) <= MAX_TRIPS and len(trips) == MAX_TRIPS, key
        want = {b + i: o + i for b, o, s in win for i in range(s)}            # slot -> column - r0
        assert sorted(want) == list(range(S)), key
        seen = {}
        for u, ((lds, col, cnt), per_lane) in enumerate(zip(trips, lanes)):
            assert len(per_lane) == R and (0 < cnt <= R if u < ntrip else cnt == 0), (key, u)
            for l, (slot, column, off) in enumerate(per_lane):
                if l < cnt:
                    assert slot not in seen and slot < S, (key, u, l)
                    seen[slot] = column
                else:
                    assert slot == S, (key, u, l)                               # past the window: the spare slot only
                c = r0 + column
                if u < ntrip:
                    assert off == (8 * c) % 2 ** 32 and (off < 8 * N) == (0 <= c < N), (key, u, l, off)
                else:
                    assert off >= 2 ** 31 and off + 8 <= 2 ** 32, (key, u, l, off)     # an unused trip loads nothing
        assert seen == want, key


def test_the_rule_at_its_edges(exe):
    R = 256
    def wins(sizes, first=-3000, gap=1500):
        out, base = [], 0
        for c, s in enumerate(sizes):
            out.append((base, first + c * (R + gap), s)); base += s
        return out
    cases = {
        "four windows, S = 4 R": ((R, 12000, 12000, 0, wins([R] * 4)), True, 4),
        "five windows": ((R, 12000, 12000, 0, wins([R] * 5)), False, 0),
        "one window of 4 R": ((R, 12000, 12000, 0, wins([4 * R])), True, 4),
        "S = 4 R + 1": ((R, 12000, 12000, 0, wins([4 * R + 1])), False, 0),
        "S = 4 R + 1 in three windows": ((R, 12000, 12000, 0, wins([R + 1, 2 * R, R])), False, 0),
        "three windows, six trips": ((R, 12000, 12000, 0, wins([R + 1, R + 2, R + 3])), True, 6),
        "x one short of the descriptor's reach": ((R, DESC_COLS - 1, 12000, 0, wins([R] * 3)), True, 3),
        "x beyond the descriptor's reach": ((R, DESC_COLS, 12000, 0, wins([R] * 3)), False, 0),
        "rows whose windows end beyond it": ((R, 12000, DESC_COLS - 2 * R, 0, wins([R] * 3, first=0, gap=0)), False, 0),
        "a window that begins before it": ((R, 12000, 12000, 0, wins([R] * 3, first=-DESC_COLS - 1)), False, 0),
    }
    names = sorted(cases)
    for name, (ok, ntrip, trips, _) in zip(names, run(exe, [cases[n][0] for n in names])):
        assert (ok, ntrip) == cases[name][1:], name
        _, ncols, nrows, _, win = cases[name][0]
        assert ok == rule(len(win), sum(s for _, _, s in win), R, ncols, nrows, win[0][1], win[-1][1] + win[-1][2] - R), name
