"""saena_amd/csrc/vw_fast.h (which operator x workgroup size and which launch take k_vidxw_fast, the common path of k_vidxw as a kernel
of its own, and the part of its argument that build_xwin computes once) as a stand-alone host program: the header has no HIP in it, so
g++ -std=c++17 compiles and runs it here.

The rule is held to every clause at its edge, on both sides.  For every named operator of tests/xwin_ref.py that the x-window mode
accepts, at R = 256 and 512 and with dictionaries of one, two and five values, the rule's verdict and -- where it takes the operator --
every precomputed field of VwFast are held to a plain numpy restatement: the trips in bytes with the unused ones substituted, the LDS
carve-up with and without the dictionaries, the body of the row loop's first turn, and the XCD remap's constants, with which the
remap must be a permutation of the workgroups."""
import os
import subprocess

import numpy as np
import pytest

from tests import xwin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (256, 512)
TAKEN, C_ROWS, C_WIDTHS, C_DICTS, C_TRIPS, C_TABLE, C_OFF = range(7)
OFF_NONE8 = 1 << 28
FIELDS = ("nblk rq rr cbytes n8 vd_u ngd xbytes S8 dict_off tab_off pos_off pw2 w8 lmin lmax body0 lds").split()

PROGRAM = r"""
#include "vw_fast.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace vwfast;

static_assert(refused(256, 8, 2, 4, 256) == TAKEN && refused(1024, 8, 2, 4, 256) == ROWS && kind(TAKEN, 2) == 2 && kind(TAKEN, 3) == 1 && kind(WIDTHS, 1) == 0,
              "usable in constant expressions");
static_assert(body(7, 7, 0) == 7 && remap(9, 2, 3) == 4, "usable in constant expressions");

// per line of stdin, by its first word:
//   rule R uw vd_u ntrip n8                 -> "rule <clause> <kind> <text>"
//   launch kind halo epi                    -> "launch <0|1>"
//   body lmin lmax j                        -> "body <index> <positions> <free4>"
//   remap n                                 -> "remap b(0) ... b(n - 1)" with rq = n / 8, rr = n % 8
//   plan R nslices ncols S lp words wp uw vd_u lmin lmax sd nwin, nwin x (base omin size)
//                                           -> "plan <FIELDS in order>" and "trip lds8 col cnt" four times
int main() {
    char word[16];
    while (std::scanf("%15s", word) == 1) {
        if (!std::strcmp(word, "rule")) {
            int R, uw, vd, nt, n8;
            if (std::scanf("%d %d %d %d %d", &R, &uw, &vd, &nt, &n8) != 5) return 1;
            const int c = refused(R, uw, vd, nt, n8);
            std::printf("rule %d %d %s\n", c, kind(c, vd), clause_text(c));
        } else if (!std::strcmp(word, "launch")) {
            int k, halo, epi;
            if (std::scanf("%d %d %d", &k, &halo, &epi) != 3) return 1;
            std::printf("launch %d\n", launch_takes(k, halo != 0, epi) ? 1 : 0);
        } else if (!std::strcmp(word, "body")) {
            int lmin, lmax, j;
            if (std::scanf("%d %d %d", &lmin, &lmax, &j) != 3) return 1;
            const int b = body(lmin, lmax, j);
            std::printf("body %d %d %d\n", b, body_positions(b), body_free4(b) ? 1 : 0);
        } else if (!std::strcmp(word, "remap")) {
            int n;
            if (std::scanf("%d", &n) != 1) return 1;
            std::printf("remap");
            for (int b = 0; b < n; ++b) std::printf(" %d", remap(b, n / NXCD, n % NXCD));
            std::printf("\n");
        } else if (!std::strcmp(word, "plan")) {
            int R, ns, ncols, S, lp, words, wp, uw, vd, lmin, lmax, sd, nwin;
            if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d", &R, &ns, &ncols, &S, &lp, &words, &wp, &uw, &vd, &lmin, &lmax, &sd, &nwin) != 13) return 1;
            std::vector<int> base(nwin), omin(nwin), size(nwin);
            for (int c = 0; c < nwin; ++c) if (std::scanf("%d %d %d", &base[c], &omin[c], &size[c]) != 3) return 1;
            xwstage::Trip t[xwstage::MAX_TRIPS];
            if (xwstage::trips(nwin, base.data(), omin.data(), size.data(), R, t) == 0) return 2;
            VwFast f{};
            const int lds = plan(f, R, ns, ncols, S, lp, words, wp, uw, vd, lmin, lmax, t, sd != 0);
            std::printf("plan %d %d %d %d %d %d %d %u %d %d %d %d %d %d %d %d %d %d\n", f.nblk, f.rq, f.rr, f.cbytes, f.n8, f.vd_u, f.ngd, f.xbytes, f.S8, f.dict_off,
                        f.tab_off, f.pos_off, f.pw2, f.w8, f.lmin, f.lmax, f.body0, lds);
            for (int u = 0; u < TRIPS; ++u) std::printf("trip %d %d %d\n", f.trip[u].lds8, f.trip[u].col, f.trip[u].cnt);
        } else return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("vw_fast_check")
    src, out = str(d / "vw_fast_check.cpp"), str(d / "vw_fast_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "saena_amd", "csrc"), src, "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    return out


def run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.splitlines()]


# ---- the plain restatement ----------------------------------------------------------------------------------------------------------------
def rule(R, uw, vd_u, ntrip, n8):
    """the first clause that refuses, in the order the issue states them"""
    if R not in (256, 512):
        return C_ROWS
    if uw == 0:
        return C_WIDTHS
    if vd_u == 0:
        return C_DICTS
    if not 1 <= ntrip <= 4:
        return C_TRIPS
    if n8 > R:
        return C_TABLE
    return TAKEN


def kind(clause, vd_u):
    return 0 if clause != TAKEN else 2 if vd_u <= 2 else 1


def body(lmin, lmax, j):
    """positions computed in the turn that begins at j (4 ... 8) and whether its first four take no select -> the index"""
    n = min(8, max(4, lmax - j))
    return 2 * (n - 4) + int(j + 4 <= lmin)


def operator_numbers(name, R):
    """what build_xwin hands vwfast::plan for a named operator, from tests/xwin_ref.py's restatement of the geometry"""
    g = xwin_ref.named_geometry(name, R)
    _, _, M, N = xwin_ref.operator(name)
    win, base = [], 0
    for lo, hi in g["windows"]:
        win.append((base, lo, R + hi - lo))
        base += win[-1][2]
    per_window = g["nwin"] <= 4 and g["S"] <= 4 * R
    ntrip = sum(-(-s // R) for _, _, s in win) if per_window else 0
    lp, wp = (g["npat"] + 7) & ~7, (g["W"] + 7) & ~7
    assert g["words"] == lp + g["npat"] * wp
    return dict(g=g, M=M, N=N, win=win, ntrip=ntrip, lp=lp, wp=wp, uw=g["w8"][0] if g["uniform"] else 0, ns=(M + 63) // 64,
                lmin=int(g["lens"].min()), lmax=int(g["lens"].max()))


ELIGIBLE = ["flat", "four", "holes", "tall", "tiny", "wide19"]            # one slice width, one to four windows of at most 4 R doubles, at both R
ACCEPTED = [(name, R) for name in sorted(xwin_ref.OPERATORS) for R in ROWS if xwin_ref.named_geometry(name, R)["verdict"] == xwin_ref.OK]


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def test_every_clause_at_its_edge_on_both_sides(exe):
    cases = {
        "256 rows": ((256, 8, 2, 4, 256), TAKEN, 2), "512 rows": ((512, 8, 2, 4, 512), TAKEN, 2),
        "1024 rows": ((1024, 8, 2, 4, 256), C_ROWS, 0), "128 rows": ((128, 8, 2, 1, 1), C_ROWS, 0), "384 rows": ((384, 8, 2, 1, 1), C_ROWS, 0),
        "one width": ((256, 8, 3, 2, 10), TAKEN, 1), "slice pointers": ((256, 0, 3, 2, 10), C_WIDTHS, 0),
        "one value": ((256, 8, 1, 2, 10), TAKEN, 2), "two values": ((256, 8, 2, 2, 10), TAKEN, 2), "three values": ((256, 8, 3, 2, 10), TAKEN, 1),
        "256 values": ((512, 16, 256, 2, 10), TAKEN, 1), "dictionaries that differ": ((256, 8, 0, 2, 10), C_DICTS, 0),
        "one trip": ((256, 8, 5, 1, 10), TAKEN, 1), "four trips": ((256, 8, 5, 4, 10), TAKEN, 1), "five trips": ((256, 8, 5, 5, 10), C_TRIPS, 0),
        "six trips": ((512, 8, 5, 6, 10), C_TRIPS, 0), "flat staging": ((256, 8, 5, 0, 10), C_TRIPS, 0),
        "R chunks at 256": ((256, 8, 5, 3, 256), TAKEN, 1), "R + 1 chunks at 256": ((256, 8, 5, 3, 257), C_TABLE, 0),
        "R chunks at 512": ((512, 8, 5, 3, 512), TAKEN, 1), "R + 1 chunks at 512": ((512, 8, 5, 3, 513), C_TABLE, 0), "one chunk": ((512, 8, 5, 3, 1), TAKEN, 1),
        "the first clause that refuses is named": ((1024, 0, 0, 0, 5000), C_ROWS, 0), "... the second": ((256, 0, 0, 0, 5000), C_WIDTHS, 0),
        "... the third": ((256, 8, 0, 0, 5000), C_DICTS, 0), "... the fourth": ((256, 8, 2, 0, 5000), C_TRIPS, 0),
    }
    names = sorted(cases)
    out = run(exe, ["rule " + " ".join(map(str, cases[n][0])) for n in names])
    texts = {}
    for n, w in zip(names, out):
        args, clause, k = cases[n]
        assert (rule(*args), kind(rule(*args), args[2])) == (clause, k), n          # the restatement agrees with the table
        assert (int(w[1]), int(w[2])) == (clause, k), (n, w)
        texts.setdefault(clause, " ".join(w[3:]))
    assert len(set(texts.values())) == len(texts) == 6 and texts[TAKEN] == "taken"


def test_which_launch_takes_it(exe):
    """no halo, and the product (0), the residual (1) or the Jacobi sweep (2); the Chebyshev steps (3, 4), u -= A e (5) and the
    restriction's sweep (6) keep the general kernel, as does every launch of an operator the rule refused"""
    cases = [(k, halo, epi) for k in (0, 1, 2) for halo in (0, 1) for epi in range(-1, 8)]
    out = run(exe, [f"launch {k} {halo} {epi}" for k, halo, epi in cases])
    for (k, halo, epi), w in zip(cases, out):
        assert int(w[1]) == int(k != 0 and not halo and epi in (0, 1, 2)), (k, halo, epi)


def test_the_row_loops_body(exe):
    cases = [(lmin, lmax, j) for lmax in range(0, 20) for lmin in range(0, lmax + 1) for j in (0, 8, 16)]
    out = run(exe, [f"body {a} {b} {j}" for a, b, j in cases])
    seen = set()
    for (lmin, lmax, j), w in zip(cases, out):
        b = body(lmin, lmax, j)
        assert [int(x) for x in w[1:]] == [b, 4 + b // 2, b % 2], (lmin, lmax, j)
        seen.add(b)
    assert seen == set(range(10))
    assert body(7, 7, 0) == 7 and body(3, 3, 0) == 0 and body(8, 8, 0) == 9 and body(5, 9, 8) == 0 and body(8, 16, 8) == 8 and body(0, 3, 0) == 0


def test_the_remap_is_a_permutation_of_the_workgroups(exe):
    sizes = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 7814]                      # (7 814: the 128^3 level at 256 rows)
    for n, w in zip(sizes, run(exe, [f"remap {n}" for n in sizes])):
        b = np.array(w[1:], int)
        assert sorted(b) == list(range(n)), n
        per, rem = divmod(n, 8)                                                # the blocks bx = x (mod 8) take consecutive workgroups
        for x in range(min(8, n)):
            own = b[x::8][:per + (x < rem)]
            assert list(own) == list(range(x * per + min(x, rem), x * per + min(x, rem) + len(own))), (n, x)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def test_the_named_operators_reach_both_verdicts():
    verdict = {(name, R): rule(R, o["uw"], 2, o["ntrip"], o["g"]["words"] // 8) for name, R in ACCEPTED for o in [operator_numbers(name, R)]}
    assert len(ACCEPTED) >= 20 and not verdict.get(("sixteen", 512))      # (sixteen at 512 rows: beyond the LDS cap, the mode itself refuses)
    assert verdict[("four", 256)] == verdict[("tall", 512)] == verdict[("holes", 256)] == verdict[("tiny", 512)] == TAKEN
    # (comb: rows of 6 ... 11 entries, slices of 8 and of 16 positions -- the width clause stands before the trips')
    assert verdict[("steps", 256)] == verdict[("comb", 256)] == verdict[("sixteen", 256)] == C_WIDTHS
    assert verdict[("five", 256)] == verdict[("gaps", 512)] == verdict[("seven", 256)] == C_TRIPS
    assert sorted({name for (name, R), c in verdict.items() if c == TAKEN}) == ELIGIBLE


@pytest.mark.parametrize("vd_u", [1, 2, 5])
def test_the_precomputed_fields_of_every_accepted_geometry(exe, vd_u):
    lines, want = [], []
    for name, R in ACCEPTED:
        o = operator_numbers(name, R)
        g = o["g"]
        clause = rule(R, o["uw"], vd_u, o["ntrip"], g["words"] // 8)
        lines.append(f"rule {R} {o['uw']} {vd_u} {o['ntrip']} {g['words'] // 8}")
        want.append(("rule", name, R, clause))
        if clause != TAKEN:
            continue
        sd = int(vd_u <= 2)
        lines.append(f"plan {R} {o['ns']} {o['N']} {g['S']} {o['lp']} {g['words']} {o['wp']} {o['uw']} {vd_u} {o['lmin']} {o['lmax']} {sd} {len(o['win'])} "
                     + " ".join(f"{b} {lo} {s}" for b, lo, s in o["win"]))
        want.append(("plan", name, R, o, sd))
        want += [("trip", name, R, u) for u in range(4)]
    out = run(exe, lines)
    assert len(out) == len(want)
    taken = 0
    for w, (what, name, R, *rest) in zip(out, want):
        key = (name, R, vd_u)
        if what == "rule":
            assert (int(w[1]), int(w[2])) == (rest[0], kind(rest[0], vd_u)), key
        elif what == "plan":
            o, sd = rest
            g, S = o["g"], o["g"]["S"]
            nwg = -(-o["ns"] // (R // 64))
            dict_off = 8 * ((S + 2) & ~1)
            tab_off = dict_off + (0 if sd else R // 256 * xwin_ref.VI_MAX * 8)
            expect = dict(nblk=o["ns"], rq=nwg // 8, rr=nwg % 8, cbytes=64 * o["uw"], n8=g["words"] // 8, vd_u=vd_u, ngd=(o["ns"] + 3) // 4, xbytes=8 * o["N"], S8=8 * S,
                          dict_off=dict_off, tab_off=tab_off, pos_off=tab_off + 2 * o["lp"], pw2=2 * o["wp"], w8=o["uw"], lmin=o["lmin"], lmax=o["lmax"],
                          body0=body(o["lmin"], o["lmax"], 0), lds=tab_off + 2 * g["words"])
            assert dict(zip(FIELDS, (int(x) for x in w[1:]))) == expect, key
            assert expect["lds"] == g["lds"] - (R // 256 * xwin_ref.VI_MAX * 8 if sd else 0) <= xwin_ref.VW_MAX_LDS, key      # k_vidxw's layout, less the dictionaries
            assert 1 <= expect["n8"] <= R and expect["pos_off"] % 16 == 0 and expect["tab_off"] % 16 == 0, key
            trips = [(8 * (b + i0), lo + i0, min(R, s - i0)) for b, lo, s in o["win"] for i0 in range(0, s, R)]
            assert 1 <= len(trips) <= 4, key
            trips += [(0, OFF_NONE8, 0)] * (4 - len(trips))                     # an unused trip: no lane of it stages, its columns are beyond every x
            taken += 1
        else:
            assert tuple(int(x) for x in w[1:]) == trips[rest[0]], (key, rest[0])
            lds8, col, cnt = trips[rest[0]]
            assert 0 <= cnt <= R and lds8 + 8 * cnt <= 8 * S, key                 # the staged lanes stay inside the windows
    assert taken == 2 * len(ELIGIBLE)
