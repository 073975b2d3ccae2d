"""saena_amd/csrc/forms.h (the SpMV forms by name: their tables, and the autotune's decision as a function of the times) as a
stand-alone host program: the header has no HIP in it, so g++ -std=c++17 compiles and runs it here.

The tables are held to what the tests already say by variant number: the keep-sets of tests/form_table.py in the bit order of
capi.STORAGE_GROUPS, and the names and summation classes of the FORMS catalogue of tests/test_gpu_forms.py.  choose_plan is held to
the plain restatement of tests/plan_choice_ref.py: one named table per clause of the rule, with the outcome written out, and a few
thousand seeded random tables whose times come from a coarse grid, so that ties and the edges of the bands occur.  Times cross
the pipe as float bit patterns: nothing is rounded on the way."""
import os
import subprocess

import numpy as np
import pytest

from tests import form_table, plan_choice_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
XW_ROWS = (0, 256, 512, 1024)
VALID_GRID = [(f, l, xw) for f in (-1, 0, 5, 11, 16, 17, 18) for l in (0, 1, 7, 64, 65) for xw in (-256, 0, 1, 128, 256, 512, 768, 1024, 2048)]

PROGRAM = r"""
#include "forms.h"
#include <cstdio>
#include <cstring>
using namespace forms;

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, sizeof u); return u; }
static float from_bits(unsigned u) { float f; std::memcpy(&f, &u, sizeof f); return f; }

// tables on stdin: "n form lanes xwin direct_lanes" (the fallback), then n lines "form lanes xwin bits-of-ms"
static int choose_tables() {
    int n, ff, fl, fx, dl;
    while (std::scanf("%d %d %d %d %d", &n, &ff, &fl, &fx, &dl) == 5) {
        std::map<Candidate, float> timed;
        for (int i = 0; i < n; ++i) {
            int f, l, x; unsigned u;
            if (std::scanf("%d %d %d %u", &f, &l, &x, &u) != 4) return 1;
            timed[Candidate{f, l, x}] = from_bits(u);
        }
        const PlanChoice c = choose_plan(timed, Candidate{ff, fl, fx}, dl);
        std::printf("%d %d %d %u %d %d %d %u %u\n", c.best.form, c.best.lanes, c.best.xwin_rows, bits(c.ms),
                    c.runner_up.form, c.runner_up.lanes, c.runner_up.xwin_rows, bits(c.runner_up_ms), bits(c.fastest));
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "choose")) return choose_tables();
    static_assert(F_STREAM16 == 0 && F_DENSE == 5 && F_VIDX == 17 && F_COUNT == 18, "the numbers are ABI");
    static_assert(plan_keeps(G_SELLP, F_VIDX, 0) && !plan_keeps(G_XWIN1, F_VIDX, 256), "usable in constant expressions");
    std::printf("counts %d %d\n", (int)F_COUNT, (int)G_COUNT);
    for (int f = 0; f < F_COUNT; ++f) {
        std::printf("name %d %s\n", f, FORM_NAMES[f]);
        std::printf("seq %d ", f);
        for (int l = 1; l <= 64; ++l) std::printf("%d", sequential_sum(f, l) ? 1 : 0);
        std::printf("\n");
        std::printf("is %d %d %d %d %d %d %d\n", f, tile_plan(f), is_dense(f) ? 1 : 0, is_column_major(f) ? 1 : 0, is_row_pattern(f) ? 1 : 0,
                    is_xlds_chunk(f) ? 1 : 0, one_candidate(f) ? 1 : 0);
        for (int vw : {0, 256, 512, 1024}) {
            std::printf("keeps %d %d ", f, vw);
            for (int grp = 0; grp < G_COUNT; ++grp) std::printf("%d", plan_keeps(grp, f, vw) ? 1 : 0);
            std::printf("\n");
        }
    }
    int f, l, x;
    while (std::scanf("%d %d %d", &f, &l, &x) == 3) std::printf("valid %d %d %d %d\n", f, l, x, plan_line_valid(f, l, x) ? 1 : 0);
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("forms_check")
    src, out = str(d / "forms_check.cpp"), str(d / "forms_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "saena_amd", "csrc"), src, "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    return out


@pytest.fixture(scope="module")
def tables(exe):
    """the program's lines by their first word"""
    r = subprocess.run([exe], input="".join(f"{f} {l} {x}\n" for f, l, x in VALID_GRID), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    by = {}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        by.setdefault(word, []).append(rest)
    return by


def catalogue():
    """(variant, kernel name, lanes, summation class) of every form the GPU suite checks"""
    from tests import test_gpu_forms as T
    return [(f.variant, f.name, f.lanes, f.cls == T.SEQ) for f in T.FORMS]


def test_one_name_per_variant(tables):
    assert tables["counts"] == ["18 19"]
    names = dict((int(v), n) for v, n in (line.split(" ", 1) for line in tables["name"]))
    assert sorted(names) == list(range(18))
    seen = set()
    for variant, name, _, _ in catalogue():
        base = names[variant]
        # the catalogue's name: the base name, up to a "*" where the slot/offset split follows, or with its <wide> / <rowbase> / <sorted>
        assert base.startswith(name[:-1]) if name.endswith("*") else (name == base or name.startswith(base + "<")), (variant, name, base)
        seen.add(variant)
    assert seen == set(range(18))


def test_sequential_sum_is_the_catalogue_s_class(tables):
    seq = {int(v): s for v, s in (line.split() for line in tables["seq"])}
    assert sorted(seq) == list(range(18)) and all(len(s) == 64 for s in seq.values())
    for variant, name, lanes, sequential in catalogue():
        assert (seq[variant][lanes - 1] == "1") == sequential, (variant, name, lanes)
    for variant, s in seq.items():                     # beyond the catalogue's lanes: a lane per row always, a tile form at one lane only
        want = "1" * 64 if variant in plan_choice_ref.SEQUENTIAL else "1" + "0" * 63 if variant in plan_choice_ref.TILE_FORMS else "0" * 64
        assert s == want, variant


def test_predicates(tables):
    got = {int(r[0]): tuple(int(x) for x in r[1:]) for r in (line.split() for line in tables["is"])}
    for v in range(18):
        tile = 0 if v in (0, 3, 7) else 1 if v in (1, 4, 8) else -1
        keeps = form_table.KEEPS[v]
        lane_per_row = v in plan_choice_ref.SEQUENTIAL or v == 12          # k_sellx: a lane per row piece
        assert got[v] == (tile, int(v == 5), int(v in plan_choice_ref.COLUMN_MAJOR), int("sellp" in keeps), int("xlds_plan" in keeps),
                          int(lane_per_row or v == 5)), v


def test_plan_keeps_is_the_keep_set_of_every_variant(tables):
    from saena_amd import capi
    groups = capi.STORAGE_GROUPS
    got = {(int(v), int(vw)): m for v, vw, m in (line.split() for line in tables["keeps"])}
    assert sorted(got) == [(v, vw) for v in range(18) for vw in XW_ROWS]
    assert sorted(form_table.KEEPS) == list(range(18))
    for (v, vw), mask in got.items():
        assert len(mask) == len(groups)
        assert {g for g, bit in zip(groups, mask) if bit == "1"} == form_table.kept(v, vw), (v, vw)


def test_a_plan_cache_line_is_valid_as_restated(tables):
    got = {tuple(int(x) for x in line.split()[:3]): line.split()[3] == "1" for line in tables["valid"]}
    assert len(got) == len(VALID_GRID)
    for key in VALID_GRID:
        assert got[key] == form_table.plan_line_valid(*key), key
    assert got[(17, 1, 512)] and not got[(11, 1, 512)] and not got[(18, 1, 0)] and not got[(17, 65, 0)] and not got[(17, 1, 768)]


# ---- choose_plan ----------------------------------------------------------------------------------------------------------------
def bits(t):
    return int(np.asarray(t, F32).view(np.uint32))


def run_choose(exe, cases):
    """cases: (table, fallback, direct_lanes) -> per case (chosen, bits of ms, runner-up or None, bits of its ms, bits of fastest)"""
    text = []
    for table, fallback, direct_lanes in cases:
        text.append(f"{len(table)} {fallback[0]} {fallback[1]} {fallback[2]} {direct_lanes}\n")
        text += [f"{f} {l} {xw} {bits(ms)}\n" for f, l, xw, ms in table]
    r = subprocess.run([exe, "choose"], input="".join(text), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        v = [int(x) for x in line.split()]
        out.append((tuple(v[0:3]), v[3], tuple(v[4:7]) if v[4] >= 0 else None, v[7], v[8]))
    assert len(out) == len(cases)
    return out


def restated(case):
    pick, ms, ru, ru_ms, fastest = plan_choice_ref.choose(*case)
    return pick, bits(ms), ru, bits(ru_ms), bits(fastest)


ONE = F32(1.0)
BAR = F32(1.03) * ONE
FALLBACK = (3, 4, 0)
# name -> (table of (form, lanes, xwin, ms), direct lanes, chosen, runner-up)
NAMED = {
    "1 a sequential form inside the band beats a faster tree form":
        ([(2, 8, 0, 1.00), (11, 1, 0, 1.02)], 1, (11, 1, 0), (2, 8, 0)),
    "2 two sequential forms inside the band: the faster":
        ([(2, 8, 0, 1.00), (11, 1, 0, 1.02), (14, 1, 0, 1.01)], 1, (14, 1, 0), (2, 8, 0)),
    "3 two tree forms inside the band: the lower (form, lanes), even if slower":
        ([(6, 8, 0, 1.01), (2, 8, 0, 1.00), (2, 4, 0, 1.02)], 1, (2, 4, 0), (2, 8, 0)),
    "4a exactly at the bar: in":
        ([(2, 8, 0, ONE), (11, 1, 0, BAR)], 1, (11, 1, 0), (2, 8, 0)),
    "4b one ulp above the bar: out":
        ([(2, 8, 0, ONE), (11, 1, 0, np.nextafter(BAR, F32(2)))], 1, (2, 8, 0), (11, 1, 0)),
    "5a column-major at 0.96: does not win, and is excluded":
        ([(2, 8, 0, 1.00), (8, 4, 0, 0.96), (8, 1, 0, 0.97)], 1, (2, 8, 0), (8, 4, 0)),
    "5b column-major at 0.94: wins, and only column-major competes":
        ([(2, 8, 0, 1.00), (11, 1, 0, 0.995), (8, 4, 0, 0.94), (8, 1, 0, 0.96)], 1, (8, 1, 0), (8, 4, 0)),
    "6a x windows fastest, direct gathers inside the band: direct":
        ([(17, 1, 0, 1.02), (17, 1, 256, 1.00), (2, 8, 0, 1.20)], 1, (17, 1, 0), (17, 1, 256)),
    "6b x windows fastest, direct gathers outside the band: the mode":
        ([(17, 1, 0, 1.05), (17, 1, 256, 1.00), (2, 8, 0, 1.20)], 1, (17, 1, 256), (17, 1, 0)),
    "7 nothing timed: the plan in force, no runner-up":
        ([], 1, FALLBACK, None),
    "8 a single candidate: no runner-up":
        ([(2, 8, 0, 1.00)], 1, (2, 8, 0), None),
    "9 runner-up ties: the first in order":
        ([(6, 8, 0, 1.50), (2, 8, 0, 1.50), (11, 1, 0, 1.00), (2, 4, 0, 1.50)], 1, (11, 1, 0), (2, 4, 0)),
}


def test_choose_plan_clause_by_clause(exe):
    names = sorted(NAMED)
    cases = [(NAMED[n][0], FALLBACK, NAMED[n][1]) for n in names]
    for name, case, got in zip(names, cases, run_choose(exe, cases)):
        _, _, chosen, runner_up = NAMED[name]
        times = {(f, l, xw): bits(ms) for f, l, xw, ms in case[0]}
        assert got[0] == chosen and got[2] == runner_up, (name, got)
        assert got[1] == times.get(chosen, bits(0.0)) and got[3] == (times[runner_up] if runner_up else bits(0.0)), (name, got)
        assert got == restated(case), (name, got, restated(case))
    assert (F32(0.96) < F32(0.95) * ONE, F32(0.94) < F32(0.95) * ONE) == (False, True)


def random_cases(n, seed=20240611):
    rng = np.random.default_rng(seed)
    lanes = (1, 2, 4, 8, 16, 32, 64)
    cases = []
    for _ in range(n):
        direct_lanes = int(rng.choice((1, 2, 4)))
        base = F32(rng.choice((0.25, 1.0, 3.5)))
        # a coarse grid around the base, and the exact edges of the two bands and their neighbours
        grid = [base * F32(1 + 0.01 * k) for k in range(-8, 9)]
        grid += [F32(1.03) * base, np.nextafter(F32(1.03) * base, F32(9)), F32(0.95) * base, np.nextafter(F32(0.95) * base, F32(0))]
        table = {}
        for _ in range(int(rng.integers(0, 9))):
            f = int(rng.choice((7, 8, 17))) if rng.random() < 0.4 else int(rng.integers(0, 18))
            xw = int(rng.choice(XW_ROWS)) if f == 17 else 0
            l = direct_lanes if xw or (f == 17 and rng.random() < 0.7) else int(rng.choice(lanes))
            table[(f, l, xw)] = F32(base if rng.random() < 0.2 else grid[int(rng.integers(len(grid)))])
        rows = [(f, l, xw, ms) for (f, l, xw), ms in table.items()]
        fallback = (int(rng.integers(0, 18)), int(rng.choice(lanes)), 0)
        cases.append((rows, fallback, direct_lanes))
    return cases


def test_choose_plan_agrees_with_the_restatement_on_random_tables(exe):
    cases = random_cases(4000)
    got = run_choose(exe, cases)
    bad = [(c, g, restated(c)) for c, g in zip(cases, got) if g != restated(c)]
    assert not bad, (len(bad), bad[0])
    # the draw reaches every clause: sequential and tree winners, column-major winners and losers, the mode chosen and overruled
    chosen = [g[0] for g in got]
    assert any(c[0] in (7, 8) for c in chosen) and any(c[2] for c in chosen) and any(c[0] == 2 for c in chosen)
    def overruled(rows, dl, g):                        # direct gathers chosen although a window size was faster
        return g[0] == (17, dl, 0) and any(f == 17 and xw and bits(ms) < g[1] for f, _, xw, ms in rows)
    assert any(overruled(rows, dl, g) for (rows, _, dl), g in zip(cases, got))
