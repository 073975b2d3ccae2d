"""The mask rows of k_vidxw_fast (saena_amd/csrc/vw_masks.h: a slice of 64 rows as 64-bit lane masks, two bits per (row, slot)) as a
stand-alone host program, compiled with g++ -std=c++17 like tests/test_vw_fast_header.py.

The rule is held on both sides of each clause: eight / nine positions, dictionaries in LDS / in scalar registers, a pattern that skips
back, a longest pattern that repeats a position, two patterns that each lack a different slot with none holding all, the switch.  The
record -- 16 words per slice, presence masks then value masks -- is held by its index functions, and the host pack by a numpy
restatement that never looks at the header's arithmetic: rows are random ordered subsets of 1 ... 8 slots, their codes random bits,
on 1, 4 and 5 slices with a partial last one; rows past nrows leave zeros; a code above 1 and a position without a slot are seen
wherever they stand."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAKEN, NOT_SCALAR, TURNS, REPEATED, NOT_SUBSEQUENCE, SWITCHED_OFF = range(6)
CODE_ABOVE_1, UNMAPPED = 1, 2
NO_SLOT = 0xff

PROGRAM = r"""
#include "vw_masks.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace vwmasks;

static_assert(MAXSLOT == 8 && REC_WORDS == 16 && REC_BYTES == 128 && total_words(5) == 80, "usable in constant expressions");
static_assert(presence_index(3, 2) == 50 && value_index(3, 2) == 58, "usable in constant expressions");
constexpr unsigned char PS[3] = {0, 2, 5};
static_assert(lane_bits(3, PS, [](int j) { return j == 1 ? 1u : 0u; }) == (0x25u | 0x04u << 8), "usable in constant expressions");
static_assert(clause_text(TAKEN)[0] == 't' && clause_text(SWITCHED_OFF)[0] == 'S', "usable in constant expressions");

// per line of stdin, by its first word:
//   rule kind off npat wp, then per pattern its length and wp positions
//        -> "rule <clause> <nslot> <8 slots> <npat * 8 pslot entries>"
//   index ns -> "index" and presence_index / value_index of every (slice, slot), presence first per slice
//   pack ns nrows uw npat, npat lengths, npat * 8 pslot entries, nrows pattern ids, ns * 64 * uw codes in the order [slice][position][lane]
//        -> per slice "pack <flags> <16 words>"
int main() {
    char word[16];
    while (std::scanf("%15s", word) == 1) {
        if (!std::strcmp(word, "rule")) {
            int kind, off, npat, wp;
            if (std::scanf("%d %d %d %d", &kind, &off, &npat, &wp) != 4) return 1;
            std::vector<unsigned short> len((size_t)npat), pos((size_t)npat * wp);
            for (int i = 0; i < npat; ++i) {
                int v;
                if (std::scanf("%d", &v) != 1) return 1;
                len[(size_t)i] = (unsigned short)v;
                for (int j = 0; j < wp; ++j) { if (std::scanf("%d", &v) != 1) return 1; pos[(size_t)i * wp + j] = (unsigned short)v; }
            }
            int nslot = -1, slot[MAXSLOT];
            std::vector<unsigned char> pslot((size_t)npat * MAXSLOT, 0x77);
            const int c = rule(kind, len.data(), pos.data(), npat, wp, off != 0, &nslot, slot, pslot.data());
            std::printf("rule %d %d", c, nslot);
            for (int u = 0; u < MAXSLOT; ++u) std::printf(" %d", slot[u]);
            for (unsigned char b : pslot) std::printf(" %d", (int)b);
            std::printf("\n");
        } else if (!std::strcmp(word, "index")) {
            int ns;
            if (std::scanf("%d", &ns) != 1) return 1;
            std::printf("index");
            for (int s = 0; s < ns; ++s) {
                for (int u = 0; u < MAXSLOT; ++u) std::printf(" %lld", (long long)presence_index(s, u));
                for (int u = 0; u < MAXSLOT; ++u) std::printf(" %lld", (long long)value_index(s, u));
            }
            std::printf("\n");
        } else if (!std::strcmp(word, "pack")) {
            int ns, nrows, uw, npat, v;
            if (std::scanf("%d %d %d %d", &ns, &nrows, &uw, &npat) != 4) return 1;
            std::vector<unsigned short> len((size_t)npat), pid((size_t)nrows);
            std::vector<unsigned char> pslot((size_t)npat * MAXSLOT), code((size_t)ns * 64 * uw);
            for (auto &x : len) { if (std::scanf("%d", &v) != 1) return 1; x = (unsigned short)v; }
            for (auto &x : pslot) { if (std::scanf("%d", &v) != 1) return 1; x = (unsigned char)v; }
            for (auto &x : pid) { if (std::scanf("%d", &v) != 1) return 1; x = (unsigned short)v; }
            for (int s = 0; s < ns; ++s) for (int j = 0; j < uw; ++j) for (int l = 0; l < 64; ++l) {
                if (std::scanf("%d", &v) != 1) return 1;
                code[(size_t)vwfast::code_index(s, j, l, uw)] = (unsigned char)v;
            }
            std::vector<uint64_t> rec((size_t)total_words(ns), ~0ull);
            for (int s = 0; s < ns; ++s) {
                const int flags = pack_slice(s, nrows, pid.data(), len.data(), pslot.data(), code.data(), uw, &rec[(size_t)presence_index(s, 0)]);
                std::printf("pack %d", flags);
                for (int w = 0; w < REC_WORDS; ++w) std::printf(" %llu", (unsigned long long)rec[(size_t)s * REC_WORDS + w]);
                std::printf("\n");
            }
        } else return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("vw_masks_check")
    src, out = str(d / "vw_masks_check.cpp"), str(d / "vw_masks_check")
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


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def rule(exe, patterns, kind=2, off=0, wp=None):
    """patterns: lists of positions -> (clause, nslot, slots, pslot as [npat][8])"""
    wp = wp or max(8, -(-max(len(p) for p in patterns) // 8) * 8)
    line = f"rule {kind} {off} {len(patterns)} {wp}"
    for p in patterns:
        padded = list(p) + [p[-1] if p else 0] * (wp - len(p))        # (the table's tail repeats the last position)
        line += f" {len(p)} " + " ".join(map(str, padded))
    w = [int(x) for x in run(exe, [line])[0][1:]]
    return w[0], w[1], w[2:10], np.array(w[10:], int).reshape(len(patterns), 8)


SEVEN = [8, 800, 1600, 1608, 1616, 2400, 3200]                       # LDS byte offsets of a 7-point interior row, in column order


def subsets(full, drop):
    return [[p for i, p in enumerate(full) if i not in d] for d in drop]


def test_a_seven_point_table_is_taken_and_its_slots_are_the_longest_pattern(exe):
    pats = subsets(SEVEN, [(0,), (), (6,), (0, 1, 2), (0, 2, 6)])      # the longest is not the first
    clause, nslot, slots, pslot = rule(exe, pats)
    assert (clause, nslot, slots) == (TAKEN, 7, SEVEN + [0])
    for p, row in zip(pats, pslot):
        assert [SEVEN[u] for u in row[:len(p)]] == p and (row[len(p):] == NO_SLOT).all() and (np.diff(row[:len(p)]) > 0).all()


def test_eight_positions_are_taken_and_nine_refused(exe):
    eight = [8 * i for i in range(8)]
    assert rule(exe, [eight, eight[:3]])[:3] == (TAKEN, 8, eight)
    nine = [8 * i for i in range(9)]
    assert rule(exe, [nine, nine[:3]], wp=16)[0] == TURNS
    assert rule(exe, [nine[:3], nine], wp=16)[0] == TURNS


def test_dictionaries_in_lds_and_the_general_kernel_are_refused(exe):
    pats = subsets(SEVEN, [(), (0,)])
    assert [rule(exe, pats, kind=k)[0] for k in (0, 1, 2)] == [NOT_SCALAR, NOT_SCALAR, TAKEN]


def test_a_pattern_that_skips_back_is_refused(exe):
    assert rule(exe, [SEVEN, [SEVEN[0], SEVEN[2], SEVEN[5]]])[0] == TAKEN
    assert rule(exe, [SEVEN, [SEVEN[2], SEVEN[0], SEVEN[5]]])[0] == NOT_SUBSEQUENCE
    assert rule(exe, [SEVEN, [SEVEN[0], SEVEN[5], SEVEN[5]]])[0] == NOT_SUBSEQUENCE      # (a slot is used once)
    assert rule(exe, [SEVEN, [SEVEN[0], 4000]])[0] == NOT_SUBSEQUENCE                    # (a position that is no slot)


def test_a_longest_pattern_with_a_repeated_position_is_refused(exe):
    assert rule(exe, [[8, 16, 24, 32], [8, 32]])[0] == TAKEN
    assert rule(exe, [[8, 16, 8, 32], [8, 32]])[0] == REPEATED
    assert rule(exe, [[8, 16, 24, 24], [8]])[0] == REPEATED


def test_two_patterns_that_each_lack_a_different_slot_are_refused_without_a_complete_one(exe):
    a, b = subsets(SEVEN, [(0,), (6,)])
    assert rule(exe, [a, b])[0] == NOT_SUBSEQUENCE and rule(exe, [b, a])[0] == NOT_SUBSEQUENCE
    assert rule(exe, [a, b, SEVEN])[0] == TAKEN


def test_the_switch_comes_last_and_keeps_the_slots(exe):
    pats = subsets(SEVEN, [(), (3,)])
    on, off = rule(exe, pats), rule(exe, pats, off=1)
    assert on[0] == TAKEN and off[0] == SWITCHED_OFF and on[1:3] == off[1:3] and np.array_equal(on[3], off[3])
    assert rule(exe, pats, kind=1, off=1)[0] == NOT_SCALAR
    assert rule(exe, [[0], []])[:3] == (TAKEN, 1, [0] * 8)               # one slot, and an empty pattern beside it


# ---- the record -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", (1, 4, 5))
def test_every_slice_and_slot_has_two_words_of_its_own(exe, ns):
    i = np.array(run(exe, [f"index {ns}"])[0][1:], np.int64)
    assert np.array_equal(i, np.arange(16 * ns))                      # slice-major, presence masks then value masks: 128 bytes a slice


# ---- the pack ---------------------------------------------------------------------------------------------------------------------------
def random_rows(ns, nslot, seed):
    """-> nrows (a partial last slice), pattern lengths, pslot, pattern ids, codes [slice][position][lane]"""
    rng = np.random.default_rng(seed)
    nrows = ns * 64 - (0 if ns == 4 else 23)
    pats = [sorted(rng.choice(nslot, size=n, replace=False).tolist()) for n in rng.integers(1, nslot + 1, size=11)] + [[]]
    pslot = np.full((len(pats), 8), NO_SLOT, int)
    for i, p in enumerate(pats):
        pslot[i, :len(p)] = p
    pid = rng.integers(0, len(pats), size=nrows)
    code = rng.integers(0, 2, size=(ns, 8, 64), dtype=np.uint8)
    return nrows, pats, pslot, pid, code


def pack(exe, ns, nrows, pats, pslot, pid, code):
    line = f"pack {ns} {nrows} 8 {len(pats)} " + " ".join(str(len(p)) for p in pats) + " " + " ".join(map(str, pslot.ravel().tolist()))
    line += " " + " ".join(map(str, np.asarray(pid).tolist())) + " " + " ".join(map(str, code.ravel().tolist()))
    out = run(exe, [line])
    assert len(out) == ns and all(o[0] == "pack" for o in out)
    return [int(o[1]) for o in out], np.array([[int(x) for x in o[2:]] for o in out], np.uint64)


def restated(ns, nrows, pats, pid, code):
    want = np.zeros((ns, 16), np.uint64)
    for r in range(nrows):
        s, l = divmod(r, 64)
        for j, u in enumerate(pats[pid[r]]):
            want[s, u] |= np.uint64(1 << l)
            if code[s, j, l] & 1:
                want[s, 8 + u] |= np.uint64(1 << l)
    return want


@pytest.mark.parametrize("nslot", (1, 4, 7, 8))
@pytest.mark.parametrize("ns", (1, 4, 5))
def test_packing_random_subsets_equals_the_restatement(exe, ns, nslot):
    nrows, pats, pslot, pid, code = random_rows(ns, nslot, 100 * ns + nslot)
    flags, rec = pack(exe, ns, nrows, pats, pslot, pid, code)
    want = restated(ns, nrows, pats, pid, code)
    assert flags == [0] * ns and np.array_equal(rec, want)
    assert not rec[:, nslot:8].any() and not rec[:, 8 + nslot:].any()           # slots the operator does not have
    assert not (rec[:, 8:] & ~rec[:, :8]).any()                                 # a value bit only where the slot is present
    if nrows % 64:
        assert not (rec[-1] >> np.uint64(nrows % 64)).any() and rec[-1].any()   # rows past nrows: zeros
    assert rec[:, :8].any() and (nslot == 1 or (rec[:, :8] != rec[:, 8:]).any())


def test_a_slice_without_rows_is_all_zero(exe):
    nrows, pats, pslot, pid, code = random_rows(4, 7, 5)
    flags, rec = pack(exe, 4, 130, pats, pslot, pid[:130], code)
    assert flags == [0] * 4 and rec[:2].any() and not (rec[2] >> np.uint64(2)).any() and not rec[3].any()


def test_a_code_above_one_and_an_unmapped_position_are_seen_wherever_they_stand(exe):
    pats = [[0, 1, 2, 3, 4, 5, 6, 7]]
    pslot = np.arange(8).reshape(1, 8)
    pid = np.zeros(128, int)
    clean = np.zeros((2, 8, 64), np.uint8)
    assert pack(exe, 2, 128, pats, pslot, pid, clean)[0] == [0, 0]
    for s, j, l, value in ((0, 0, 0, 2), (0, 7, 63, 255), (1, 3, 17, 128), (1, 7, 63, 3)):
        code = clean.copy()
        code[s, j, l] = value
        flags, _ = pack(exe, 2, 128, pats, pslot, pid, code)
        assert flags == [CODE_ABOVE_1 if t == s else 0 for t in range(2)], (s, j, l, value)
    for j in (0, 3, 7):
        bad = pslot.copy()
        bad[0, j] = NO_SLOT
        flags, rec = pack(exe, 2, 128, pats, bad, pid, clean)
        assert flags == [UNMAPPED, UNMAPPED] and not rec[:, j].any()
    # beyond a pattern's length neither is looked at
    short = [[0, 1, 2]]
    ps = np.full((1, 8), NO_SLOT, int)
    ps[0, :3] = (0, 1, 2)
    code = clean.copy()
    code[:, 3:, :] = 9
    assert pack(exe, 2, 128, short, ps, pid, code)[0] == [0, 0]


# ---- the sanitizers ---------------------------------------------------------------------------------------------------------------------
def test_the_rule_and_the_pack_under_the_sanitizers(tmp_path):
    """a stand-alone program with the sanitizer runtimes linked in statically: it runs in whatever environment the suite runs in"""
    out = str(tmp_path / "sanitize_vw_masks")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tools", "sanitize_vw_masks.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("vw_masks.h: the rule's edges and the pack ran clean"), r.stdout + r.stderr
