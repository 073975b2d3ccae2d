"""The bit codes of k_vidxw_fast (saena_amd/csrc/vw_fast.h: one bit per entry where a dictionary holds at most two values) as a
stand-alone host program, compiled with g++ -std=c++17 like tests/test_vw_fast_header.py.

The rule is held on both sides of each clause (dictionaries of 1, 2 and 3 values; an operator the lean kernel refuses; the switch).
The layout -- byte [slice][turn j / 8][lane], bit u = bit 0 of the code of position j + u, a slice of 8 uw bytes, one turn of padding
behind the last slice -- is held for uw in {8, 16, 24} and 1, 4 and 5 slices: every (slice, turn, lane) has a byte of its own inside
the array, and packing random 0 / 1 codes through the header's two indices and its pack8 equals numpy's packbits over the position
axis of the codes as a plain [slice][position][lane] array, which never looks at the header's arithmetic."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS, SLICES = (8, 16, 24), (1, 4, 5)

PROGRAM = r"""
#include "vw_fast.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace vwfast;

static_assert(bit_codes(2, false) && !bit_codes(2, true) && !bit_codes(1, false) && !bit_codes(0, false), "usable in constant expressions");
static_assert(bit_slice_bytes(16) == 128 && bit_total(4, 8) == 4 * 64 + 64 && bit_index(1, 1, 3, 16) == 128 + 64 + 3 && code_index(1, 9, 3, 16) == 1024 + (64 + 3) * 8 + 1,
              "usable in constant expressions");
static_assert(pack8(0x01000001u, 0x00010100u) == 0x69u && !above1(0x01010101u, 0x01010101u) && above1(0u, 0x00020000u) && above1(0x80000000u, 0u), "usable in constant expressions");

// per line of stdin, by its first word:
//   rule vd_u clause off          -> "rule <kind> <0|1> <width>"
//   sizes ns uw                   -> "sizes <slice bytes> <total> <pad> <code pad>"
//   index ns uw                   -> "index" and bit_index of every (slice, turn, lane) in that order
//   pack ns uw, ns * 64 * uw codes in the order [slice][position][lane]
//                                 -> "pack <1 if a code is above 1> " and the bytes of the bit array, padding included
int main() {
    char word[16];
    while (std::scanf("%15s", word) == 1) {
        if (!std::strcmp(word, "rule")) {
            int vd, clause, off;
            if (std::scanf("%d %d %d", &vd, &clause, &off) != 3) return 1;
            const int k = kind(clause, vd);
            std::printf("rule %d %d %d\n", k, bit_codes(k, off != 0) ? 1 : 0, code_width(bit_codes(k, off != 0)));
        } else if (!std::strcmp(word, "sizes")) {
            int ns, uw;
            if (std::scanf("%d %d", &ns, &uw) != 2) return 1;
            std::printf("sizes %d %lld %d %d\n", bit_slice_bytes(uw), (long long)bit_total(ns, uw), BIT_PAD, CODE_PAD);
        } else if (!std::strcmp(word, "index")) {
            int ns, uw;
            if (std::scanf("%d %d", &ns, &uw) != 2) return 1;
            std::printf("index");
            for (int s = 0; s < ns; ++s) for (int t = 0; t < uw / 8; ++t) for (int l = 0; l < 64; ++l) std::printf(" %lld", (long long)bit_index(s, t, l, uw));
            std::printf("\n");
        } else if (!std::strcmp(word, "pack")) {
            int ns, uw;
            if (std::scanf("%d %d", &ns, &uw) != 2) return 1;
            // k_vidx's codes as k_vi_build lays them out, behind them the padding
            std::vector<unsigned char> code((size_t)ns * 64 * uw + CODE_PAD, 0), bits((size_t)bit_total(ns, uw), 0xff);
            for (int s = 0; s < ns; ++s) for (int j = 0; j < uw; ++j) for (int l = 0; l < 64; ++l) {
                int c;
                if (std::scanf("%d", &c) != 1) return 1;
                code[(size_t)code_index(s, j, l, uw)] = (unsigned char)c;
            }
            if (code.size() != 8 * bits.size()) return 4;
            // the device pass of build_xwin: word i of the codes -> byte i
            bool bad = false;
            for (size_t i = 0; i < bits.size(); ++i) {
                unsigned lo, hi;
                std::memcpy(&lo, &code[8 * i], 4); std::memcpy(&hi, &code[8 * i + 4], 4);
                bits[i] = (unsigned char)pack8(lo, hi);
                bad = bad || above1(lo, hi);
            }
            // ... and byte (slice, turn, lane) is where the eight codes of that turn begin
            for (int s = 0; s < ns; ++s) for (int t = 0; t < uw / 8; ++t) for (int l = 0; l < 64; ++l)
                if (8 * bit_index(s, t, l, uw) != code_index(s, 8 * t, l, uw)) return 5;
            std::printf("pack %d", bad ? 1 : 0);
            for (unsigned char b : bits) std::printf(" %d", (int)b);
            std::printf("\n");
        } else return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("vw_fast_bits_check")
    src, out = str(d / "vw_fast_bits_check.cpp"), str(d / "vw_fast_bits_check")
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


def test_the_rule_on_both_sides_of_each_clause(exe):
    """bit codes exactly where the lean kernel runs with scalar dictionaries (kind 2: one or two values) and the switch is not off"""
    TAKEN, WIDTHS_DIFFER = 0, 2
    cases = {
        "one value": ((1, TAKEN, 0), (2, 1, 1)), "two values": ((2, TAKEN, 0), (2, 1, 1)), "three values": ((3, TAKEN, 0), (1, 0, 8)),
        "one value, switched off": ((1, TAKEN, 1), (2, 0, 8)), "two values, switched off": ((2, TAKEN, 1), (2, 0, 8)), "three values, switched off": ((3, TAKEN, 1), (1, 0, 8)),
        "two values on an operator the lean kernel refuses": ((2, WIDTHS_DIFFER, 0), (0, 0, 8)), "... switched off": ((2, WIDTHS_DIFFER, 1), (0, 0, 8)),
    }
    names = sorted(cases)
    for n, w in zip(names, run(exe, ["rule %d %d %d" % cases[n][0] for n in names])):
        assert tuple(int(x) for x in w[1:]) == cases[n][1], (n, w)


@pytest.mark.parametrize("uw", WIDTHS)
@pytest.mark.parametrize("ns", SLICES)
def test_every_slice_turn_and_lane_has_a_byte_of_its_own_inside_the_array(exe, ns, uw):
    sizes, index = run(exe, [f"sizes {ns} {uw}", f"index {ns} {uw}"])
    slice_bytes, total, pad, code_pad = (int(x) for x in sizes[1:])
    assert slice_bytes == 8 * uw == 64 * uw // 8                     # an eighth of the slice's 64 uw bytes of codes
    assert (pad, code_pad) == (64, 512) and total == ns * slice_bytes + pad      # one turn of one slice behind the last, as the 8-bit codes have
    i = np.array(index[1:], np.int64)
    assert len(i) == ns * (uw // 8) * 64 and len(set(i.tolist())) == len(i)
    assert i.min() == 0 and i.max() == ns * slice_bytes - 1 < total              # dense: the codes' bytes and nothing between them
    # slice-major, then turn, then lane: a wave's load of a turn is 64 consecutive bytes
    assert np.array_equal(i, np.arange(len(i)))


@pytest.mark.parametrize("uw", WIDTHS)
@pytest.mark.parametrize("ns", SLICES)
def test_packing_random_codes_equals_packbits_over_the_position_axis(exe, ns, uw):
    rng = np.random.default_rng(1000 * ns + uw)
    code = rng.integers(0, 2, size=(ns, uw, 64), dtype=np.uint8)     # [slice][position][lane]
    out = run(exe, [f"pack {ns} {uw} " + " ".join(map(str, code.ravel().tolist()))])[0]
    assert out[0] == "pack" and out[1] == "0"
    got = np.array(out[2:], np.uint8)
    want = np.packbits(code, axis=1, bitorder="little")              # [slice][turn][lane]: bit u of a byte = position 8 turn + u
    assert want.shape == (ns, uw // 8, 64)
    assert np.array_equal(got[:want.size], want.ravel()) and len(got) == want.size + 64 and not got[want.size:].any()
    assert want.any() and (want != 0xff).any()


def test_a_code_above_one_is_seen_wherever_it_stands(exe):
    for pos, value in ((0, 2), (7, 255), (64 * 8 + 5, 128), (2 * 64 * 8 - 1, 3)):
        code = np.zeros((2, 8, 64), np.uint8)
        code.ravel()[pos] = value
        out = run(exe, ["pack 2 8 " + " ".join(map(str, code.ravel().tolist()))])[0]
        assert out[1] == "1", (pos, value)
