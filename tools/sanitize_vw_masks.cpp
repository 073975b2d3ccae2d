// sanitize_vw_masks.cpp -- saena_amd/csrc/vw_masks.h (the rule of the mask rows of k_vidxw_fast, the record of a slice and the host
// pack) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program on the host:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       tools/sanitize_vw_masks.cpp -o sanitize_vw_masks && ./sanitize_vw_masks
// The rule's edges -- no pattern, an empty table row, eight and nine positions, a table exactly eight positions wide, a repeated
// position, a pattern that skips back -- run on vectors sized to the element, so that a read past a pattern's positions or a write
// past the pattern -> slot table is the sanitizer's to report (another exit status); the pack runs on a partial last slice with the
// pattern ids and codes sized to the element as well.  A wrong verdict or a wrong word fails a check below.
#include "../saena_amd/csrc/vw_masks.h"

#include <cstdio>
#include <vector>

using namespace vwmasks;
using Patterns = std::vector<std::vector<int>>;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Ruled { int clause, nslot, slot[MAXSLOT]; std::vector<unsigned char> pslot; std::vector<unsigned short> len, pos; };
// the table as plan_vidxw lays it out: wp positions per pattern, the tail repeating the last one
static Ruled ruled(const Patterns &pats, int wp, int kind = 2, bool off = false) {
    Ruled r;
    const int npat = (int)pats.size();
    r.len.resize((size_t)npat); r.pos.assign((size_t)npat * wp, 0); r.pslot.assign((size_t)npat * MAXSLOT, 0x77);
    for (int i = 0; i < npat; ++i) {
        r.len[(size_t)i] = (unsigned short)pats[(size_t)i].size();
        unsigned short last = 0;
        for (int j = 0; j < wp; ++j) {
            if (j < (int)pats[(size_t)i].size()) last = (unsigned short)pats[(size_t)i][(size_t)j];
            r.pos[(size_t)i * wp + j] = last;
        }
    }
    r.clause = rule(kind, r.len.data(), r.pos.data(), npat, wp, off, &r.nslot, r.slot, r.pslot.data());
    return r;
}

int main() {
    const std::vector<int> seven = {8, 800, 1600, 1608, 1616, 2400, 3200}, eight = {0, 8, 16, 24, 32, 40, 48, 65528}, nine = {0, 8, 16, 24, 32, 40, 48, 56, 64};
    // ---- the rule ----
    CHECK(ruled({}, 8).clause == TAKEN && ruled({}, 8).nslot == 0);
    CHECK(ruled({{}}, 8).clause == TAKEN);
    CHECK(ruled({seven, {8, 1608}, {}}, 8).clause == TAKEN);
    CHECK(ruled({eight, {65528}}, 8).clause == TAKEN && ruled({eight}, 8).nslot == 8 && ruled({eight}, 8).slot[7] == 65528);
    CHECK(ruled({nine}, 16).clause == TURNS && ruled({{8}, nine}, 16).clause == TURNS);
    CHECK(ruled({seven}, 8, 1).clause == NOT_SCALAR && ruled({seven}, 8, 0).clause == NOT_SCALAR);
    CHECK(ruled({{8, 16, 8}}, 8).clause == REPEATED);
    CHECK(ruled({seven, {1608, 8}}, 8).clause == NOT_SUBSEQUENCE && ruled({seven, {8, 8}}, 8).clause == NOT_SUBSEQUENCE && ruled({seven, {3208}}, 8).clause == NOT_SUBSEQUENCE);
    CHECK(ruled({{800, 1600}, {8, 800}}, 8).clause == NOT_SUBSEQUENCE);
    CHECK(ruled({seven}, 8, 2, true).clause == SWITCHED_OFF && ruled({nine}, 16, 2, true).clause == TURNS);
    {
        const Ruled r = ruled({{8, 1608}, seven}, 8);
        CHECK(r.clause == TAKEN && r.nslot == 7 && r.pslot[0] == 0 && r.pslot[1] == 3 && r.pslot[2] == NO_SLOT && r.pslot[MAXSLOT + 6] == 6 && r.pslot[MAXSLOT + 7] == NO_SLOT);
    }
    // ---- the record and the pack: three slices, the last of 5 rows ----
    static_assert(REC_BYTES == 128 && presence_index(2, 7) == 39 && value_index(2, 7) == 47, "the record");
    const Ruled r = ruled({seven, {8, 1608, 3200}, {}}, 8);
    const int ns = 3, nrows = 2 * 64 + 5, uw = 8;
    std::vector<unsigned short> pid((size_t)nrows);
    std::vector<unsigned char> code((size_t)ns * 64 * uw, 0);
    for (int i = 0; i < nrows; ++i) pid[(size_t)i] = (unsigned short)(i % 3);
    for (int s = 0; s < ns; ++s) for (int l = 0; l < 64; ++l) for (int j = 0; j < uw; ++j) code[(size_t)vwfast::code_index(s, j, l, uw)] = (unsigned char)((s + l + j) & 1);
    std::vector<uint64_t> rec((size_t)total_words(ns), ~0ull);
    for (int s = 0; s < ns; ++s) CHECK(pack_slice(s, nrows, pid.data(), r.len.data(), r.pslot.data(), code.data(), uw, &rec[(size_t)presence_index(s, 0)]) == 0);
    for (int s = 0; s < ns; ++s) for (int u = 0; u < MAXSLOT; ++u) {
        uint64_t pm = 0, vm = 0;
        for (int l = 0; l < 64 && s * 64 + l < nrows; ++l) {
            const int p = (s * 64 + l) % 3;
            for (int j = 0; j < (int)r.len[(size_t)p]; ++j) if (r.pslot[(size_t)p * MAXSLOT + j] == u) { pm |= 1ull << l; vm |= (uint64_t)((s + l + j) & 1) << l; }
        }
        CHECK(rec[(size_t)presence_index(s, u)] == pm && rec[(size_t)value_index(s, u)] == vm);
    }
    CHECK(rec[(size_t)presence_index(2, 0)] >> 5 == 0 && rec[(size_t)presence_index(0, 7)] == 0);
    // a code above 1 in the last row's last position (beyond a pattern's length a code is not looked at); a position without a slot
    code[(size_t)vwfast::code_index(2, 6, 3, uw)] = 2;           // (row 131 is empty)
    CHECK(pack_slice(2, nrows, pid.data(), r.len.data(), r.pslot.data(), code.data(), uw, &rec[(size_t)presence_index(2, 0)]) == 0);
    code[(size_t)vwfast::code_index(2, 6, 4, uw)] = 2;           // (row 132 follows the seven-slot pattern)
    CHECK(pack_slice(2, nrows, pid.data(), r.len.data(), r.pslot.data(), code.data(), uw, &rec[(size_t)presence_index(2, 0)]) == CODE_ABOVE_1);
    std::vector<unsigned char> bad = r.pslot;
    bad[MAXSLOT + 2] = (unsigned char)NO_SLOT;
    CHECK(pack_slice(0, nrows, pid.data(), r.len.data(), bad.data(), code.data(), uw, &rec[0]) == UNMAPPED);
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("vw_masks.h: the rule's edges and the pack ran clean");
    return 0;
}
