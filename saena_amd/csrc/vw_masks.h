// vw_masks.h -- the rows of k_vidxw_fast as LANE MASKS: the rule that says which operator x workgroup size takes them, the record a
// slice of 64 rows becomes, and the host-side pack of one slice.  Plain C++17, no HIP, every function constexpr: plan_vidxw decides
// through it, build_xwin and k_vi_pack_masks lay the records out through it, k_vidxw_fast<MASKS> reads them through it, and a host
// compiler can test and sanitize it (tests/test_vw_masks_header.py, tools/sanitize_vw_masks.cpp).
//
// On a stencil-like operator every row pattern is an ordered subset of ONE pattern's positions -- the SLOTS.  The LDS byte offset of
// slot u relative to a lane's own element is then the same for every row of every workgroup: a plan-time scalar (VwFast::slot_off).
// What differs from lane to lane is which slots a row holds and which of the two dictionary values a slot takes: two bits per
// (row, slot), stored per slice as 64-bit lane masks -- the operand a select takes from a scalar register pair.  A wave then needs no
// pattern id, no code byte, no table in LDS and no LDS round trip in front of its x reads.
#pragma once
#include <cstdint>
#include "vw_fast.h"

namespace vwmasks {

constexpr int MAXSLOT = vwfast::MASK_SLOTS;       // slots of a record: one turn of eight positions
constexpr int NO_SLOT = 0xff;                     // a position of the pattern -> slot table that maps to no slot

// ---- the rule ----
// which clause refuses an operator x R, in the order the rule is written; TAKEN: eligible
enum Clause : int { TAKEN = 0, NOT_SCALAR, TURNS, REPEATED, NOT_SUBSEQUENCE, SWITCHED_OFF };
constexpr const char *clause_text(int c) {
    return c == NOT_SCALAR ? "the dictionaries are not in scalar registers" : c == TURNS ? "a pattern of more than eight positions"
         : c == REPEATED ? "the longest pattern repeats a position" : c == NOT_SUBSEQUENCE ? "a pattern is no ordered subset of the longest pattern"
         : c == SWITCHED_OFF ? "SAENA_VIDXW_MASKS=0" : "taken";
}
// kind: vwfast::kind of the plan; len: the npat patterns' lengths; pos: per pattern wp positions (any unit, LDS byte offsets in
// build_xwin's table), of which the first len count; off: SAENA_VIDXW_MASKS=0.
// -> the clause.  Where the clauses before the switch hold: nslot = the longest pattern's length, slot[u] = position of slot u (the
// FIRST longest pattern's, in its order; 0 from nslot on), pslot[i * MAXSLOT + j] = the slot of position j of pattern i (NO_SLOT from
// its length on).  slot: MAXSLOT ints, pslot: npat * MAXSLOT bytes.
constexpr int rule(int kind, const unsigned short *len, const unsigned short *pos, int npat, int wp, bool off, int *nslot, int *slot, unsigned char *pslot) {
    *nslot = 0;
    for (int u = 0; u < MAXSLOT; ++u) slot[u] = 0;
    if (kind != 2) return NOT_SCALAR;
    int longest = 0;
    for (int i = 0; i < npat; ++i) if (len[i] > len[longest]) longest = i;
    const int n = npat > 0 ? (int)len[longest] : 0;
    if (n > MAXSLOT || n > wp) return TURNS;
    for (int u = 0; u < n; ++u) {
        for (int t = 0; t < u; ++t) if (pos[(int64_t)longest * wp + u] == pos[(int64_t)longest * wp + t]) return REPEATED;
        slot[u] = pos[(int64_t)longest * wp + u];
    }
    *nslot = n;
    for (int i = 0; i < npat; ++i) {
        int u = 0;                                                // the slots below u are used up: strictly increasing
        for (int j = 0; j < MAXSLOT; ++j) {
            if (j >= (int)len[i]) { pslot[(int64_t)i * MAXSLOT + j] = (unsigned char)NO_SLOT; continue; }
            while (u < n && slot[u] != (int)pos[(int64_t)i * wp + j]) ++u;
            if (u == n) return NOT_SUBSEQUENCE;
            pslot[(int64_t)i * MAXSLOT + j] = (unsigned char)u++;
        }
    }
    return off ? SWITCHED_OFF : TAKEN;
}

// ---- the record: per slice of 64 rows 16 words of 64 bits -- MAXSLOT presence masks (bit l of mask u: lane l's row holds slot u),
// then MAXSLOT value masks (bit l of mask u: that slot takes dictionary value 1).  Masks of slots the operator does not have and the
// bits of lanes without a row are zero.  A spare wave reads slice 0's record: the array needs no padding.
constexpr int REC_WORDS = 2 * MAXSLOT, REC_BYTES = 8 * REC_WORDS;
constexpr int64_t total_words(int nslices) { return (int64_t)nslices * REC_WORDS; }
constexpr int64_t presence_index(int slice, int u) { return (int64_t)slice * REC_WORDS + u; }
constexpr int64_t value_index(int slice, int u) { return (int64_t)slice * REC_WORDS + MAXSLOT + u; }

// ---- the pack ----
constexpr int CODE_ABOVE_1 = 1, UNMAPPED = 2;     // what keeps the table rows: a code that is neither 0 nor 1; a position without a slot
// One lane's part of its slice's record: len positions, slot of position j = ps[j], code of position j = code(j).  -> its presence
// bits (bit u: slot u) | its value bits << 8 | flags << 16.  The device pack (k_vi_pack_masks) and pack_slice share it.
template <class Code>
constexpr unsigned lane_bits(int len, const unsigned char *ps, Code code) {
    unsigned pb = 0, vb = 0, flags = 0;
    for (int j = 0; j < MAXSLOT; ++j) {
        if (j >= len) continue;
        const unsigned u = ps[j], c = code(j);
        if (c > 1u) flags |= CODE_ABOVE_1;
        if (u >= (unsigned)MAXSLOT) { flags |= UNMAPPED; continue; }
        pb |= 1u << u;
        vb |= (c & 1u) << u;
    }
    return pb | vb << 8 | flags << 16;
}
// The record of slice `slice` of an operator of nrows rows on the host.  pid: the rows' pattern ids; len, pslot: the rule's; code:
// k_vidx's codes (vwfast::code_index) at uw positions per slice; rec: REC_WORDS words.  -> the flags of its rows, or-ed
constexpr int pack_slice(int slice, int nrows, const unsigned short *pid, const unsigned short *len, const unsigned char *pslot, const unsigned char *code, int uw, uint64_t *rec) {
    for (int w = 0; w < REC_WORDS; ++w) rec[w] = 0;
    int flags = 0;
    for (int l = 0; l < 64; ++l) {
        const int64_t r = (int64_t)slice * 64 + l;
        if (r >= nrows) break;
        const int p = pid[r];
        const int n = len[p] < MAXSLOT ? (int)len[p] : MAXSLOT;
        const unsigned b = lane_bits(n, pslot + (int64_t)p * MAXSLOT, [&](int j) { return (unsigned)code[vwfast::code_index(slice, j, l, uw)]; });
        for (int u = 0; u < MAXSLOT; ++u) {
            rec[u] |= (uint64_t)((b >> u) & 1u) << l;
            rec[MAXSLOT + u] |= (uint64_t)((b >> (8 + u)) & 1u) << l;
        }
        flags |= (int)(b >> 16);
    }
    return flags;
}

}
