// vw_fast.h -- the common path of k_vidxw as a kernel of its own (k_vidxw_fast): the rule that says which operator x workgroup size and
// which launch take it, its one argument (VwFast), and how build_xwin fills the part of that argument which is a function of the plan
// alone.  Plain C++17, no HIP, every function constexpr: build_xwin and launch_part decide through it, the kernels read the row loop's
// body through it, and a host compiler can test it (tests/test_vw_fast_header.py).
//
// k_vidxw serves every geometry the x-window mode accepts, and every wave of every launch works the geometry out again in scalar
// instructions: log2 of R from blockDim, the dictionaries of the workgroup, the LDS carve-up, per trip its offset and slot base, and
// the branches that pick the common path.  On the operators the mode is kept for (one slice width, one dictionary length, at most four
// trips, a table of at most R chunks) all of that is known once build_xwin has run.  The lean kernel takes it as arguments in the form
// it consumes, with R, the epilogue and the dictionary treatment as template parameters.
#pragma once
#include <cstdint>
#include "xwin_stage.h"
#include "xwin_head.h"

namespace vwfast {

constexpr int TRIPS = 4;                          // trips the lean kernel issues, used or not (the 7-point levels: 1 + 2 + 1)
using sk::NXCD;
using sk::VI_MAX;                                 // values of a dictionary, one per 256 rows
constexpr int MASK_SLOTS = 8;                     // slots of a row held as lane masks (vw_masks.h: MAXSLOT)

// ---- the rule ----
// which clause refuses an operator x R, in the order the rule is written; TAKEN: eligible
enum Clause : int { TAKEN = 0, ROWS, WIDTHS, DICT_LENGTHS, TRIP_COUNT, TABLE_CHUNKS, SWITCHED_OFF };
// R: rows per workgroup; uw: the slices' common width (0: they differ); vd_u: the dictionaries' common length (0: they differ);
// ntrip: trips of the window-by-window staging (0: flat staging); n8: 16-byte chunks of the pattern table
constexpr int refused(int R, int uw, int vd_u, int ntrip, int n8) {
    return !(R == 256 || R == 512) ? ROWS : uw == 0 ? WIDTHS : vd_u == 0 ? DICT_LENGTHS : !(ntrip >= 1 && ntrip <= TRIPS) ? TRIP_COUNT : n8 > R ? TABLE_CHUNKS : TAKEN;
}
constexpr const char *clause_text(int c) {
    return c == ROWS ? "workgroups of neither 256 nor 512 rows" : c == WIDTHS ? "slices of differing widths" : c == DICT_LENGTHS ? "dictionaries of differing lengths"
         : c == TRIP_COUNT ? "not staged window by window in one to four trips" : c == TABLE_CHUNKS ? "a pattern table of more 16-byte chunks than rows per workgroup"
         : c == SWITCHED_OFF ? "SAENA_VIDXW_FAST=0" : "taken";
}
// dictionaries of at most two values stay in scalar registers: a position's value is a select by bit 0 of its code
constexpr bool scalar_dict(int vd_u) { return vd_u == 1 || vd_u == 2; }
// what the operator runs: 0 the general kernel, 1 the lean kernel with its dictionaries in LDS, 2 with scalar dictionaries
constexpr int kind(int clause, int vd_u) { return clause != TAKEN ? 0 : scalar_dict(vd_u) ? 2 : 1; }
// a launch of an eligible operator takes the lean kernel without a halo and with the plain product (0), the residual (1) or the
// Jacobi sweep (2): the epilogues k_vidxw treats with operands fetched up front (kernels.hip.h: sk::Epi)
constexpr bool launch_takes(int kind_, bool halo, int epi) { return kind_ != 0 && !halo && epi >= 0 && epi <= 2; }

// ---- bit codes: the codes of an operator with scalar dictionaries are 0 or 1 and the kernel reads bit 0 alone, so the lean kernel
// streams ONE BIT per entry: byte [slice][turn j / 8][lane] holds, as bit u, bit 0 of the code of position j + u.  A lane's turn is one
// byte where k_vidx's codes are eight; every entry still carries a code of its own.  build_xwin packs the array from k_vidx's codes
// (which k_vidx, k_vidxw and every halo launch go on reading); both arrays end in one turn of one slice of zeros.
constexpr int CODE_PAD = 512;                     // bytes k_vidx's codes are padded by: a turn of a slice (64 lanes x 8 positions)
constexpr int BIT_PAD = CODE_PAD / 8;             // ... and the bit codes: the same turn
// taken exactly where the dictionaries stay in scalar registers (kind 2), unless SAENA_VIDXW_BITS=0 (bits_off)
constexpr bool bit_codes(int kind_, bool bits_off) { return kind_ == 2 && !bits_off; }
// bits per entry of the code stream a launch reads
constexpr int code_width(bool bits) { return bits ? 1 : 8; }
// bytes of a slice of uw positions (a multiple of 8): an eighth of its 64 uw bytes of codes
constexpr int bit_slice_bytes(int uw) { return 8 * uw; }
constexpr int64_t bit_total(int nslices, int uw) { return (int64_t)nslices * bit_slice_bytes(uw) + BIT_PAD; }
// the byte of (slice, turn, lane), turn < uw / 8, lane < 64 ...
constexpr int64_t bit_index(int slice, int turn, int lane, int uw) { return (int64_t)slice * bit_slice_bytes(uw) + (int64_t)turn * 64 + lane; }
// ... and the byte of k_vidx's codes that holds position j of that lane (k_vi_build's layout: a lane's turn is eight bytes side by
// side).  The eight codes of bit_index(s, t, l, uw) begin at 8 bit_index(s, t, l, uw): the pack is one pass over 8-byte words
constexpr int64_t code_index(int slice, int j, int lane, int uw) { return (int64_t)slice * 64 * uw + ((int64_t)(j >> 3) * 64 + lane) * 8 + (j & 7); }
// a turn's eight codes (c[0]: position j, as the low byte of the low word) -> its byte; above1: a code that is neither 0 nor 1
constexpr unsigned pack8(unsigned lo, unsigned hi) {
    unsigned b = 0;
    for (int u = 0; u < 4; ++u) b |= ((lo >> (8 * u)) & 1u) << u | ((hi >> (8 * u)) & 1u) << (4 + u);
    return b;
}
constexpr bool above1(unsigned lo, unsigned hi) { return ((lo | hi) & 0xfefefefeu) != 0; }

// ---- the row loop's body, for both kernels: positions j ... j + 7 of a row, lmin / lmax the shortest and the longest pattern ----
// the positions at or beyond the longest pattern are not computed (never fewer than four: the lengths 1 ... 3 share the body of 4),
// the first four take no select where every row holds them -> 2 (n - 4) + free4, n = 4 ... 8
constexpr int body(int lmin, int lmax, int j) {
    const int n = lmax - j;
    return 2 * ((n < 4 ? 4 : n > 8 ? 8 : n) - 4) + (j + 4 <= lmin ? 1 : 0);
}
constexpr int body_positions(int body_) { return 4 + (body_ >> 1); }
constexpr bool body_free4(int body_) { return (body_ & 1) != 0; }

// ---- the XCD remap (kernels.hip.h: xcd_remap) with its quotient rq = n / NXCD and remainder rr = n % NXCD taken from the plan: the
// launch's block bx -> the workgroup it computes, so that the blocks that share an XCD take consecutive workgroups ----
constexpr int remap(int bx, int rq, int rr) {
    const int xc = (int)((unsigned)bx % (unsigned)NXCD), xk = (int)((unsigned)bx / (unsigned)NXCD);      // (bx >= 0: an and, a shift)
    return xk < rq + (xc < rr ? 1 : 0) ? xc * rq + (xc < rr ? xc : rr) + xk : bx;
}

// ---- the argument ----
struct Trip {
    int lds8;         // LDS byte offset of lane 0's slot
    int col;          // lane 0's column - r0; an unused trip: OFF_NONE / 8 -- byte offsets from 2^31 on, which no descriptor reaches, for
                      // every row below 2^28 (whatever such a trip loads goes to the spare slot: cnt = 0)
    int cnt;          // lanes that hold an element of the window (the others write the spare slot); 0: an unused trip
};
// Everything k_vidxw_fast reads and nothing else, in the order it is needed.  build_xwin fills the operator's part once (plan()
// below, and the operator's arrays); launch_part copies it and sets x, y, rhs, inv_diag, u, c0, nt_from, st_plain, nrows.
struct VwFast {
    // the prologue's loads
    const unsigned char  *vcode;      // k_vidx's codes, or the bit codes (launch_part sets this and cbytes by the format)
    const unsigned short *dst;        // pattern ids
    const void           *ptab;       // the table as 16-bit words (build_xwin's), read in 16-byte chunks
    const double         *vdict;      // the dictionaries back to back
    const unsigned long long *masks;  // the rows as lane masks, a record per slice (vw_masks.h), or null: rows through the table
    const double         *x;
    const double         *rhs, *inv_diag, *u;
    int nrows, nblk;                  // rows; slices of 64 rows
    int rq, rr;                       // the XCD remap: workgroups / NXCD, workgroups % NXCD
    int cbytes;                       // bytes of a slice's codes: 64 uw (bit codes: 8 uw)
    int n8;                           // 16-byte chunks of the table (1 ... R)
    int vd_u, ngd;                    // values per dictionary; dictionaries of the operator
    unsigned xbytes;                  // 8 ncols: the buffer descriptor's num_records
    int nt_from;                      // first slice read with non-temporal loads
    Trip trip[TRIPS];
    // behind the loads: the LDS carve-up in bytes
    int S8;                           // the spare slot behind the windows
    int dict_off, tab_off, pos_off;   // dictionaries (LDS dictionaries only), table, the table's positions (behind the patterns' lengths)
    int pw2;                          // bytes of a pattern's positions: 2 pt_w
    // the row loop and the store
    int w8;                           // positions of a slice (a multiple of 8)
    int lmin, lmax, body0;            // the shortest and the longest pattern; body(lmin, lmax, 0)
    int slot_off[MASK_SLOTS];         // mask rows: the LDS byte offset of slot u for the workgroup's first row (vw_masks.h: rule)
    int st_plain;
    double *y;
    double  c0;
};

// The operator's part of VwFast but its four arrays, and the LDS bytes a workgroup needs -> those bytes.
// R, nslices: rows per workgroup, slices of 64 rows; S: doubles of x in LDS; lp, words: 16-bit words of the patterns' lengths and of
// the whole table; wp: positions per pattern; uw, vd_u, lmin, lmax: VwHead's; t: xwin_stage.h's trips (at least TRIPS of them);
// sd: scalar dictionaries.  The layout is k_vidxw's -- [windows, spare slot, rounded to 16 B][R / 256 dictionaries][table] -- without
// the dictionaries where they stay in scalar registers.
constexpr int plan(VwFast &f, int R, int nslices, int ncols, int S, int lp, int words, int wp, int uw, int vd_u, int lmin, int lmax, const xwstage::Trip *t, bool sd) {
    const int spb = R / 64, nwg = (nslices + spb - 1) / spb;
    f.nblk = nslices; f.rq = nwg / NXCD; f.rr = nwg % NXCD;
    f.cbytes = 64 * uw; f.n8 = words >> 3; f.vd_u = vd_u; f.ngd = (nslices + 3) >> 2;
    f.xbytes = 8u * (unsigned)ncols;
    for (int u = 0; u < TRIPS; ++u) f.trip[u] = Trip{8 * t[u].lds, t[u].cnt > 0 ? t[u].col : (int)(xwstage::OFF_NONE / 8u), t[u].cnt};
    f.S8 = 8 * S;
    f.dict_off = 8 * ((S + 2) & ~1);
    f.tab_off = f.dict_off + (sd ? 0 : (R / 256) * VI_MAX * 8);
    f.pos_off = f.tab_off + 2 * lp;
    f.pw2 = 2 * wp;
    f.w8 = uw; f.lmin = lmin; f.lmax = lmax; f.body0 = body(lmin, lmax, 0);
    return f.tab_off + 2 * words;
}

}
