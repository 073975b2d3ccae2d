// xwin_stage.h -- how k_vidxw's workgroup brings its windows of x into LDS window by window: the rule that picks this staging over
// the flat one, and the map (lane, trip) -> (LDS slot, column - r0).  Plain C++17, no HIP, every function constexpr: build_xwin fills
// the kernel's trips through it, k_vidxw forms its addresses through it, and a host compiler can test it
// (tests/test_xwin_stage_header.py).
//
// A workgroup of R lanes stages window c -- `size` doubles, the columns r0 + omin + i at the LDS slots base + i -- in trips of R
// consecutive elements: lane l of trip (c, k) holds element i = k R + l where i < size.  A trip is three scalars, so a staged element
// costs its lane one add for the load's offset and one compare/select for its slot; which window it belongs to is never asked of a lane.
//
// The loads are buffer loads through a descriptor of x with num_records = 8 ncols: the hardware's range check compares the byte
// offset the LANE supplies (a raw buffer, stride 0: the vector offset plus the instruction's immediate; the scalar offset operand is
// not part of that sum, so it stays 0 and r0, the window and the lane all go into the vector offset) with num_records as an UNSIGNED
// 32-bit number and returns zero beyond it.  A column right of x lands in [8 ncols, 2^31); a column left of x has a negative offset,
// which as an unsigned number lands in [2^31, 2^32 - 8]; per_window() refuses operators whose columns would leave those two ranges.
#pragma once
#include <cstdint>

namespace xwstage {

constexpr int MAX_WIN = 4;                        // windows this staging takes
constexpr int MAX_TRIPS = 6;                      // trips they can need: nwin + sum over the windows of ceil((size - R) / R), with S <= 4 R
constexpr int64_t DESC_COLS = int64_t(1) << 28;   // columns below it have byte offsets below 2^31, and so has num_records of an x shorter than it
constexpr unsigned OFF_NONE = 0x80000000u;        // the offset of a trip that loads nothing: beyond every descriptor, for every lane (8 R <= 8 KiB more)

struct Trip {
    int lds;          // LDS slot of lane 0
    int col;          // its column - r0
    int cnt;          // lanes that hold an element of the window (the others write the spare slot); 0: an unused trip
};

// The rule.  nwin windows of S doubles in all for workgroups of R rows; x has ncols elements, the operator nrows rows; the windows
// begin at omin_first (relative to r0) and end at omax_last + R.  Every lane of a trip loads, also past its window's size, so the
// columns asked for lie in [omin_first, r0_last + omax_last + 2 R).
constexpr bool per_window(int nwin, int64_t S, int R, int64_t ncols, int64_t nrows, int64_t omin_first, int64_t omax_last) {
    return nwin >= 1 && nwin <= MAX_WIN && S <= 4 * int64_t(R) && ncols < DESC_COLS && omin_first >= -DESC_COLS &&
           nrows + omax_last + 2 * int64_t(R) <= DESC_COLS;
}

// The trips of nwin windows (LDS base, omin, size per window), in window order -> their count; out[] holds MAX_TRIPS, the unused
// ones with cnt = 0.  Returns 0 where they do not fit (per_window() said no).
constexpr int trips(int nwin, const int *base, const int *omin, const int *size, int R, Trip *out) {
    for (int t = 0; t < MAX_TRIPS; ++t) out[t] = Trip{0, 0, 0};
    int n = 0;
    for (int c = 0; c < nwin; ++c)
        for (int i0 = 0; i0 < size[c]; i0 += R) {
            if (n == MAX_TRIPS) return 0;
            out[n++] = Trip{base[c] + i0, omin[c] + i0, size[c] - i0 < R ? size[c] - i0 : R};
        }
    return n;
}

// The map.  S: the spare slot behind the windows.
constexpr int slot(const Trip &t, int lane, int S) { return lane < t.cnt ? t.lds + lane : S; }
constexpr int column(const Trip &t, int lane) { return t.col + lane; }                 // minus r0
// the byte offset the lane hands the buffer load, in unsigned arithmetic: it wraps where the column is negative
constexpr unsigned byte_offset(int r0, const Trip &t, int lane) {
    return 8u * ((t.cnt > 0 ? (unsigned)(r0 + t.col) : OFF_NONE / 8u) + (unsigned)lane);      // (the choice is a scalar's: one add and shift per lane)
}

}
