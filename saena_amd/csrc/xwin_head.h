// xwin_head.h -- what the x-in-LDS kernels (k_sellpx, k_vidxw, k_vidxw_fast), the plans that feed them (xwin_plan.h, vw_fast.h) and
// the runtime agree on: the limits of the two forms, each defined here and nowhere else, and the head of k_vidxw's tables that travels
// by value.  Plain C++17, no HIP: kernels.hip.h reads these as sk:: names, and a host compiler sees the struct the plan fills.
#pragma once
#include "xwin_stage.h"

namespace sk {

constexpr int NXCD = 8;                        // XCDs a launch's workgroups are dealt to in turn (kernels.hip.h: xcd_remap, vw_fast.h: remap)
constexpr int VI_MAX = 256;                    // values of a dictionary of the value-indexed form, one per 256 rows
constexpr int VW_MAX_LDS = 64 * 1024;          // k_vidxw: windows + dictionaries + table: at least two workgroups per CU
constexpr int SPX_ROWS  = 512;                 // k_sellpx: rows per workgroup: 8 slices of 64 (256 rows, 3-4 workgroups per CU: 127.5 against 119.7 us of k_sellp<WIDE>)
constexpr int SPX_MAXWIN = 16;                 // windows either form takes
constexpr int SPX_LDS_BYTES = 80 * 1024;       // k_sellpx: windows + table: two workgroups per CU

// the head of k_vidxw's window table and what else the prologue would fetch from memory before it can form an address: by value,
// k_vidxw's second parameter (build_xwin fills it through xwin_plan.h)
struct VwHead {
    int nwin, S;          // windows; doubles of x in LDS
    int win[8];           // (LDS base, omin - base) of the first four windows (unused ones: base INT32_MAX)
    int lp, tn;           // 16-bit words of the table: the patterns' lengths, all of it (multiples of 8)
    int vd_u;             // every dictionary of the operator holds this many values, or 0: they differ, read a.vdptr
    int lmin, lmax;       // the shortest and the longest pattern: positions below lmin are real in every row, none at or beyond lmax in any
    int ntrip;            // the windows are staged one by one in this many trips (xwin_stage.h), or 0: the flat staging
    xwstage::Trip trip[xwstage::MAX_TRIPS];      // ... the sizes of the first four windows next to their bases, trip by trip (unused: cnt 0)
};

}
