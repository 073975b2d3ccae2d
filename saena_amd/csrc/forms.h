// forms.h -- the forms of the local SpMV, named once.  Plain C++17, no HIP: sgpu_runtime.hip builds, launches, frees and ranks
// the forms through it, and a host compiler can test it (tests/test_forms_header.py).
//
//   Form, FORM_NAMES             the variant numbers of include/saena_gpu.h (ABI: sgpu_op_set_variant, the plan cache and the
//                                tests use the numbers) and the kernel each one launches
//   tile_plan ... one_candidate  what the runtime asks about a form instead of listing numbers
//   PartGroup, plan_keeps        the storage groups of a part and which of them a settled plan retains
//   plan_line_valid              what a line of the plan cache may say
//   Candidate, choose_plan       what the autotune times, and its decision as a function of the times alone
#pragma once
#include <algorithm>
#include <map>
#include <tuple>

namespace forms {

enum Form : int {
    F_STREAM16 = 0,   // k_csr_stream, 16 KiB tiles
    F_STREAM32 = 1,   // k_csr_stream, 32 KiB tiles
    F_VECTOR = 2,     // k_csr_vector
    F_CC16_16 = 3,    // k_csr_cc16: 16-bit compressed columns, 16 KiB tiles
    F_CC16_32 = 4,    // ... 32 KiB tiles
    F_DENSE = 5,      // k_dense_rows
    F_WAVE = 6,       // k_csr_wave
    F_CM16 = 7,       // k_csr_cm: column order inside a block, on the compressed columns of the 16 KiB plan
    F_CM32 = 8,       // ... of the 32 KiB plan
    F_SELL = 9,       // k_sell: sliced ELLPACK
    F_XLDS = 10,      // k_csr_xlds: x in LDS, nnz-balanced row chunks
    F_SELLP = 11,     // k_sellp: sliced-ELLPACK values + row patterns
    F_SELLX = 12,     // k_sellx: sliced ELLPACK inside the x-in-LDS chunks
    F_ROWT = 13,      // k_rowt: row templates (opt-in)
    F_SELLP2 = 14,    // k_sellp2: row patterns, a lane per two rows
    F_SELLPX = 15,    // k_sellpx: row patterns, x in LDS windows
    F_XLDSR = 16,     // k_csr_xldsr: x in LDS, four rows per group step
    F_VIDX = 17,      // k_vidx: row patterns + 8-bit value codes (k_vidxw: its x-window launch mode)
    F_COUNT
};

// base names (sgpu_op_get_variant decorates them from the part's flags: <wide>, <rowbase>, <sorted>, the slot/offset split)
constexpr const char *FORM_NAMES[] = {"k_csr_stream<16KiB>", "k_csr_stream<32KiB>", "k_csr_vector", "k_csr_cc16<16KiB>", "k_csr_cc16<32KiB>", "k_dense_rows", "k_csr_wave", "k_csr_cm<16KiB>", "k_csr_cm<32KiB>", "k_sell", "k_csr_xlds", "k_sellp", "k_sellx", "k_rowt", "k_sellp2", "k_sellpx", "k_csr_xldsr", "k_vidx"};
static_assert(sizeof FORM_NAMES / sizeof FORM_NAMES[0] == F_COUNT, "one name per form");

// the row-block plan a tile form runs on: 0 (16 KiB tiles), 1 (32 KiB), -1 for a form without tiles
constexpr int tile_plan(int f) {
    return f == F_STREAM16 || f == F_CC16_16 || f == F_CM16 ? 0 : f == F_STREAM32 || f == F_CC16_32 || f == F_CM32 ? 1 : -1;
}
constexpr bool is_dense(int f) { return f == F_DENSE; }
constexpr bool is_cc16(int f) { return f == F_CC16_16 || f == F_CC16_32; }
constexpr bool is_column_major(int f) { return f == F_CM16 || f == F_CM32; }
// the forms over the row-pattern table of build_sellp
constexpr bool is_row_pattern(int f) { return f == F_SELLP || f == F_SELLP2 || f == F_SELLPX || f == F_VIDX; }
// the forms over the x-in-LDS chunk plan of build_xlds
constexpr bool is_xlds_chunk(int f) { return f == F_XLDS || f == F_SELLX || f == F_XLDSR; }
// does the form add a row's products one after the other in column order (the reference's sum, whatever else is tuned)?
constexpr bool sequential_sum(int f, int lanes) {
    return f == F_SELL || f == F_SELLP || f == F_ROWT || f == F_SELLP2 || f == F_SELLPX || f == F_VIDX ||
           (lanes == 1 && tile_plan(f) >= 0);
}
// one autotune candidate whatever the lanes setting: a lane per row (piece), or a wave per dense row
constexpr bool one_candidate(int f) {
    return f == F_SELL || f == F_SELLP || f == F_SELLX || f == F_ROWT || f == F_SELLP2 || f == F_SELLPX || f == F_VIDX || is_dense(f);
}
// the x-window mode of F_VIDX: workgroups of 256 << k rows, k = 0, 1, 2 (-1: no such size)
constexpr int xwin_slot(int rows) { return rows == 256 ? 0 : rows == 512 ? 1 : rows == 1024 ? 2 : -1; }

// The storage groups of a part in the order of sgpu_debug_op_storage's bits, and which of them the plan that settles on form
// `f` keeps (finish_plan resets the others).  vw_rows: the x-window workgroup size in use, its tables alone stay with F_VIDX.
enum PartGroup { G_CSR, G_DENSE, G_CC0, G_CC1, G_CM0, G_CM1, G_SELL_VALUES, G_SELL_COLUMNS, G_SELLP, G_VIDX, G_XWIN0, G_XWIN1, G_XWIN2,
                 G_SELLP2, G_SELLPX, G_ROWT, G_XLDS_PLAN, G_XLDS_COLUMNS, G_SELLX, G_COUNT };
constexpr bool plan_keeps(int grp, int f, int vw_rows) {
    switch (grp) {
    case G_CSR:          return true;
    case G_DENSE:        return is_dense(f);
    case G_CC0: case G_CC1: return (is_cc16(f) || is_column_major(f)) && tile_plan(f) == grp - G_CC0;
    case G_CM0: case G_CM1: return is_column_major(f) && tile_plan(f) == grp - G_CM0;
    case G_SELL_VALUES:  return f == F_SELL || f == F_SELLP || f == F_SELLPX;
    case G_SELL_COLUMNS: return f == F_SELL;
    case G_SELLP:        return is_row_pattern(f);
    case G_VIDX:         return f == F_VIDX;
    case G_XWIN0: case G_XWIN1: case G_XWIN2: return f == F_VIDX && xwin_slot(vw_rows) == grp - G_XWIN0;
    case G_SELLP2:       return f == F_SELLP2;
    case G_SELLPX:       return f == F_SELLPX;
    case G_ROWT:         return f == F_ROWT;
    case G_XLDS_PLAN:    return is_xlds_chunk(f);
    case G_XLDS_COLUMNS: return f == F_XLDS || f == F_XLDSR;
    case G_SELLX:        return f == F_SELLX;
    }
    return true;
}

// a line of the plan cache: a form, a lanes setting, and x-window rows that F_VIDX alone may carry
constexpr bool plan_line_valid(int f, int lanes, int xwin_rows) {
    return f >= 0 && f < F_COUNT && lanes >= 1 && lanes <= 64 && (xwin_rows == 0 || (f == F_VIDX && xwin_slot(xwin_rows) >= 0));
}

// What the autotune times: a form at a lanes setting; xwin_rows != 0: F_VIDX in its x-window mode at that many rows per workgroup.
// The order -- form, direct gathers before x windows, then lanes or rows -- is the fixed order that breaks ties in choose_plan.
struct Candidate { int form, lanes, xwin_rows; };
inline bool operator<(const Candidate &a, const Candidate &b) { return std::tie(a.form, a.xwin_rows, a.lanes) < std::tie(b.form, b.xwin_rows, b.lanes); }
inline bool operator==(const Candidate &a, const Candidate &b) { return a.form == b.form && a.lanes == b.lanes && a.xwin_rows == b.xwin_rows; }

struct PlanChoice {
    Candidate best; float ms;                 // the plan and its time (0 where nothing was timed)
    Candidate runner_up; float runner_up_ms;  // the fastest of the others (form -1: there is no other)
    float fastest;                            // of the family that competed (column-major or the rest)
};

// The autotune's decision.  timed: every candidate with its best time (ms), in Candidate order; fallback: the plan in force before
// the sweep, kept where nothing was timed; direct_lanes: the lanes setting of the one-candidate forms.
//   * the column-major copy costs 2 B per entry more: its forms compete only where their fastest beats every other by 5 %, and
//     then among themselves;
//   * candidates within 3 % of the fastest: forms with the reference's sequential row sum first.  They are bit-identical to ONE
//     ANOTHER, so among them the choice cannot move a result and goes to the fastest; between forms whose sums differ it goes by the
//     fixed Candidate order, so that noise does not move a result;
//   * the x-window mode has to win clearly: direct gathers inside the band come first;
//   * runner-up: the fastest of all others, the first in order on a tie.
inline PlanChoice choose_plan(const std::map<Candidate, float> &timed, Candidate fallback, int direct_lanes) {
    float best = 1e30f, best_cm = 1e30f;
    for (const auto &kv : timed) {
        float &b = is_column_major(kv.first.form) ? best_cm : best;
        b = std::min(b, kv.second);
    }
    const bool cm_wins = best_cm < 0.95f * best;
    PlanChoice c{fallback, 0.0f, Candidate{-1, 0, 0}, 0.0f, cm_wins ? best_cm : best};
    const float bar = 1.03f * c.fastest;
    int brank = 1 << 30;
    for (const auto &kv : timed) {
        if (is_column_major(kv.first.form) != cm_wins || kv.second > bar) continue;
        const int rank = sequential_sum(kv.first.form, kv.first.lanes) ? 0 : 1;
        if (rank < brank || (rank == 0 && brank == 0 && kv.second < c.ms)) { brank = rank; c.best = kv.first; c.ms = kv.second; }
    }
    if (c.best.form == F_VIDX && c.best.xwin_rows) {
        const auto it = timed.find(Candidate{F_VIDX, direct_lanes, 0});
        if (it != timed.end() && it->second <= bar) { c.best = it->first; c.ms = it->second; }
    }
    for (const auto &kv : timed)
        if (!(kv.first == c.best) && (c.runner_up.form < 0 || kv.second < c.runner_up_ms)) { c.runner_up = kv.first; c.runner_up_ms = kv.second; }
    return c;
}

}   // namespace forms
