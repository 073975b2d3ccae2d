// xwin_plan.h -- the host's plans for the kernels that keep x in LDS windows, as pure functions of the operator's patterns: the
// windows (one clustering, one lookup), the tables and heads of k_vidxw / k_vidxw_fast and of k_sellpx, and the slice widths of the
// value-indexed form.  Plain C++17, no HIP, no environment, no output, no device memory: build_vidx, build_xwin and build_sellpx read
// back, call, upload and report; a host compiler can run and sanitize every address the kernels form from these tables
// (tests/test_xwin_plan_header.py, tools/sanitize_xwin_plan.cpp).
//
// Windows.  The offsets (column - row) of all patterns fall into clusters: a gap of more than `gap` columns between neighbours begins
// a new one.  A workgroup of `rows` rows starting at r0 needs x inside [r0 + omin_c, r0 + rows + omax_c) per cluster c; the windows
// lie one after the other in LDS, window c at `base_c`, S doubles in all.  A pattern's entry becomes the LDS position of its column
// for the workgroup's FIRST row: base_c + (offset - omin_c); a lane adds its row's index in the workgroup.
//
// k_vidxw (workgroups of R = 256 << k rows, the gap rule at R): build_sellp's ONE pattern table (npat rows of W + 1 ints: length,
// then offsets) is rewritten ONCE for the whole operator as 16-bit words -- the patterns' lengths (lp words, padded to a multiple of
// 8), then per pattern wp (a multiple of 8) LDS BYTE offsets, the tail repeating the last real one (read, never added; an empty
// pattern reads offset 0).  The window list as uploaded: nwin, S, then (base, omin - base) per window, at least four (unused: INT32_MAX,
// which never matches -- the kernel reads the first four unconditionally).  The head (VwHead) carries the first four windows, the
// table's word counts, the dictionaries' common length, the shortest and the longest pattern and, where xwin_stage.h's rule allows
// it, the trips that stage the windows one by one.  Refused: see Refusal.
//
// k_sellpx (workgroups of SPX_ROWS rows, the gap rule at SPX_ROWS): positions in doubles, and every workgroup gets its own small table
// -- the patterns its rows follow, in order of first appearance -- with its rows' ids counting within it.  The form applies when
// windows and the largest of these tables fit SPX_LDS_BYTES (two workgroups per CU).  Its limits are its own, not k_vidxw's.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "vw_fast.h"
#include "vw_masks.h"

namespace xwplan {

// ---- the windows ----
struct Windows {
    std::vector<int> omin, omax, base;         // per window: first and last offset, LDS position of the first
    int64_t S = 0;                             // doubles of x in all (base holds positions only while S fits an int: the callers refuse long before)
    int nwin() const { return (int)omin.size(); }
    int size(int c, int rows) const { return rows + (omax[(size_t)c] - omin[(size_t)c]); }
    int window(int off) const { return (int)(std::upper_bound(omin.begin(), omin.end(), off) - omin.begin()) - 1; }      // the window that holds the offset
    int position(int off) const { const size_t w = (size_t)window(off); return base[w] + (off - omin[w]); }              // ... and its place in the layout
};
// offs: the sorted distinct offsets
inline Windows cluster(const std::vector<int> &offs, int gap, int rows) {
    Windows w;
    for (size_t i = 0; i < offs.size(); ++i) {
        if (i == 0 || (int64_t)offs[i] - offs[i - 1] > gap) { w.omin.push_back(offs[i]); w.omax.push_back(offs[i]); }
        else w.omax.back() = offs[i];
    }
    for (size_t c = 0; c < w.omin.size(); ++c) { w.base.push_back((int)std::min<int64_t>(w.S, INT32_MAX)); w.S += (int64_t)rows + ((int64_t)w.omax[c] - w.omin[c]); }
    return w;
}
inline void sort_distinct(std::vector<int> &offs) {
    std::sort(offs.begin(), offs.end());
    offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
}

// ---- k_vidxw ----
enum Refusal : int { ACCEPTED = 0, PATTERN_LENGTH, NO_ENTRIES, WINDOW_COUNT, POSITIONS_16, COLUMNS_32, SLICE_WIDTH, LDS_CAP };
constexpr const char *refusal_text(int r) {
    return r == PATTERN_LENGTH ? "a pattern longer than the table's width" : r == NO_ENTRIES ? "no entries" : r == WINDOW_COUNT ? "more windows than SPX_MAXWIN"
         : r == POSITIONS_16 ? "LDS positions beyond 16 bits" : r == COLUMNS_32 ? "column arithmetic beyond 32 bits" : r == SLICE_WIDTH ? "slices wider than the table"
         : r == LDS_CAP ? "windows, dictionaries and table exceed the LDS cap" : "accepted";
}
// what of the plan stays with the operator once its arrays are uploaded: head: k_vidxw's second argument; wp: positions per pattern;
// lds: k_vidxw's LDS bytes; fast: the operator's part of k_vidxw_fast's argument where vw_fast.h's rule takes the operator at this R
// (fast_kind 1: dictionaries in LDS, 2: in scalar registers; 0: the general kernel, fast_clause says which clause refused), fast_lds:
// its LDS bytes
struct VwScalars {
    sk::VwHead head{};
    int wp = 0, lds = 0;
    vwfast::VwFast fast{};
    int fast_kind = 0, fast_clause = 0, fast_lds = 0;
    int mask_clause = vwmasks::NOT_SCALAR;     // vw_masks.h's rule at this R: TAKEN -> fast.slot_off holds the slots, the rows can be lane masks
};
struct VwPlan {
    int refusal = ACCEPTED;
    VwScalars s;
    std::vector<unsigned short> tab;           // the table as 16-bit words
    std::vector<int> win;                      // the window list as uploaded
    std::vector<unsigned char> pslot;          // mask rows (mask_clause TAKEN or SWITCHED_OFF): pattern x position -> slot, vwmasks::MAXSLOT per pattern
};
// tab: the pattern table as read back, npat rows of W + 1 ints; M x ncols: the operator; R: rows per workgroup; uw: the slices' common
// code width (0: they differ); dptr: where the dictionaries begin, one per 256 rows and the end; fast_off: SAENA_VIDXW_FAST=0;
// masks_off: SAENA_VIDXW_MASKS=0
inline VwPlan plan_vidxw(const int *tab, int npat, int W, int M, int ncols, int R, int uw, const int *dptr, bool fast_off, bool masks_off = false) {
    VwPlan p;
    auto no = [&](Refusal r) { p.refusal = r; return p; };
    std::vector<int> offs;
    for (int i = 0; i < npat; ++i) {
        const int *c = &tab[(size_t)i * (W + 1)];
        if (c[0] < 0 || c[0] > W) return no(PATTERN_LENGTH);
        offs.insert(offs.end(), c + 1, c + 1 + c[0]);
    }
    sort_distinct(offs);
    if (offs.empty()) return no(NO_ENTRIES);
    const Windows w = cluster(offs, R, R);
    const int nwin = w.nwin();
    const int64_t S = w.S;
    if (nwin > sk::SPX_MAXWIN) return no(WINDOW_COUNT);
    if (S > 65536) return no(POSITIONS_16);
    if ((int64_t)M + R + S + std::max<int64_t>(std::abs((int64_t)offs.front()), std::abs((int64_t)offs.back())) > (int64_t)INT32_MAX - 8) return no(COLUMNS_32);
    const int wp = (W + 7) & ~7, lp = (npat + 7) & ~7;
    if (uw > wp) return no(SLICE_WIDTH);
    const int64_t words = (int64_t)lp + (int64_t)npat * wp;
    const int64_t lds = ((S + 2) & ~(int64_t)1) * 8 + (int64_t)(R / 256) * sk::VI_MAX * 8 + words * 2;
    if (lds > (int64_t)sk::VW_MAX_LDS) return no(LDS_CAP);
    sk::VwHead &h = p.s.head;
    p.tab.assign((size_t)words, 0);
    h.lmin = h.lmax = tab[0];
    for (int i = 0; i < npat; ++i) {
        const int *c = &tab[(size_t)i * (W + 1)];
        p.tab[(size_t)i] = (unsigned short)c[0];
        h.lmin = std::min(h.lmin, c[0]); h.lmax = std::max(h.lmax, c[0]);
        unsigned short last = 0;                                  // (an empty row reads position 0 and adds nothing)
        for (int j = 0; j < wp; ++j) {
            if (j < c[0]) last = (unsigned short)(8 * w.position(c[1 + j]));      // (a byte offset: S doubles fit the LDS cap, so below 64 KiB)
            p.tab[(size_t)lp + (size_t)i * wp + j] = last;      // (the tail repeats the last position: read, never added)
        }
    }
    p.win.assign(2 + 2 * (size_t)std::max(nwin, 4), INT32_MAX);          // (the kernel reads the first four windows unconditionally: unused ones never match)
    p.win[0] = nwin; p.win[1] = (int)S;
    for (int c = 0; c < nwin; ++c) { p.win[2 + 2 * (size_t)c] = w.base[(size_t)c]; p.win[3 + 2 * (size_t)c] = w.omin[(size_t)c] - w.base[(size_t)c]; }
    // the dictionaries' common length, where they have one: the kernel then computes where a workgroup's values begin and reads no vi_dptr
    const int ngd = ((M + 63) / 64 + 3) / 4;
    int vd_u = ngd > 0 ? dptr[1] - dptr[0] : 0;
    for (int b = 1; b < ngd; ++b) if (dptr[(size_t)b + 1] - dptr[(size_t)b] != vd_u) vd_u = 0;
    h.nwin = nwin; h.S = (int)S;
    std::copy(p.win.begin() + 2, p.win.begin() + 10, h.win);
    h.lp = lp; h.tn = (int)words; h.vd_u = vd_u;
    // window by window where xwin_stage.h's rule allows it (else ntrip = 0: the flat staging)
    h.ntrip = 0;
    if (xwstage::per_window(nwin, S, R, ncols, M, w.omin.front(), w.omax.back())) {
        std::vector<int> size;
        for (int c = 0; c < nwin; ++c) size.push_back(w.size(c, R));
        h.ntrip = xwstage::trips(nwin, w.base.data(), w.omin.data(), size.data(), R, h.trip);
    }
    p.s.wp = wp; p.s.lds = (int)lds;
    // the common-path kernel where vw_fast.h's rule takes the operator at this R
    p.s.fast_clause = vwfast::refused(R, uw, vd_u, h.ntrip, (int)(words >> 3));
    if (p.s.fast_clause == vwfast::TAKEN && fast_off) p.s.fast_clause = vwfast::SWITCHED_OFF;
    p.s.fast_kind = vwfast::kind(p.s.fast_clause, vd_u);
    if (p.s.fast_kind)
        p.s.fast_lds = vwfast::plan(p.s.fast, R, (M + 63) / 64, ncols, (int)S, lp, (int)words, wp, uw, vd_u, h.lmin, h.lmax, h.trip, p.s.fast_kind == 2);
    // the rows as lane masks where vw_masks.h's rule takes the table: the slots' LDS byte offsets are the longest pattern's positions
    p.pslot.assign((size_t)npat * vwmasks::MAXSLOT, (unsigned char)vwmasks::NO_SLOT);
    int nslot = 0;
    p.s.mask_clause = vwmasks::rule(p.s.fast_kind, p.tab.data(), p.tab.data() + lp, npat, wp, masks_off, &nslot, p.s.fast.slot_off, p.pslot.data());
    if (p.s.mask_clause != vwmasks::TAKEN && p.s.mask_clause != vwmasks::SWITCHED_OFF) p.pslot.clear();
    return p;
}

// ---- k_sellpx ----
enum SpxRefusal : int { SPX_ACCEPTED = 0, SPX_NO_ENTRIES, SPX_WINDOW_COUNT, SPX_POSITIONS_16, SPX_WINDOWS_LDS, SPX_TABLE };
struct SpxPlan {
    int refusal = SPX_ACCEPTED;
    int nwin = 0;
    int64_t S = 0, max_words = 0;              // doubles of x per workgroup; words of the largest workgroup's table
    std::vector<unsigned short> tab, pat;      // the workgroups' tables back to back (+ 8 words of padding); workgroup-local pattern ids per row
    std::vector<int> wgptr, win;               // table of workgroup g: words [wgptr[g], wgptr[g + 1]); windows: count, then (omin, LDS base, size) each
};
// the host copy of the patterns: pattern i is ptab[pstart[i]] = its length, then its offsets; pat: the rows' pattern ids
inline SpxPlan plan_sellpx(const std::vector<int> &pstart, const std::vector<int> &ptab, const std::vector<unsigned short> &pat, int M) {
    SpxPlan p;
    auto no = [&](SpxRefusal r) { p.refusal = r; return p; };
    const int npat = (int)pstart.size(), ROWS = sk::SPX_ROWS;
    std::vector<int> offs;
    for (int i = 0; i < npat; ++i) {
        const int *c = &ptab[(size_t)pstart[(size_t)i]];
        offs.insert(offs.end(), c + 1, c + 1 + c[0]);
    }
    sort_distinct(offs);
    if (offs.empty()) return no(SPX_NO_ENTRIES);
    const Windows w = cluster(offs, ROWS, ROWS);
    const int64_t S = w.S;
    p.nwin = w.nwin(); p.S = S;
    if (p.nwin > sk::SPX_MAXWIN) return no(SPX_WINDOW_COUNT);
    if (S > 65535) return no(SPX_POSITIONS_16);
    if (S * 8 >= (int64_t)sk::SPX_LDS_BYTES) return no(SPX_WINDOWS_LDS);
    const int64_t room = ((int64_t)sk::SPX_LDS_BYTES - S * 8) / 2;           // 16-bit words left for a workgroup's table
    // every pattern once as (length, LDS positions)
    std::vector<unsigned short> pos16;
    std::vector<int> pstart16((size_t)npat + 1, 0);
    for (int i = 0; i < npat; ++i) {
        const int *c = &ptab[(size_t)pstart[(size_t)i]];
        pstart16[(size_t)i] = (int)pos16.size();
        pos16.push_back((unsigned short)c[0]);
        for (int j = 0; j < c[0]; ++j) pos16.push_back((unsigned short)w.position(c[1 + j]));
        if (c[0] == 0) pos16.push_back(0);                        // (an empty row reads position 0 and adds nothing)
    }
    pstart16[(size_t)npat] = (int)pos16.size();
    const int ngrp = (M + ROWS - 1) / ROWS;
    p.wgptr.assign((size_t)ngrp + 1, 0);
    p.pat.assign(pat.size(), 0);
    std::vector<int> local((size_t)npat, -1), used;
    for (int g = 0; g < ngrp; ++g) {
        used.clear();
        const int r1 = std::min(M, (g + 1) * ROWS);
        for (int r = g * ROWS; r < r1; ++r) {
            const int id = pat[(size_t)r];
            if (local[(size_t)id] < 0) { local[(size_t)id] = (int)used.size(); used.push_back(id); }
            p.pat[(size_t)r] = (unsigned short)local[(size_t)id];
        }
        if (used.empty()) { used.push_back(0); }
        int64_t words = (int64_t)used.size();
        for (int id : used) words += pstart16[(size_t)id + 1] - pstart16[(size_t)id];
        words = (words + 3) / 4 * 4;
        p.max_words = std::max(p.max_words, words);
        if (words > room || words > 65535 || (int64_t)p.tab.size() + words > (int64_t)INT32_MAX - 8) return no(SPX_TABLE);
        const size_t t0 = p.tab.size();
        p.tab.resize(t0 + (size_t)words, 0);
        size_t at = t0 + used.size();
        for (size_t k = 0; k < used.size(); ++k) {
            const int id = used[k];
            p.tab[t0 + k] = (unsigned short)(at - t0);
            for (int q = pstart16[(size_t)id]; q < pstart16[(size_t)id + 1]; ++q) p.tab[at++] = pos16[(size_t)q];
            local[(size_t)id] = -1;
        }
        p.wgptr[(size_t)g + 1] = (int)p.tab.size();
    }
    p.win.assign(1 + 3 * (size_t)p.nwin, 0);
    p.win[0] = p.nwin;
    for (int c = 0; c < p.nwin; ++c) { p.win[1 + 3 * (size_t)c] = w.omin[(size_t)c]; p.win[2 + 3 * (size_t)c] = w.base[(size_t)c]; p.win[3 + 3 * (size_t)c] = w.size(c, ROWS); }
    p.tab.resize(p.tab.size() + 8, 0);
    return p;
}

// ---- the slices of the value-indexed form: 64 rows each, padded to the longest row rounded up to 8 positions ----
struct SliceWidths {
    bool ok = false;                           // the codes fit 32-bit positions
    std::vector<int> ptr;                      // where the slices' codes begin, and the end
    int uw = 0;                                // every slice has this many code positions (a narrower last slice is padded up), or 0: read ptr
    int64_t tot = 0;                           // code bytes
};
// rp: the CSR row pointer, M + 1 entries
inline SliceWidths slice_widths(const int *rp, int M) {
    SliceWidths s;
    const int ns = (M + 63) / 64;
    s.ptr.assign((size_t)ns + 1, 0);
    bool uniform = true;
    int w8_0 = 0;
    for (int k = 0; k < ns; ++k) {
        int w = 0;
        for (int r = k * 64; r < std::min(M, k * 64 + 64); ++r) w = std::max(w, rp[(size_t)r + 1] - rp[(size_t)r]);
        const int w8 = (w + 7) & ~7;
        if (k == 0) w8_0 = w8;
        else if (w8 != w8_0 && !(k == ns - 1 && w8 < w8_0)) uniform = false;     // (a narrower last slice is padded up)
        s.tot += (int64_t)w8 * 64;
        if (s.tot > (int64_t)INT32_MAX - 1024) return s;
        s.ptr[(size_t)k + 1] = (int)s.tot;
    }
    if (uniform && w8_0 > 0 && (int64_t)ns * w8_0 * 64 <= (int64_t)INT32_MAX - 1024) { s.tot = (int64_t)ns * w8_0 * 64; s.uw = w8_0; }
    s.ok = true;
    return s;
}

}
