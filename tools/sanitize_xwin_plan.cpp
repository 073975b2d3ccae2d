// sanitize_xwin_plan.cpp -- saena_amd/csrc/xwin_plan.h (the plans build_xwin, build_sellpx and build_vidx upload) under
// AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program on the host:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       tools/sanitize_xwin_plan.cpp -o sanitize_xwin_plan && ./sanitize_xwin_plan
// (tests/test_xwin_plan_header.py builds and runs exactly this).
// The edge cases of that test: every refusal clause of both plans on both sides of its edge, with the inputs that sit next to an
// overflow -- an offset near 2^31 on either side, seventeen windows, S of 65536 and 65537, the LDS cap to the byte, slices of close
// to 2^31 code bytes.  An access outside a vector or an overflow is the sanitizer's to report (another exit status); a wrong verdict,
// or a table entry that does not map back to its pattern's offset, fails a check below.
#include "../saena_amd/csrc/xwin_plan.h"

#include <cstdio>

using namespace xwplan;
using Patterns = std::vector<std::vector<int>>;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// one window of S doubles for workgroups of R rows: offsets 0 ... S - R in steps of R
static std::vector<int> dense(int S, int R) {
    std::vector<int> o;
    for (int v = 0; v < S - R; v += R) o.push_back(v);
    o.push_back(S - R);
    return o;
}
static std::vector<int> every(int step, int n) { std::vector<int> o; for (int k = 0; k < n; ++k) o.push_back(step * k); return o; }

// plan_vidxw on the patterns as build_sellp lays them out, dictionaries of three values; an accepted plan's table by round trip
static int vidxw(const Patterns &pats, int W, int M, int ncols, int R, int uw) {
    const int npat = (int)pats.size();
    std::vector<int> tab((size_t)npat * (W + 1), 0), dptr((size_t)((M + 63) / 64 + 3) / 4 + 1);
    for (size_t b = 0; b < dptr.size(); ++b) dptr[b] = 3 * (int)b;
    for (int i = 0; i < npat; ++i) {
        tab[(size_t)i * (W + 1)] = (int)pats[(size_t)i].size();
        for (int j = 0; j < std::min(W, (int)pats[(size_t)i].size()); ++j) tab[(size_t)i * (W + 1) + 1 + j] = pats[(size_t)i][(size_t)j];
    }
    const VwPlan p = plan_vidxw(tab.data(), npat, W, M, ncols, R, uw, dptr.data(), false);
    if (p.refusal) { CHECK(p.tab.empty() && p.win.empty()); return p.refusal; }
    const sk::VwHead &h = p.s.head;
    CHECK((int)p.tab.size() == h.tn && (int)p.win.size() == 2 + 2 * std::max(h.nwin, 4) && p.s.lds <= sk::VW_MAX_LDS && h.vd_u == 3);
    for (int i = 0; i < npat; ++i) {
        const std::vector<int> &o = pats[(size_t)i];
        CHECK((size_t)p.tab[(size_t)i] == o.size());
        for (int j = 0; j < p.s.wp; ++j) {
            const int at = p.tab[(size_t)h.lp + (size_t)i * p.s.wp + j];
            CHECK(at % 8 == 0 && at / 8 < h.S);
            const int want = o.empty() ? 0 : o[std::min((size_t)j, o.size() - 1)];
            int holds = 0;
            for (int c = 0; c < h.nwin; ++c) {
                const int lo = p.win[2 + 2 * (size_t)c], hi = c + 1 < h.nwin ? p.win[4 + 2 * (size_t)c] : h.S;
                if (lo <= at / 8 && at / 8 < hi) { ++holds; CHECK(o.empty() || (int64_t)at / 8 + p.win[3 + 2 * (size_t)c] == want); }
            }
            CHECK(holds == 1);
        }
    }
    return ACCEPTED;
}

// plan_sellpx with every row on pattern ids[r]; an accepted plan's tables by round trip
static int spx(const Patterns &pats, const std::vector<unsigned short> &ids) {
    std::vector<int> pstart, ptab;
    for (const std::vector<int> &o : pats) { pstart.push_back((int)ptab.size()); ptab.push_back((int)o.size()); ptab.insert(ptab.end(), o.begin(), o.end()); }
    const int M = (int)ids.size();
    const SpxPlan p = plan_sellpx(pstart, ptab, ids, M);
    if (p.refusal) return p.refusal;
    CHECK(8 * p.S + 2 * p.max_words <= sk::SPX_LDS_BYTES && p.tab.size() == (size_t)p.wgptr.back() + 8 && (int)p.win.size() == 1 + 3 * p.nwin);
    for (int r = 0; r < M; ++r) {
        const int g = r / sk::SPX_ROWS;
        const unsigned short *t = &p.tab[(size_t)p.wgptr[(size_t)g]];
        const int words = p.wgptr[(size_t)g + 1] - p.wgptr[(size_t)g], at = t[p.pat[(size_t)r]];
        const std::vector<int> &o = pats[ids[(size_t)r]];
        CHECK(words % 4 == 0 && at < words && t[at] == o.size() && at + (int)o.size() < words);
        for (size_t j = 0; j < o.size(); ++j) {
            int holds = 0;
            for (int c = 0; c < p.nwin; ++c) {
                const int lo = p.win[2 + 3 * (size_t)c], size = p.win[3 + 3 * (size_t)c];
                if (lo <= t[at + 1 + j] && t[at + 1 + j] < lo + size) { ++holds; CHECK(t[at + 1 + j] - lo + p.win[1 + 3 * (size_t)c] == o[j]); }
            }
            CHECK(holds == 1);
        }
    }
    return SPX_ACCEPTED;
}

int main() {
    const int FAR = INT32_MAX - 8 - 1000 - 256 - 512;          // M + R + S + FAR = INT32_MAX - 8 on 1000 rows at R = 256 with two windows
    // ---- plan_vidxw ----
    CHECK(vidxw({{0, 1, 2}}, 3, 300, 300, 256, 8) == ACCEPTED);
    CHECK(vidxw({{0, 1, 2, 3}}, 3, 300, 300, 256, 8) == PATTERN_LENGTH);
    { const int bad[] = {-1, 0, 0, 0}, dptr[] = {0, 3, 6}; CHECK(plan_vidxw(bad, 1, 3, 300, 300, 256, 8, dptr, false).refusal == PATTERN_LENGTH); }
    CHECK(vidxw({{}, {5}}, 1, 300, 300, 256, 8) == ACCEPTED);
    CHECK(vidxw({{}, {}}, 1, 300, 300, 256, 8) == NO_ENTRIES);
    CHECK(vidxw({}, 1, 300, 300, 256, 8) == NO_ENTRIES);
    for (int R : {256, 512, 1024}) {
        CHECK(vidxw({every(1100, 16)}, 16, 300, 20000, R, 16) == (R == 256 ? ACCEPTED : LDS_CAP));
        CHECK(vidxw({every(1100, 17)}, 17, 300, 20000, R, 24) == WINDOW_COUNT);
        CHECK(vidxw({dense(65536, R)}, 257, 300, 70000, R, 8) == LDS_CAP);
        CHECK(vidxw({dense(65537, R)}, 257, 300, 70000, R, 8) == POSITIONS_16);
        CHECK(vidxw({{-3, 0, 300}, {0}, {}}, 3, 3000, 3000, R, 8) == ACCEPTED);
    }
    CHECK(vidxw({dense(7925, 256)}, 31, 300, 9000, 256, 8) == ACCEPTED);           // 7926 * 8 + 2048 + 2 * (8 + 32) = VW_MAX_LDS
    CHECK(vidxw({dense(7926, 256)}, 31, 300, 9000, 256, 8) == LDS_CAP);
    CHECK(vidxw({dense(7925, 256)}, 33, 300, 9000, 256, 8) == LDS_CAP);
    CHECK(vidxw({{0, 1}}, 8, 300, 300, 256, 8) == ACCEPTED);
    CHECK(vidxw({{0, 1}}, 8, 300, 300, 256, 16) == SLICE_WIDTH);
    CHECK(vidxw({{0}, {FAR}}, 1, 1000, 1000, 256, 8) == ACCEPTED);
    CHECK(vidxw({{0}, {FAR + 1}}, 1, 1000, 1000, 256, 8) == COLUMNS_32);
    CHECK(vidxw({{-FAR}, {0}}, 1, 1000, 1000, 256, 8) == ACCEPTED);
    CHECK(vidxw({{-FAR - 1}, {0}}, 1, 1000, 1000, 256, 8) == COLUMNS_32);
    CHECK(vidxw({{INT32_MIN}, {INT32_MAX}}, 1, 1000, 1000, 256, 8) == COLUMNS_32);
    // ---- plan_sellpx ----
    const std::vector<unsigned short> ten(10, 0);
    CHECK(spx({{}}, ten) == SPX_NO_ENTRIES);
    CHECK(spx({every(1100, 16)}, ten) == SPX_ACCEPTED);
    CHECK(spx({every(1100, 17)}, ten) == SPX_WINDOW_COUNT);
    CHECK(spx({dense(65535, 512)}, ten) == SPX_WINDOWS_LDS);
    CHECK(spx({dense(65536, 512)}, ten) == SPX_POSITIONS_16);
    CHECK(spx({{INT32_MIN, INT32_MAX}}, ten) == SPX_ACCEPTED);               // (two windows of 512 doubles, however far apart)
    CHECK(spx({dense(10240, 512)}, ten) == SPX_WINDOWS_LDS);
    {   // S = 10239 leaves four words for a workgroup's table; the second pattern, which no row follows, keeps the window in one piece
        std::vector<int> rest = dense(10239, 512);
        rest.erase(rest.begin()); rest.pop_back();
        CHECK(spx({{0, 9727}, rest}, ten) == SPX_ACCEPTED);
        CHECK(spx({{0, 512, 9727}, rest}, ten) == SPX_TABLE);
    }
    {   // a workgroup of empty rows, a partial last workgroup, no row at all
        std::vector<unsigned short> ids(512, 0);
        ids.insert(ids.end(), 512, 1);
        ids.insert(ids.end(), 100, 2);
        CHECK(spx({{0, 1}, {}, {-600, 0, 700}}, ids) == SPX_ACCEPTED);
        CHECK(spx({{0, 1}}, {}) == SPX_ACCEPTED);
    }
    // ---- slice_widths ----
    {
        const int big = ((INT32_MAX - 1024) / 64) & ~7;
        const int one[] = {0, big}, more[] = {0, big + 1}, none[] = {0};
        CHECK(slice_widths(one, 1).ok && slice_widths(one, 1).uw == big && slice_widths(one, 1).tot == (int64_t)64 * big);
        CHECK(!slice_widths(more, 1).ok);
        CHECK(slice_widths(none, 0).ok && slice_widths(none, 0).uw == 0 && slice_widths(none, 0).ptr.size() == 1);
        std::vector<int> rp(66, 0);
        for (int r = 0; r < 65; ++r) rp[(size_t)r + 1] = rp[(size_t)r] + (r < 64 ? 9 : 3);
        const SliceWidths s = slice_widths(rp.data(), 65);
        CHECK(s.ok && s.uw == 16 && s.tot == 2 * 64 * 16 && s.ptr[1] == 1024 && s.ptr[2] == 1536);
    }
    if (failures) { std::printf("FAILED: %d checks\n", failures); return 1; }
    std::printf("ok: xwin_plan.h under ASan + UBSan\n");
    return 0;
}
