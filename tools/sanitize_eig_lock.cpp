// sanitize_eig_lock.cpp -- saena_amd/csrc/eig_lock_plan.h (the sweep bookkeeping of sgpu_eigs_LOBPCG_many) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a stand-alone program on the host:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       tools/sanitize_eig_lock.cpp -o sanitize_eig_lock && ./sanitize_eig_lock
// (tests/test_eig_lock_ref.py builds and runs exactly this).
// It walks the driver's loop with the header's functions on arrays of exactly the sizes the driver allocates -- nev slots for the
// locked pairs, K columns of the block -- for scripted answers of the block solve: nev not a multiple of sweep_nev, a sweep that
// locks all K columns, nev = 1, a solve that reports more leading columns than fit, one that reports none, nev = 64 at K = 2, and
// equal eigenvalues in the final order.  An access outside an array is the sanitizer's to report (another exit status); a wrong
// count, a reused counter or a final order that is no stable ascending permutation fails a check below.
#include "../saena_amd/csrc/eig_lock_plan.h"

#include <cstdio>
#include <memory>
#include <set>

using namespace eig_lock;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// the driver's loop; leading[s] is what sweep s reports (the last entry repeats); -> sweeps run, or -1 when a sweep locked nothing
static int drive(int nev, int K, int sweep_nev, const std::vector<int> &leading, bool generated_start, int *locked_out) {
    std::unique_ptr<double[]> lam(new double[(size_t)nev]);          // exactly nev slots: one past the end is the sanitizer's
    std::unique_ptr<uint32_t[]> block(new uint32_t[(size_t)K]);      // the counter value each block column was filled from
    std::set<uint32_t> used;
    uint32_t counter = 0;
    if (!sweep_nev) sweep_nev = default_sweep_nev(K);
    if (generated_start)
        for (const Refill &r : refill_plan(K, &counter)) { CHECK(r.col >= 0 && r.col < K); block[r.col] = r.counter; CHECK(used.insert(r.counter).second); }
    int L = 0, sweeps = 0;
    while (L < nev) {
        const int want = sweep_want(nev, L, sweep_nev);
        CHECK(want >= 1 && want <= sweep_nev && want <= nev - L);
        const int lead = leading[std::min<size_t>((size_t)sweeps, leading.size() - 1)];
        ++sweeps;
        const int take = sweep_take(K, nev, L, lead);
        CHECK(take >= 0 && take <= K && take <= nev - L && take <= std::max(lead, 0));
        for (int j = 0; j < take; ++j) lam[(size_t)(L + j)] = 100.0 - (L + j) / 2;      // pairs of equal values, descending
        L += take;
        if (!take) { *locked_out = L; return -1; }
        if (L < nev) {
            const uint32_t before = counter;
            const std::vector<Refill> plan = refill_plan(take, &counter);
            CHECK((int)plan.size() == take && counter == before + (uint32_t)take);
            for (const Refill &r : plan) { CHECK(r.col >= 0 && r.col < take); block[r.col] = r.counter; CHECK(used.insert(r.counter).second); }
        }
    }
    CHECK(L == nev);
    const std::vector<int> perm = final_order(L, lam.get());
    CHECK((int)perm.size() == L);
    std::set<int> seen(perm.begin(), perm.end());
    CHECK((int)seen.size() == L && (L == 0 || (*seen.begin() == 0 && *seen.rbegin() == L - 1)));
    for (int k = 1; k < L; ++k) {
        CHECK(lam[(size_t)perm[(size_t)k - 1]] <= lam[(size_t)perm[(size_t)k]]);
        if (lam[(size_t)perm[(size_t)k - 1]] == lam[(size_t)perm[(size_t)k]]) CHECK(perm[(size_t)k - 1] < perm[(size_t)k]);      // stable
    }
    *locked_out = L;
    return sweeps;
}

int main() {
    int L = 0;
    CHECK(drive(20, 8, 4, {4}, true, &L) == 5 && L == 20);
    CHECK(drive(10, 8, 4, {4}, true, &L) == 3 && L == 10);             // nev no multiple of sweep_nev: 4 + 4 + 2
    CHECK(drive(7, 4, 3, {3, 4, 4}, false, &L) == 2 && L == 7);        // the second sweep locks all K = 4 columns
    CHECK(drive(20, 8, 4, {8}, true, &L) == 3 && L == 20);             // every sweep locks all K: 8 + 8 + 4
    CHECK(drive(1, 2, 0, {2}, true, &L) == 1 && L == 1);               // nev = 1, a solve that leads with more than fit
    CHECK(drive(1, 8, 8, {1}, false, &L) == 1 && L == 1);
    CHECK(drive(64, 2, 0, {1}, true, &L) == 64 && L == 64);            // the most sweeps: one pair each
    CHECK(drive(64, 8, 8, {8}, true, &L) == 8 && L == 64);
    CHECK(drive(12, 4, 2, {2, 0}, true, &L) == -1 && L == 2);          // a sweep that locks nothing ends the loop
    CHECK(drive(12, 4, 2, {99, -3}, true, &L) == -1 && L == 4);        // nonsense from the solve is clamped
    CHECK(default_sweep_nev(2) == 1 && default_sweep_nev(4) == 2 && default_sweep_nev(8) == 4);
    CHECK(sweep_want(20, 20, 4) == 0 && sweep_want(20, 25, 4) == 0 && sweep_take(8, 20, 20, 8) == 0);
    uint32_t c = 0xFFFFFFFEu;                                          // the counter wraps as an unsigned value does
    const std::vector<Refill> r = refill_plan(3, &c);
    CHECK(r.size() == 3 && r[0].counter == 0xFFFFFFFEu && r[2].counter == 0u && c == 1u);
    CHECK(refill_plan(0, &c).empty() && refill_plan(-2, &c).empty() && c == 1u);
    CHECK(final_order(0, nullptr).empty() && final_order(-1, nullptr).empty());
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
