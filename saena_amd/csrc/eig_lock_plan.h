// eig_lock_plan.h -- the sweep bookkeeping of sgpu_eigs_LOBPCG_many (sgpu_eig_lock.hip.inc) as pure host functions: no GPU, no
// library state, testable alone (tests/test_eig_lock_ref.py holds it to its numpy restatement, tools/sanitize_eig_lock.cpp runs its
// edge cases under the sanitizers).
//
// A sweep is one constrained block solve on K columns for `want` pairs.  It reports `leading`: how many leading columns of the block
// are converged on recomputed norms.  The driver locks min(leading, nev - nlocked) of them -- ALL that converged, which can be more
// than were asked for --, the others stay where they are as the next sweep's start vectors, and the freed columns (always the first
// `take` columns of the block) are refilled from the generator with a counter that runs over the whole call and is never reused.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace eig_lock {

constexpr int MAX_LOCKED = 64;

// the default number of pairs a sweep asks for: half the block as guard vectors (at least one pair)
inline int default_sweep_nev(int K) { return std::max(1, K / 2); }

// how many pairs the next sweep asks for
inline int sweep_want(int nev, int nlocked, int sweep_nev) { return std::max(0, std::min(sweep_nev, nev - nlocked)); }

// how many leading columns are locked after a sweep
inline int sweep_take(int K, int nev, int nlocked, int leading) { return std::max(0, std::min(std::min(leading, K), nev - nlocked)); }

struct Refill { int col; uint32_t counter; };

// the columns refilled after `take` columns were locked, with their counter values; *counter advances by take.
// (the start block of a call without start vectors is refill_plan(K, &counter) from counter = 0)
inline std::vector<Refill> refill_plan(int take, uint32_t *counter) {
    std::vector<Refill> r;
    for (int j = 0; j < take; ++j) r.push_back(Refill{j, (*counter)++});
    return r;
}

// perm[k] = the locked column that goes to position k: ascending lambda, stable (equal values keep their locking order)
inline std::vector<int> final_order(int nlocked, const double *lambda) {
    std::vector<int> perm((size_t)std::max(0, nlocked));
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return lambda[a] < lambda[b]; });
    return perm;
}

} // namespace eig_lock
