// sanitize_aggregation.cpp -- the threaded host setup (host/amg_setup.cpp: the aggregation's rounds dealt to threads, waiting
// rows pushed onto their blockers' chains with an atomic exchange; strength graph, smoothed P, products and filter on row
// chunks) under ThreadSanitizer, as a stand-alone program:
//   g++ -std=c++17 -O1 -g -fsanitize=thread -ffp-contract=off -Iinclude tools/sanitize_aggregation.cpp saena_amd/csrc/host/*.cpp \
//       -lpthread -lrt -ldl -o sanitize_aggregation && ./sanitize_aggregation 16 && ./sanitize_aggregation 1
// A weighted 7-point grid graph on m^3 vertices (default m = 36: 46 656 rows, above the 32 768 from which a round is dealt to
// threads; weights 10^U(-2, 2), 15 % of the edges deleted), two coarsening steps at the given number of setup threads.  Prints
// one line per level: rows, entries and a hash of the aggregates -- the lines of two thread counts must be equal.  A data race
// ends the program with ThreadSanitizer's report and status 66.
#include "../include/saena_c.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static double lcg_next(unsigned long long &s) {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (s >> 11) * (1.0 / 9007199254740992.0);
}

int main(int argc, char **argv) {
    const char *threads = argc > 1 ? argv[1] : "16";
    const int m = argc > 2 ? std::atoi(argv[2]) : 36;
    setenv("SAENA_SETUP_THREADS", threads, 1);               // read once, at the first threaded loop
    const int n = m * m * m;
    std::vector<index_t> rows, cols;
    std::vector<value_t> vals, diag((size_t)n, 1.0);
    unsigned long long seed = 3;
    auto edge = [&](int a, int b) {
        const double w = std::pow(10.0, 4.0 * lcg_next(seed) - 2.0);
        if (lcg_next(seed) < 0.15) return;
        rows.push_back(a); cols.push_back(b); vals.push_back(-w);
        rows.push_back(b); cols.push_back(a); vals.push_back(-w);
        diag[(size_t)a] += w; diag[(size_t)b] += w;
    };
    for (int x = 0; x < m; ++x)
        for (int y = 0; y < m; ++y)
            for (int z = 0; z < m; ++z) {
                const int i = (x * m + y) * m + z;
                if (x + 1 < m) edge(i, i + m * m);
                if (y + 1 < m) edge(i, i + m);
                if (z + 1 < m) edge(i, i + 1);
            }
    for (int i = 0; i < n; ++i) { rows.push_back(i); cols.push_back(i); vals.push_back(diag[(size_t)i]); }
    saena_comm *comm = saena_comm_self();
    saena_matrix_h *A = saena_matrix_new(comm);
    if (saena_matrix_set_many(A, rows.data(), cols.data(), vals.data(), (nnz_t)rows.size()) || saena_matrix_assemble(A)) { printf("assemble: %s\n", saena_last_error()); return 1; }
    saena_options_c o;
    saena_options_default(&o);
    o.smoother = 1; o.connStrength = 0.2f; o.max_level = 2; o.filter_thre = 1e-14; o.filter_max = 1e-8; o.filter_start = 1; o.filter_rate = 2;
    saena_amg_h *S = saena_amg_new();
    if (saena_amg_set_matrix(S, A, &o)) { printf("setup: %s\n", saena_last_error()); return 1; }
    const int nl = saena_amg_num_levels(S);
    for (int l = 0; l < nl; ++l) {
        index_t r = 0, nagg = 0;
        nnz_t na = 0, np_ = 0;
        double eig = 0;
        saena_amg_level_info(S, l, &r, &na, &np_, &eig);
        unsigned long long h = 1469598103934665603ULL;
        if (l < nl - 1) {
            std::vector<index_t> agg((size_t)r);
            if (saena_amg_level_aggregates(S, l, agg.data(), &nagg)) { printf("aggregates: %s\n", saena_last_error()); return 1; }
            for (index_t a : agg) h = (h ^ (unsigned long long)a) * 1099511628211ULL;
        }
        printf("level %d: %d rows, %ld entries, %d aggregates, hash %016llx, eig %.17g\n", l, (int)r, (long)na, (int)nagg, h, eig);
    }
    saena_amg_free(S);
    saena_matrix_free(A);
    saena_comm_free(comm);
    return 0;
}
