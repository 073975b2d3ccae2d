// sanitize_update.cpp -- update1 / update2 of the host hierarchy (host/amg_setup.cpp: amg_hierarchy::update, the tail of coarsen it
// shares with the setup; host/saena_c_api.cpp: saena_amg_update) under AddressSanitizer and UBSan, as a stand-alone program against
// the CPU build of the host library -- no interpreter, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -Iinclude tools/sanitize_update.cpp \
//       saena_amd/csrc/host/*.cpp -lpthread -lrt -ldl -o sanitize_update && ./sanitize_update 16 && ./sanitize_update 1
// A weighted 7-point grid graph on m^3 vertices (default m = 20; weights 10^U(-2, 2), 15 % of the edges deleted) at the given number
// of setup threads: set_matrix -> update2 with a shifted diagonal (the old matrix is freed right after: nothing may read it again) ->
// update1 -> three refused updates (another size, mode 3, a matrix that was never assembled) -> update2 once more -> free.
// Prints rows and entries of every level after each step; the lines of two thread counts must be equal.  An AddressSanitizer finding
// ends the program with its report; UBSan prints "runtime error" lines and goes on.  Known, from assemble() and not from the update:
// SelfComm::alltoallv (host/comm.h) hands memcpy two null pointers for an exchange of zero bytes.
#include "../include/saena_c.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static double lcg_next(unsigned long long &s) {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (s >> 11) * (1.0 / 9007199254740992.0);
}

struct Entries { std::vector<index_t> rows, cols; std::vector<value_t> vals; int n = 0; };

static Entries wgrid(int m, double shift, int cut = 0) {
    Entries e;
    const int n = m * m * m - cut;                           // cut > 0: the last vertices are left out (another size)
    e.n = n;
    std::vector<value_t> diag((size_t)n, 1.0);
    unsigned long long seed = 3;
    auto edge = [&](int a, int b) {
        const double w = std::pow(10.0, 4.0 * lcg_next(seed) - 2.0);
        if (lcg_next(seed) < 0.15 || a >= n || b >= n) return;
        e.rows.push_back(a); e.cols.push_back(b); e.vals.push_back(-w);
        e.rows.push_back(b); e.cols.push_back(a); e.vals.push_back(-w);
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
    for (int i = 0; i < n; ++i) { e.rows.push_back(i); e.cols.push_back(i); e.vals.push_back(diag[(size_t)i] + shift * (1.0 + (i % 5) * 0.25)); }
    return e;
}

static saena_matrix_h *matrix(saena_comm *c, const Entries &e, bool assemble = true) {
    saena_matrix_h *A = saena_matrix_new(c);
    saena_matrix_set_remove_boundary(A, 0);
    if (saena_matrix_set_many(A, e.rows.data(), e.cols.data(), e.vals.data(), (nnz_t)e.vals.size())) { printf("set_many: %s\n", saena_last_error()); exit(2); }
    if (assemble && saena_matrix_assemble(A)) { printf("assemble: %s\n", saena_last_error()); exit(2); }
    return A;
}

static void report(const char *what, saena_amg_h *S) {
    printf("%-28s", what);
    for (int l = 0; l < saena_amg_num_levels(S); ++l) {
        index_t rows = 0; nnz_t nnz = 0, nnzP = 0; double eig = 0;
        saena_amg_level_info(S, l, &rows, &nnz, &nnzP, &eig);
        printf("  L%d %d rows %ld entries eig %.6f", l, (int)rows, (long)nnz, eig);
    }
    printf("\n");
}

static void must(int status, const char *what) {
    if (status) { printf("%s failed: %s\n", what, saena_last_error()); exit(3); }
}

static void must_refuse(int status, const char *what, const char *word) {
    if (!status || !std::strstr(saena_last_error(), word)) { printf("%s: expected a refusal that says \"%s\", got status %d \"%s\"\n", what, word, status, saena_last_error()); exit(4); }
    printf("refused (%s): %s\n", what, saena_last_error());
}

int main(int argc, char **argv) {
    const char *threads = argc > 1 ? argv[1] : "16";
    const int m = argc > 2 ? std::atoi(argv[2]) : 20;
    setenv("SAENA_SETUP_THREADS", threads, 1);               // read once, at the first threaded loop
    saena_comm *c = saena_comm_self();
    saena_options_c o;
    saena_options_default(&o);
    o.connStrength = 0.2f; o.max_level = 3; o.filter_thre = 1e-3; o.filter_max = 1e-1;     // Chebyshev (find_eig runs), a filter that rewrites levels

    saena_matrix_h *A = matrix(c, wgrid(m, 0.0));
    saena_amg_h *S = saena_amg_new();
    must_refuse(saena_amg_update(S, A, 2), "no set_matrix yet", "set_matrix");
    must(saena_amg_set_matrix(S, A, &o), "set_matrix");
    report("set_matrix", S);

    saena_matrix_h *B = matrix(c, wgrid(m, 5.0));
    must(saena_amg_update(S, B, 2), "update2");
    saena_matrix_free(A);                                    // the hierarchy no longer refers to it
    report("update2 (shifted)", S);

    saena_matrix_h *C1 = matrix(c, wgrid(m, 0.5));
    must(saena_amg_update(S, C1, 1), "update1");
    saena_matrix_free(B);
    report("update1", S);

    saena_matrix_h *small = matrix(c, wgrid(m, 0.0, 7)), *loose = matrix(c, wgrid(m, 0.0), false);
    must_refuse(saena_amg_update(S, small, 2), "another size", "rows");
    must_refuse(saena_amg_update(S, C1, 3), "mode 3", "mode 3");
    must_refuse(saena_amg_update(S, loose, 2), "never assembled", "not assembled");
    report("after the refusals", S);

    saena_matrix_h *D = matrix(c, wgrid(m, 0.05));
    must(saena_amg_update(S, D, 2), "update2 again");
    saena_matrix_free(C1);
    report("update2 (nearly the first)", S);

    saena_amg_free(S);
    saena_matrix_free(D); saena_matrix_free(small); saena_matrix_free(loose);
    saena_comm_free(c);
    printf("done\n");
    return 0;
}
