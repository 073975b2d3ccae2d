// poisson_update.cpp -- a sequence of operators of one size through saena::amg::update1 / update2.
//   ./poisson_update <n> [steps = 3]
// Operator k is the 7-point Laplacian on an n^3 grid (x fastest) plus c_k times a fixed positive diagonal field (a reaction term
// that grows from step to step: c_k = 0.01 k, the field between 0.5 and 1.5).  Every operator is solved three ways with solve_pCG:
//   fresh    a new saena::amg, set_matrix: the whole smoothed-aggregation setup;
//   update2  one saena::amg built on operator 0, update2 at every step: R A P over the aggregates and transfer operators of operator 0;
//   update1  one saena::amg built on operator 0, update1 at every step: only the finest operator follows, the coarse ones stay operator 0's
//            (for operators that change little: the coarse correction is that of operator 0, and c_k is small against the grid's
//            smallest eigenvalue only on small grids).
// Prints, per step, the seconds of set_matrix / update2 / update1 (host setup and upload of the device operators) and the pCG
// iterations of each.  One rank.  Returns non-zero when a solve does not converge.
#include "saena.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void assemble(saena::matrix &A, index_t n, double c) {
    A.set_remove_boundary(false);
    for (index_t k = 0; k < n; ++k)
        for (index_t j = 0; j < n; ++j)
            for (index_t i = 0; i < n; ++i) {
                const index_t r = (k * n + j) * n + i;
                if (k > 0) A.set(r, r - n * n, -1.0);
                if (j > 0) A.set(r, r - n, -1.0);
                if (i > 0) A.set(r, r - 1, -1.0);
                A.set(r, r, 6.0 + c * (1.0 + 0.5 * std::sin(0.01 * r)));
                if (i < n - 1) A.set(r, r + 1, -1.0);
                if (j < n - 1) A.set(r, r + n, -1.0);
                if (k < n - 1) A.set(r, r + n * n, -1.0);
            }
    A.assemble();
}

// -> iterations, or -1 when the solve did not converge
int solve(saena::amg &S, saena::options &opts) {
    value_t *u = nullptr;
    const int st = S.solve_pCG(u, &opts, false);
    saena::free_vector(u);
    return st == 0 ? S.last_iterations() : -1;
}
} // namespace

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: %s <n> [steps]\n", argv[0]); return 1; }
    const index_t n = atoi(argv[1]);
    const int steps = argc > 2 ? atoi(argv[2]) : 3;
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;
    const index_t N = n * n * n;
    std::vector<value_t> b((size_t)N);
    for (index_t i = 0; i < N; ++i) b[(size_t)i] = std::sin(0.37 * i) + 0.2 * std::cos(1.3 * i) + 0.05;
    saena::options opts(100, 1e-8, "chebyshev", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);

    int failed = 0;
    {
        // the two kept hierarchies, built on operator 0; every matrix a hierarchy refers to stays alive until the hierarchy has moved on
        std::unique_ptr<saena::matrix> A2(new saena::matrix(comm)), A1(new saena::matrix(comm));
        assemble(*A2, n, 0.0);
        assemble(*A1, n, 0.0);
        saena::amg S2, S1;
        S2.set_matrix(A2.get(), &opts); S2.set_rhs(b.data(), N);
        S1.set_matrix(A1.get(), &opts); S1.set_rhs(b.data(), N);
        printf("rows = %d, levels = %d, steps = %d\n", (int)N, S2.get_num_levels(), steps);

        for (int k = 1; k <= steps; ++k) {
            const double c = 0.01 * k;
            saena::matrix Af(comm);
            assemble(Af, n, c);
            std::unique_ptr<saena::matrix> B2(new saena::matrix(comm)), B1(new saena::matrix(comm));
            assemble(*B2, n, c);
            assemble(*B1, n, c);

            double t = now();
            saena::amg Sf;
            Sf.set_matrix(&Af, &opts);
            const double t_fresh = now() - t;
            Sf.set_rhs(b.data(), N);

            t = now();
            S2.update2(B2.get());
            const double t_u2 = now() - t;
            A2->destroy(); A2 = std::move(B2);               // the old matrix may go once the update has returned

            t = now();
            S1.update1(B1.get());
            const double t_u1 = now() - t;
            A1->destroy(); A1 = std::move(B1);

            const int it_f = solve(Sf, opts), it_2 = solve(S2, opts), it_1 = solve(S1, opts);
            failed += (it_f < 0) + (it_2 < 0) + (it_1 < 0);
            printf("step %d (c = %.3f): set_matrix %.4f s, update2 %.4f s, update1 %.4f s; pCG iterations fresh %d, update2 %d, update1 %d%s\n", k, c,
                   t_fresh, t_u2, t_u1, it_f, it_2, it_1, (it_f < 0 || it_2 < 0 || it_1 < 0) ? "  (-1: not converged)" : "");
            Sf.destroy();
            Af.destroy();
        }
        S2.destroy(); S1.destroy();
        A2->destroy(); A1->destroy();
    }
    if (failed) printf("%d solves did not converge\n", failed); else printf("every solve converged\n");
    saena::finalize();
    return failed ? 1 : 0;
}
