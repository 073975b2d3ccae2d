// poisson_fgmres.cpp -- a nonsymmetric operator through the C++ surface: restarted flexible GMRES with the V-cycle as preconditioner.
//   ./poisson_fgmres <n> [pe = 4] [restart = 30]
// Upwinded convection-diffusion on an n^3 grid (x fastest): the 7-point Laplacian plus pe times first-order upwind differences with
// velocities (1, 0.5, 0.25), set entry by entry through saena::matrix::set.  solve_pCG is not defined for it; solve_pFGMRES is.
// The setup is the product's own (smoothed aggregation, Jacobi smoother).  One rank.
// Prints the inner iterations and ||b - A u|| / ||b|| recomputed on the host in extended precision.
#include "saena.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: %s <n> [pe] [restart]\n", argv[0]); return 1; }
    const index_t n = atoi(argv[1]);
    const double pe = argc > 2 ? atof(argv[2]) : 4.0;
    const int restart = argc > 3 ? atoi(argv[3]) : 30;
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;

    std::vector<index_t> row, col;
    std::vector<value_t> val;
    auto put = [&](index_t r, index_t c, value_t v) { row.push_back(r); col.push_back(c); val.push_back(v); };
    const index_t N = n * n * n;
    for (index_t k = 0; k < n; ++k)
        for (index_t j = 0; j < n; ++j)
            for (index_t i = 0; i < n; ++i) {
                const index_t r = (k * n + j) * n + i;
                if (k > 0) put(r, r - n * n, -1.0 - 0.25 * pe);
                if (j > 0) put(r, r - n, -1.0 - 0.5 * pe);
                if (i > 0) put(r, r - 1, -1.0 - pe);
                put(r, r, 6.0 + 1.75 * pe);
                if (i < n - 1) put(r, r + 1, -1.0);
                if (j < n - 1) put(r, r + n, -1.0);
                if (k < n - 1) put(r, r + n * n, -1.0);
            }
    saena::matrix A(comm);
    A.set_remove_boundary(false);
    for (size_t e = 0; e < val.size(); ++e) A.set(row[e], col[e], val[e]);
    A.assemble();
    if (A.get_num_local_rows() != N) { printf("matrix rows: %d, expected %d\n", (int)A.get_num_local_rows(), (int)N); return 2; }

    std::vector<value_t> b((size_t)N);
    for (index_t i = 0; i < N; ++i) b[(size_t)i] = std::sin(0.37 * i) + 0.2 * std::cos(1.3 * i) + 0.05;

    saena::options opts(100, 1e-8, "jacobi", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);
    saena::amg solver;
    solver.set_scale(false);
    solver.set_matrix(&A, &opts);
    solver.set_rhs(b.data(), N);

    value_t *u = nullptr;
    const int st = solver.solve_pFGMRES(u, &opts, restart, true);

    std::vector<long double> r(b.begin(), b.end());
    for (size_t e = 0; e < val.size(); ++e) r[(size_t)row[e]] -= (long double)val[e] * (long double)u[col[e]];
    long double rr = 0, bb = 0;
    for (index_t i = 0; i < N; ++i) { rr += r[(size_t)i] * r[(size_t)i]; bb += (long double)b[(size_t)i] * b[(size_t)i]; }
    printf("levels = %d, rows = %d, pe = %g, restart = %d\n", solver.get_num_levels(), (int)N, pe, restart);
    printf("solve_pFGMRES: %s, iterations = %d\n", st == 0 ? "converged" : "not converged", solver.last_iterations());
    printf("recomputed relative residual = %e\n", (double)std::sqrt(rr / bb));

    saena::free_vector(u);
    solver.destroy();
    A.destroy();
    saena::finalize();
    return st;
}
