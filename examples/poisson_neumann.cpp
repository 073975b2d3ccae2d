// poisson_neumann.cpp -- a singular system through saena::amg::set_null_space("constant"):
//   ./poisson_neumann <n>
// The 7-point Laplacian of an n^3 box with Neumann boundaries (the graph Laplacian of the grid: A 1 = 0), set entry by entry through
// saena::matrix::set, and a right-hand side that is NOT consistent (its mean is about 0.5).  With the null space known the solver
// solves A u = b - mean(b) and returns the solution of zero mean.  Prints the pCG iteration count, ||b~ - A u|| / ||b~|| recomputed
// here in long double (b~ = b - mean(b)) and mean(u); then the first three nonzero eigenvalues through eigs (the constant vector is
// locked) next to the closed form 2 - 2 cos(k pi / n): the first is a triple, so K = 4 vectors and nev = 3.  One rank.
#include "saena.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: %s <n>\n", argv[0]); return 1; }
    const index_t n = atoi(argv[1]), N = n * n * n;
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;

    std::vector<index_t> row, col;
    std::vector<value_t> val;
    auto put = [&](index_t r, index_t c, value_t v) { row.push_back(r); col.push_back(c); val.push_back(v); };
    for (index_t k = 0; k < n; ++k)
        for (index_t j = 0; j < n; ++j)
            for (index_t i = 0; i < n; ++i) {
                const index_t r = (k * n + j) * n + i;
                const int deg = (i > 0) + (i < n - 1) + (j > 0) + (j < n - 1) + (k > 0) + (k < n - 1);
                if (k > 0) put(r, r - n * n, -1.0);
                if (j > 0) put(r, r - n, -1.0);
                if (i > 0) put(r, r - 1, -1.0);
                put(r, r, (value_t)deg);
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
    for (index_t i = 0; i < N; ++i) b[(size_t)i] = std::sin(0.37 * i) + 0.2 * std::cos(1.3 * i) + 0.5;

    saena::options opts(100, 1e-8, "jacobi", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);
    saena::amg solver;
    solver.set_scale(false);
    solver.set_null_space("constant");
    solver.set_matrix(&A, &opts);
    solver.set_rhs(b.data(), N);

    value_t *u = nullptr;
    const int st = solver.solve_pCG(u, &opts, false);

    long double bm = 0, um = 0;
    for (index_t i = 0; i < N; ++i) { bm += b[(size_t)i]; um += u[i]; }
    bm /= N; um /= N;
    std::vector<long double> r((size_t)N);
    for (index_t i = 0; i < N; ++i) r[(size_t)i] = (long double)b[(size_t)i] - bm;
    long double bb = 0, rr = 0;
    for (index_t i = 0; i < N; ++i) bb += r[(size_t)i] * r[(size_t)i];
    for (size_t e = 0; e < val.size(); ++e) r[(size_t)row[e]] -= (long double)val[e] * (long double)u[col[e]];
    for (index_t i = 0; i < N; ++i) rr += r[(size_t)i] * r[(size_t)i];
    printf("levels = %d, rows = %d, mean(b) = %e\n", solver.get_num_levels(), (int)N, (double)bm);
    printf("solve_pCG: %s, iterations = %d\n", st == 0 ? "converged" : "not converged", solver.last_iterations());
    printf("recomputed relative residual = %e\n", (double)std::sqrt(rr / bb));
    printf("mean(u) = %e\n", (double)um);

    const int K = 4, nev = 3;
    value_t *x = nullptr;
    std::vector<value_t> lambda;
    const int se = solver.eigs(x, lambda, &opts, K, nev);
    const double exact = 2.0 - 2.0 * std::cos(std::acos(-1.0) / n);
    printf("eigs with the constant vector locked: %d iterations\n", solver.last_iterations());
    for (int j = 0; j < nev; ++j) printf("lambda_%d = %.10e   closed form = %.10e\n", j + 1, lambda[(size_t)j], exact);
    printf("eigs: %s\n", se == 0 ? "every wanted pair converged" : "a wanted pair did not converge");

    saena::free_vector(x);
    saena::free_vector(u);
    solver.destroy();
    A.destroy();
    saena::finalize();
    return st ? st : se;
}
