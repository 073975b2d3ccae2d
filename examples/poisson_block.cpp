// poisson_block.cpp -- examples/poisson.cpp's problem with several right-hand sides through ONE solve:
//   ./poisson_block <mx> [nrhs = 4]
// 3D 7-point Poisson on an mx^3 grid; column j of the block is the reference's right-hand side times 2^j, so every column
// must take the iterations of the scalar ./poisson run and reach its final residual times 2^j.  One rank.
// Prints, per column: iterations, initial and final residual.
#include "saena.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: %s <mx> [nrhs]\n", argv[0]); return 1; }
    const index_t mx = atoi(argv[1]);
    const int nrhs = argc > 2 ? atoi(argv[2]) : 4;
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;

    saena::matrix A(comm);
    saena::laplacian3D(&A, mx, mx, mx);
    A.assemble();

    // the right-hand side over the whole grid, boundary included, as the reference generates it; the assembled system keeps the
    // interior rows in their order (what saena::amg::set_rhs(saena::vector&) does with the boundary rows: it drops them)
    value_t *rhs_std = nullptr;
    index_t first = 0;
    const index_t sz = saena::laplacian3D_set_rhs(rhs_std, mx, mx, mx, comm, &first);
    const index_t n = A.get_num_local_rows();
    std::vector<value_t> interior;
    for (index_t g = 0; g < sz; ++g) {
        const index_t i = g % mx, j = (g / mx) % mx, k = g / (mx * mx);
        if (i == 0 || j == 0 || k == 0 || i == mx - 1 || j == mx - 1 || k == mx - 1) continue;
        interior.push_back(rhs_std[g]);
    }
    if ((index_t)interior.size() != n) { printf("interior rows: %zu, matrix rows: %d\n", interior.size(), (int)n); return 2; }
    std::vector<value_t> B((size_t)n * nrhs);                 // column-major n x nrhs
    for (int c = 0; c < nrhs; ++c)
        for (index_t r = 0; r < n; ++r) B[(size_t)c * n + r] = std::ldexp(interior[(size_t)r], c);

    saena::options opts(50, 1e-8, "jacobi", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);
    saena::amg solver;
    solver.set_scale(false);
    solver.set_matrix(&A, &opts);
    solver.set_rhs_block(B.data(), n, nrhs);

    value_t *u = nullptr;
    const int st = solver.solve_pCG_block(u, &opts);
    for (int c = 0; c < nrhs; ++c) {
        const std::vector<value_t> &h = solver.residual_history_block(c);
        printf("column %d: iterations = %d, initial residual = %e, final absolute residual = %e\n", c, (int)h.size() - 1, h.front(), h.back());
    }
    printf("solve_pCG_block: %s\n", st == 0 ? "every column converged" : "a column did not converge");

    saena::free_vector(u);
    free(rhs_std);
    solver.destroy();
    A.destroy();
    saena::finalize();
    return st;
}
