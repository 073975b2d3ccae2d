// poisson_eigs.cpp -- the smallest eigenpairs of the 3D 7-point Poisson operator through saena::amg::eigs:
//   ./poisson_eigs <m> [nev = 4]
// m^3 interior points (saena::laplacian3D on an (m+2)^3 grid, boundary rows removed), a block of K = 4 vectors, LOBPCG with the
// V-cycle as preconditioner.  The spectrum is known in closed form,
//   lambda = (m+1)^2 sum_{d = x,y,z} 4 sin^2(pi k_d / (2 (m+1))),  k_d = 1 .. m,
// and its smallest values come in clusters of 1, 3, 3, 1, ...: nev = 4 ends at a gap, nev = 2 or 3 would cut a triple in two
// and converge slowly.  One rank.  Prints, per eigenvalue: lambda_j next to the closed form, and the residual ||A x - lambda x||.
#include "saena.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: %s <m> [nev]\n", argv[0]); return 1; }
    const index_t m = atoi(argv[1]), mx = m + 2;
    const int K = 4, nev = argc > 2 ? atoi(argv[2]) : 4;
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;

    saena::matrix A(comm);
    saena::laplacian3D(&A, mx, mx, mx);
    A.assemble();

    saena::options opts(100, 1e-8, "jacobi", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);
    saena::amg solver;
    solver.set_scale(false);
    solver.set_matrix(&A, &opts);

    std::vector<value_t> exact;
    const double pi = std::acos(-1.0), s = (double)(m + 1) * (m + 1);
    auto mode = [&](int k) { const double t = std::sin(pi * k / (2.0 * (m + 1))); return 4.0 * t * t; };
    const int top = (int)std::min<index_t>(m, 4);
    for (int a = 1; a <= top; ++a)
        for (int b = 1; b <= top; ++b)
            for (int c = 1; c <= top; ++c) exact.push_back(s * (mode(a) + mode(b) + mode(c)));
    std::sort(exact.begin(), exact.end());

    value_t *x = nullptr;
    std::vector<value_t> lambda;
    const int st = solver.eigs(x, lambda, &opts, K, nev);
    const std::vector<value_t> &res = solver.eig_residuals();
    printf("LOBPCG on %d^3 rows, K = %d, nev = %d: %d iterations\n", (int)m, K, nev, solver.last_iterations());
    for (int j = 0; j < K; ++j)
        printf("lambda_%d = %.10e   closed form = %.10e   residual = %e%s\n", j, lambda[(size_t)j], exact[(size_t)j], res[(size_t)j], j < nev ? "" : "   (guard vector)");
    printf("eigs: %s\n", st == 0 ? "every wanted pair converged" : "a wanted pair did not converge");

    saena::free_vector(x);
    solver.destroy();
    A.destroy();
    saena::finalize();
    return st;
}
