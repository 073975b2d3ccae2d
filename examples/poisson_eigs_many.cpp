// poisson_eigs_many.cpp -- the first 20 modes of the 3D 7-point Poisson operator through saena::amg::eigs_many:
//   ./poisson_eigs_many <m> [nev = 20]
// m^3 interior points (saena::laplacian3D on an (m+2)^3 grid, boundary rows removed).  More pairs than a block of K = 8 vectors
// holds: sweeps of LOBPCG (the V-cycle as preconditioner) for 4 pairs each with 4 guard vectors; what converges is locked and the
// block goes on in the orthogonal complement of what is locked.  The spectrum is known in closed form,
//   lambda = (m+1)^2 sum_{d = x,y,z} 4 sin^2(pi k_d / (2 (m+1))),  k_d = 1 .. m,
// in clusters of 1, 3, 3, 3, 1, 6, ...; sweeps of 4 cut them, and every value still comes with its multiplicity.  One rank.
// Prints, per eigenvalue: lambda_j next to the closed form, the residual ||A x - lambda x||, and whether
// |lambda_j - closed form_j| <= residual (the bound of a normalised x for a symmetric matrix); exit status 0 when all nev pairs
// converged inside it.
#include "saena.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: %s <m> [nev]\n", argv[0]); return 1; }
    const index_t m = atoi(argv[1]), mx = m + 2;
    const int K = 8, nev = argc > 2 ? atoi(argv[2]) : 20;
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;

    saena::matrix A(comm);
    saena::laplacian3D(&A, mx, mx, mx);
    A.assemble();

    saena::options opts(400, 1e-8, "jacobi", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);      // 400: the total over all sweeps
    saena::amg solver;
    solver.set_scale(false);
    solver.set_matrix(&A, &opts);

    std::vector<value_t> exact;
    const double pi = std::acos(-1.0), s = (double)(m + 1) * (m + 1);
    auto mode = [&](int k) { const double t = std::sin(pi * k / (2.0 * (m + 1))); return 4.0 * t * t; };
    const int top = (int)std::min<index_t>(m, 8);
    for (int a = 1; a <= top; ++a)
        for (int b = 1; b <= top; ++b)
            for (int c = 1; c <= top; ++c) exact.push_back(s * (mode(a) + mode(b) + mode(c)));
    std::sort(exact.begin(), exact.end());

    value_t *q = nullptr;
    std::vector<value_t> lambda;
    const int st = solver.eigs_many(q, lambda, &opts, nev, K);
    const std::vector<value_t> &res = solver.eig_residuals();
    printf("LOBPCG with locking on %d^3 rows, K = %d, nev = %d: %d pairs in %d iterations, %d sweeps\n", (int)m, K, nev, (int)lambda.size(),
           solver.last_iterations(), solver.eig_sweeps());
    int outside = 0;
    for (size_t j = 0; j < lambda.size(); ++j) {
        const bool in = std::fabs(lambda[j] - exact[j]) <= res[j];
        outside += !in;
        printf("lambda_%zu = %.10e   closed form = %.10e   residual = %e   %s\n", j, lambda[j], exact[j], res[j], in ? "within the bound" : "OUTSIDE the bound");
    }
    printf("eigs_many: %s\n", st == 0 ? "every wanted pair converged" : "the iterations ran out: the pairs above are those locked so far");

    saena::free_vector(q);
    solver.destroy();
    A.destroy();
    saena::finalize();
    return st || outside;
}
