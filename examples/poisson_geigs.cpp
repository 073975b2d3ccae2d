// poisson_geigs.cpp -- the smallest eigenpairs of the generalised problem K x = lambda M x through saena::amg::eigs_gen:
//   ./poisson_geigs <m> [nev = 4]
// K is the 3D 7-point Poisson operator on m^3 interior points (saena::laplacian3D on an (m+2)^3 grid, boundary rows removed), M the
// 27-point consistent mass matrix M1 x M1 x M1 (Kronecker), M1 = tridiag(1/6, 4/6, 1/6) of order m.  K and every factor of M are
// polynomials in the same 1-D second-difference matrix, so the eigenvectors are shared and the spectrum is known in closed form,
//   lambda = (m+1)^2 (t_i + t_j + t_k) / (mu_i mu_j mu_k),   t_i = 4 sin^2(pi i / (2 (m+1))),  mu_i = 1 - t_i / 6,  i, j, k = 1 .. m,
// in clusters of 1, 3, 3, 1, ... like the standard problem's (examples/poisson_eigs.cpp): nev = 4 ends at a gap.  A block of K = 4
// vectors, LOBPCG in the M-inner product, the V-cycle of K as preconditioner.  One rank.  Prints, per eigenvalue: lambda_j next to
// the closed form, and the residual ||K x - lambda M x||.
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
    if (m < 3 || nev < 1 || nev > K) { printf("m must be at least 3 (3 K = 12 rows are needed, and K closed-form values are printed), nev in 1..%d\n", K); return 1; }
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;

    saena::matrix A(comm);
    saena::laplacian3D(&A, mx, mx, mx);
    A.assemble();

    // the mass matrix: row (i, j, k) -> i + m (j + m k); entry M1[i][i'] M1[j][j'] M1[k][k'] for neighbours inside the grid
    saena::matrix M(comm);
    const double m1[3] = {1.0 / 6.0, 4.0 / 6.0, 1.0 / 6.0};
    for (index_t k = 0; k < m; ++k)
        for (index_t j = 0; j < m; ++j)
            for (index_t i = 0; i < m; ++i)
                for (int dk = -1; dk <= 1; ++dk)
                    for (int dj = -1; dj <= 1; ++dj)
                        for (int di = -1; di <= 1; ++di) {
                            const index_t i2 = i + di, j2 = j + dj, k2 = k + dk;
                            if (i2 < 0 || i2 >= m || j2 < 0 || j2 >= m || k2 < 0 || k2 >= m) continue;
                            M.set(i + m * (j + m * k), i2 + m * (j2 + m * k2), m1[di + 1] * m1[dj + 1] * m1[dk + 1]);
                        }
    M.assemble();

    saena::options opts(100, 1e-8, "jacobi", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);
    saena::amg solver;
    solver.set_scale(false);
    solver.set_matrix(&A, &opts);

    std::vector<value_t> exact;
    const double pi = std::acos(-1.0), s = (double)(m + 1) * (m + 1);
    auto mode = [&](int q) { const double t = std::sin(pi * q / (2.0 * (m + 1))); return 4.0 * t * t; };
    const int top = (int)std::min<index_t>(m, 4);
    for (int a = 1; a <= top; ++a)
        for (int b = 1; b <= top; ++b)
            for (int c = 1; c <= top; ++c) {
                const double ta = mode(a), tb = mode(b), tc = mode(c);
                exact.push_back(s * (ta + tb + tc) / ((1.0 - ta / 6.0) * (1.0 - tb / 6.0) * (1.0 - tc / 6.0)));
            }
    std::sort(exact.begin(), exact.end());

    value_t *x = nullptr;
    std::vector<value_t> lambda;
    const int st = solver.eigs_gen(x, lambda, &M, &opts, K, nev);
    const std::vector<value_t> &res = solver.eig_residuals();
    printf("generalised LOBPCG on %d^3 rows, 27-point mass matrix, K = %d, nev = %d: %d iterations\n", (int)m, K, nev, solver.last_iterations());
    for (int j = 0; j < K; ++j)
        printf("lambda_%d = %.10e   closed form = %.10e   residual = %e%s\n", j, lambda[(size_t)j], exact[(size_t)j], res[(size_t)j], j < nev ? "" : "   (guard vector)");
    printf("eigs_gen: %s\n", st == 0 ? "every wanted pair converged" : "a wanted pair did not converge");

    saena::free_vector(x);
    solver.destroy();
    M.destroy();
    A.destroy();
    saena::finalize();
    return st;
}
