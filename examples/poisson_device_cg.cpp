// poisson_device_cg.cpp -- a coarsest level past 1 024 rows: saena::amg::set_coarse_solver("device_cg").
//   ./poisson_device_cg <n> [max_level = 1]
// The 7-point Laplacian on an n^3 grid (x fastest) with the hierarchy cut off at `max_level`, so that its coarsest level is larger
// than the LDS-resident solvers hold (n = 24, max_level = 1: 5 324 rows):
//   default    a saena::amg as it is: "direct" falls back to the host-driven CG loop there, and the V-cycle is not captured;
//   device_cg  a saena::amg after set_coarse_solver("device_cg"): the same CG with its scalars on the device, inside the V-cycle's graph.
// Prints the pCG iterations and the solve time of each, and the largest difference of the two solutions.  One rank.  Returns non-zero
// when a solve does not converge, when the iterations differ by more than one (the dots of the two CGs are summed in different
// orders), when the solutions differ by more than 1e-6 relative (the solves stop at 1e-8), or when an unknown name is accepted.
#include "saena.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

namespace {
void assemble(saena::matrix &A, index_t n) {
    A.set_remove_boundary(false);
    for (index_t k = 0; k < n; ++k)
        for (index_t j = 0; j < n; ++j)
            for (index_t i = 0; i < n; ++i) {
                const index_t r = (k * n + j) * n + i;
                if (k > 0) A.set(r, r - n * n, -1.0);
                if (j > 0) A.set(r, r - n, -1.0);
                if (i > 0) A.set(r, r - 1, -1.0);
                A.set(r, r, 6.0);
                if (i < n - 1) A.set(r, r + 1, -1.0);
                if (j < n - 1) A.set(r, r + n, -1.0);
                if (k < n - 1) A.set(r, r + n * n, -1.0);
            }
    A.assemble();
}

// -> iterations, or -1 when the solve did not converge; the second solve is the timed one (the first one captures the graph)
int solve(saena::amg &S, saena::options &opts, std::vector<value_t> &x, double *ms) {
    int it = -1;
    for (int rep = 0; rep < 2; ++rep) {
        value_t *u = nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        const int st = S.solve_pCG(u, &opts, false);
        *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        x.assign(u, u + x.size());
        saena::free_vector(u);
        it = st == 0 ? S.last_iterations() : -1;
    }
    return it;
}
} // namespace

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: %s <n> [max_level]\n", argv[0]); return 1; }
    const index_t n = atoi(argv[1]);
    const int max_level = argc > 2 ? atoi(argv[2]) : 1;
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;
    const index_t N = n * n * n;
    std::vector<value_t> b((size_t)N);
    for (index_t i = 0; i < N; ++i) b[(size_t)i] = std::sin(0.37 * i) + 0.2 * std::cos(1.3 * i) + 0.05;
    saena::options opts(100, 1e-8, "chebyshev", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);

    int failed = 0;
    {
        saena::matrix Ah(comm), Ad(comm);
        assemble(Ah, n); assemble(Ad, n);
        saena::amg Sh, Sd;
        bool refused = false;
        try { Sd.set_coarse_solver("lu"); } catch (const std::runtime_error &) { refused = true; }
        failed += !refused;
        Sd.set_coarse_solver("device_cg");
        Sh.set_multigrid_max_level(max_level); Sd.set_multigrid_max_level(max_level);
        Sh.set_matrix(&Ah, &opts); Sh.set_rhs(b.data(), N);
        Sd.set_matrix(&Ad, &opts); Sd.set_rhs(b.data(), N);
        printf("rows = %d, %d levels\n", (int)N, Sd.get_num_levels());

        std::vector<value_t> xh((size_t)N), xd((size_t)N);
        double ms_h = 0, ms_d = 0;
        const int it_h = solve(Sh, opts, xh, &ms_h), it_d = solve(Sd, opts, xd, &ms_d);
        double diff = 0, nrm = 0;
        for (index_t i = 0; i < N; ++i) { diff = std::fmax(diff, std::fabs(xh[(size_t)i] - xd[(size_t)i])); nrm = std::fmax(nrm, std::fabs(xh[(size_t)i])); }
        printf("default:   pCG iterations %d, %.3f ms\n", it_h, ms_h);
        printf("device_cg: pCG iterations %d, %.3f ms\n", it_d, ms_d);
        printf("largest difference of the solutions, relative: %.3e\n", nrm > 0 ? diff / nrm : diff);
        failed += (it_h < 0) + (it_d < 0) + (std::abs(it_h - it_d) > 1) + !(diff <= 1e-6 * nrm);
        Sh.destroy(); Sd.destroy();
    }
    if (failed) printf("%d checks failed\n", failed); else printf("every check passed\n");
    saena::finalize();
    return failed ? 1 : 0;
}
