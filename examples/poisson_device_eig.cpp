// poisson_device_eig.cpp -- the Chebyshev smoother's eig_max from the device: saena::amg::set_device_eig and saena::matrix::estimate_eig.
//   ./poisson_device_eig <n>
// The 7-point Laplacian on an n^3 grid (x fastest) plus a small positive diagonal field, under the Chebyshev smoother:
//   host     a saena::amg as it is by default: every level's eig_max from the host Lanczos loop;
//   device   a saena::amg after set_device_eig(true): the same recurrence on the card, for the setup and for update2;
//   own      the caller's own estimate: B.set_eig(B.estimate_eig()) before update1 on the default saena::amg -- no host loop runs.
// Prints the estimates and the pCG iterations of each.  One rank.  Returns non-zero when a solve does not converge, when the two
// hierarchies disagree on the iterations by more than one (the estimates differ in their last bits), or when an estimate is not a usable bound (D^-1 A of this operator has lambda_max < 2).
#include "saena.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
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
    if (argc < 2) { printf("usage: %s <n>\n", argv[0]); return 1; }
    const index_t n = atoi(argv[1]);
    saena::init(0, 0, 1, nullptr);
    saena::comm comm;
    const index_t N = n * n * n;
    std::vector<value_t> b((size_t)N);
    for (index_t i = 0; i < N; ++i) b[(size_t)i] = std::sin(0.37 * i) + 0.2 * std::cos(1.3 * i) + 0.05;
    saena::options opts(100, 1e-8, "chebyshev", 3, 3, "jacobi", 0.2f, true, 20, 3, 1e-14, 1e-8, 1, 2);

    int failed = 0;
    {
        saena::matrix Ah(comm), Ad(comm), Bh(comm), Bd(comm), Bo(comm);
        assemble(Ah, n, 0.0); assemble(Ad, n, 0.0);
        assemble(Bh, n, 0.02); assemble(Bd, n, 0.02); assemble(Bo, n, 0.02);

        const double e20 = Ah.estimate_eig(), e20b = Ah.estimate_eig(20), e5 = Ah.estimate_eig(5);
        printf("rows = %d: estimate_eig() = %.15g, with 5 steps %.15g\n", (int)N, e20, e5);
        failed += !(e20 == e20b) + !(e5 < e20) + !(e20 > 1.0 && e20 < 2.0 * 1.0001);

        saena::amg Sh, Sd;
        Sd.set_device_eig(true);
        Sh.set_matrix(&Ah, &opts); Sh.set_rhs(b.data(), N);
        Sd.set_matrix(&Ad, &opts); Sd.set_rhs(b.data(), N);
        int it_h = solve(Sh, opts), it_d = solve(Sd, opts);
        printf("set_matrix: pCG iterations host %d, device %d (%d levels)\n", it_h, it_d, Sd.get_num_levels());
        failed += (it_h < 0) + (it_d < 0) + (std::abs(it_h - it_d) > 1);

        Sh.update2(&Bh);
        Sd.update2(&Bd);
        it_h = solve(Sh, opts); it_d = solve(Sd, opts);
        printf("update2:    pCG iterations host %d, device %d\n", it_h, it_d);
        failed += (it_h < 0) + (it_d < 0) + (std::abs(it_h - it_d) > 1);

        const double own = Bo.estimate_eig();
        Bo.set_eig(own);
        Sh.update1(&Bo);                                    // the value set on Bo is kept: update1 estimates nothing
        const int it_o = solve(Sh, opts);
        printf("update1 after set_eig(estimate_eig() = %.15g): pCG iterations %d\n", own, it_o);
        failed += (it_o < 0) + !(own > 1.0 && own < 2.0 * 1.0001);

        Sh.destroy(); Sd.destroy();
    }
    if (failed) printf("%d checks failed\n", failed); else printf("every check passed\n");
    saena::finalize();
    return failed ? 1 : 0;
}
