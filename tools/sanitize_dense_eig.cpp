// sanitize_dense_eig.cpp -- host/dense_eig.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Iinclude \
//       tools/sanitize_dense_eig.cpp saena_amd/csrc/host/dense_eig.cpp -o sanitize_dense_eig && ./sanitize_dense_eig
// (tests/test_dense_eig.py builds and runs exactly this).  Every order 1 .. 24 the Rayleigh-Ritz step can ask for, in arrays of
// exactly n * n doubles on the heap, so that an index past the order is an error: a well-conditioned pair, a pair with a
// repeated eigenvalue, an indefinite B, a B with a NaN, and orders outside 1 .. 24.  Exit status 0 and "ok" when the residuals
// are small; a sanitizer report ends the program with another status.
#include "../saena_amd/csrc/host/dense_eig.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace saena_host;

static double lcg_next(unsigned long long &s) {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return ((s >> 11) * (1.0 / 9007199254740992.0)) * 2.0 - 1.0;
}

int main() {
    unsigned long long seed = 12345;
    double worst = 0.0;
    for (int n = 1; n <= DENSE_EIG_MAXN; ++n) {
        const size_t nn = (size_t)n * n;
        std::vector<double> A(nn), B(nn), M(nn), w((size_t)n), V(nn);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) { A[(size_t)i * n + j] = A[(size_t)j * n + i] = lcg_next(seed); M[(size_t)i * n + j] = lcg_next(seed); M[(size_t)j * n + i] = lcg_next(seed); }
        for (int i = 0; i < n; ++i)                                   // B = M M^T / n + I
            for (int j = 0; j < n; ++j) {
                double s = i == j ? 1.0 : 0.0;
                for (int k = 0; k < n; ++k) s += M[(size_t)i * n + k] * M[(size_t)j * n + k] / n;
                B[(size_t)i * n + j] = s;
            }
        for (int rep = 0; rep < 2; ++rep) {
            if (rep == 1)                                             // a repeated eigenvalue: A = 2 B + a rank-one term
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < n; ++j) A[(size_t)i * n + j] = 2.0 * B[(size_t)i * n + j] + (i == 0 && j == 0 ? 1.0 : 0.0);
            const int st = dense_sym_geig(n, A.data(), B.data(), w.data(), V.data());
            if (st < 0) { printf("order %d: status %d\n", n, st); return 1; }
            for (int k = 0; k < n; ++k) {
                double r2 = 0.0, v2 = 0.0;
                for (int i = 0; i < n; ++i) {
                    double s = 0.0;
                    for (int j = 0; j < n; ++j) s += (A[(size_t)i * n + j] - w[(size_t)k] * B[(size_t)i * n + j]) * V[(size_t)j * n + k];
                    r2 += s * s; v2 += V[(size_t)i * n + k] * V[(size_t)i * n + k];
                }
                worst = std::fmax(worst, std::sqrt(r2 / v2));
                if (k && w[(size_t)k] < w[(size_t)k - 1]) { printf("order %d: eigenvalues not ascending\n", n); return 1; }
            }
        }
        std::vector<double> Bad(B);
        Bad[nn - 1] = -1.0;                                           // not positive definite: reported, not factored
        if (dense_sym_geig(n, A.data(), Bad.data(), w.data(), V.data()) != -1) { printf("order %d: an indefinite B was accepted\n", n); return 1; }
        Bad[nn - 1] = std::numeric_limits<double>::quiet_NaN();
        if (dense_sym_geig(n, A.data(), Bad.data(), w.data(), V.data()) != -1) { printf("order %d: a NaN in B was accepted\n", n); return 1; }
        std::vector<double> L(nn), T(nn);
        if (!dense_cholesky(n, B.data(), L.data())) { printf("order %d: Cholesky refused a positive definite matrix\n", n); return 1; }
        dense_inv_lower_transposed(n, L.data(), T.data());
        if (dense_sym_eig(n, A.data(), w.data(), V.data()) < 0) { printf("order %d: Jacobi failed\n", n); return 1; }
    }
    double one = 1.0, out = 0.0;
    if (dense_sym_geig(0, &one, &one, &out, &out) != -3 || dense_sym_geig(DENSE_EIG_MAXN + 1, &one, &one, &out, &out) != -3) { printf("an order outside 1 .. 24 was accepted\n"); return 1; }
    if (!(worst < 1e-12)) { printf("largest residual %g\n", worst); return 1; }
    printf("ok: orders 1 .. %d, largest residual %.2e\n", DENSE_EIG_MAXN, worst);
    return 0;
}
