// sanitize_null_space.cpp -- saena_amd/csrc/coarse_pinv.h (the dense factorisations behind the direct coarsest solve, host only) under
// AddressSanitizer and UBSan, as a stand-alone program -- no interpreter, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off tools/sanitize_null_space.cpp \
//       -o sanitize_null_space && ./sanitize_null_space
// The edges of both functions: n = 0, 1 and 2, the path Laplacian at 1 024 rows (the most the LDS-resident solvers hold), a zero
// matrix (refused by both), a matrix whose first pivot needs a row swap.  Checks A A^+ = I - 1 1^T / n and that every row and column
// of A^+ sums to rounding.  Prints "every check passed" and returns 0, or the number of failed checks.
#include "../saena_amd/csrc/coarse_pinv.h"

#include <cstdio>

static std::vector<double> path(int n) {
    std::vector<double> a((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        a[(size_t)i * n + i] = (i > 0) + (i < n - 1);
        if (i > 0) a[(size_t)i * n + i - 1] = -1.0;
        if (i < n - 1) a[(size_t)i * n + i + 1] = -1.0;
    }
    return a;
}

int main() {
    int failed = 0;
    auto want = [&](bool ok, const char *what) { if (!ok) { printf("FAILED: %s\n", what); ++failed; } };
    std::vector<double> a, inv, pinv;

    a.clear();
    want(coarse_pinv::gauss_jordan_inverse(a, 0, inv) && inv.empty(), "n = 0: the empty inverse");
    want(coarse_pinv::pseudo_inverse(a, 0, pinv) && pinv.empty(), "n = 0: the empty pseudo-inverse");

    a = {4.0};
    want(coarse_pinv::gauss_jordan_inverse(a, 1, inv) && inv[0] == 0.25, "n = 1: 1 / a");
    a = {4.0};
    want(coarse_pinv::pseudo_inverse(a, 1, pinv) && pinv[0] == 0.0, "n = 1: the complement of constants is empty");
    a = {0.0};
    want(!coarse_pinv::gauss_jordan_inverse(a, 1, inv), "n = 1, a = 0: refused");
    a = {0.0};
    want(!coarse_pinv::pseudo_inverse(a, 1, pinv), "n = 1, a = 0: refused");

    a = path(2);
    want(!coarse_pinv::gauss_jordan_inverse(a, 2, inv), "path(2): the plain elimination meets an exact zero");
    a = path(2);
    want(coarse_pinv::pseudo_inverse(a, 2, pinv) && pinv[0] == 0.25 && pinv[1] == -0.25 && pinv[2] == -0.25 && pinv[3] == 0.25, "path(2): its pseudo-inverse");
    a = {0.0, 2.0, 2.0, 0.0};
    want(coarse_pinv::gauss_jordan_inverse(a, 2, inv) && inv[0] == 0.0 && inv[1] == 0.5 && inv[2] == 0.5 && inv[3] == 0.0, "a zero on the diagonal: the row swap");

    a.assign(9, 0.0);
    want(!coarse_pinv::gauss_jordan_inverse(a, 3, inv), "a zero matrix: refused");
    a.assign(9, 0.0);
    want(!coarse_pinv::pseudo_inverse(a, 3, pinv), "a zero matrix: no scale to shift by, refused");

    const int n = 1024;
    a = path(n);
    want(coarse_pinv::pseudo_inverse(a, n, pinv) && pinv.size() == (size_t)n * n, "path(1024)");
    const std::vector<double> A = path(n);
    double worst = 0.0, sums = 0.0, big = 0.0;
    for (int i = 0; i < n; ++i) {
        double r = 0.0, c = 0.0;
        for (int j = 0; j < n; ++j) { r += pinv[(size_t)i * n + j]; c += pinv[(size_t)j * n + i]; big = std::fmax(big, std::fabs(pinv[(size_t)i * n + j])); }
        sums = std::fmax(sums, std::fmax(std::fabs(r), std::fabs(c)));
        for (int j = 0; j < n; j += 37) {                 // (A A^+)_ij on a sample of columns: three products per entry
            double s = 0.0;
            for (int k = (i > 0 ? i - 1 : 0); k <= (i < n - 1 ? i + 1 : n - 1); ++k) s += A[(size_t)i * n + k] * pinv[(size_t)k * n + j];
            worst = std::fmax(worst, std::fabs(s - ((i == j ? 1.0 : 0.0) - 1.0 / n)));
        }
    }
    want(sums <= 1e-12 * n * big, "path(1024): rows and columns of the pseudo-inverse sum to rounding");
    want(worst <= 1e-8, "path(1024): A A^+ = I - 1 1^T / n");

    if (!failed) printf("every check passed\n");
    return failed;
}
