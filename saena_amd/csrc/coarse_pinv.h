// The dense factorisations behind the direct coarsest solve (coarse_solver == 1), host only and free of the runtime: they take a
// dense row-major array, so a test compiles this header with g++ and holds it to its numpy restatement
// (tests/test_null_space_ref.py), and tools/sanitize_null_space.cpp runs its edges under ASan + UBSan.
//
//   gauss_jordan_inverse   inv = a^-1 by Gauss-Jordan on [a | I] with partial pivoting (the first largest |a| at or below the
//                          diagonal), the pivot row scaled by 1 / pivot; an exact-zero pivot is refused.  What sgpu_amg_create has
//                          always stored for a nonsingular coarsest operator.
//   pseudo_inverse         for a symmetric a with a 1 = 0 (the constant null space, sgpu_amg_create_null_space kind 1): the same
//                          elimination on a + (s / n) 1 1^T, s the mean of a's diagonal, then every column of the result has its mean
//                          taken off, then every row.  With z = 1 / sqrt(n): (a + s z z^T)^-1 = a^+ + z z^T / s, and the two
//                          centrings remove the second term (and what rounding put into the null space), so k_dense_solve applies
//                          a^+ with no change and no extra launch.  The shifted matrix is as well conditioned as a is on the
//                          complement of constants.  Every sum is sequential, in index order.
#pragma once
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace coarse_pinv {

// a: n x n row-major, destroyed; inv: n x n row-major.  false: an exact-zero pivot (a is singular); a and inv are then unspecified
inline bool gauss_jordan_inverse(std::vector<double> &a, int n, std::vector<double> &inv) {
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1.0;
    for (int c = 0; c < n; ++c) {
        int piv = c;
        for (int r = c + 1; r < n; ++r) if (std::fabs(a[(size_t)r * n + c]) > std::fabs(a[(size_t)piv * n + c])) piv = r;
        if (a[(size_t)piv * n + c] == 0.0) return false;
        if (piv != c) for (int j = 0; j < n; ++j) { std::swap(a[(size_t)piv * n + j], a[(size_t)c * n + j]); std::swap(inv[(size_t)piv * n + j], inv[(size_t)c * n + j]); }
        const double d = 1.0 / a[(size_t)c * n + c];
        for (int j = 0; j < n; ++j) { a[(size_t)c * n + j] *= d; inv[(size_t)c * n + j] *= d; }
        for (int r = 0; r < n; ++r) {
            if (r == c) continue;
            const double f = a[(size_t)r * n + c];
            if (f == 0.0) continue;
            for (int j = 0; j < n; ++j) { a[(size_t)r * n + j] -= f * a[(size_t)c * n + j]; inv[(size_t)r * n + j] -= f * inv[(size_t)c * n + j]; }
        }
    }
    return true;
}

// a: n x n row-major, symmetric with a 1 = 0, destroyed; pinv: n x n row-major.  false: the diagonal's mean is not positive (a zero
// matrix has no scale to shift by), or the shifted matrix met an exact-zero pivot
inline bool pseudo_inverse(std::vector<double> &a, int n, std::vector<double> &pinv) {
    if (n < 1) { pinv.clear(); return true; }
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += a[(size_t)i * n + i];
    const double s = tr / (double)n;
    if (!(s > 0.0)) return false;
    const double shift = s / (double)n;
    for (size_t k = 0; k < (size_t)n * n; ++k) a[k] += shift;
    if (!gauss_jordan_inverse(a, n, pinv)) return false;
    std::vector<double> m((size_t)n);
    for (int j = 0; j < n; ++j) m[j] = 0.0;
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) m[j] += pinv[(size_t)i * n + j];          // column sums, rows in order
    for (int j = 0; j < n; ++j) m[j] /= (double)n;
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) pinv[(size_t)i * n + j] -= m[j];
    for (int i = 0; i < n; ++i) {
        double r = 0.0;
        for (int j = 0; j < n; ++j) r += pinv[(size_t)i * n + j];                                     // row sum, columns in order
        r /= (double)n;
        for (int j = 0; j < n; ++j) pinv[(size_t)i * n + j] -= r;
    }
    return true;
}

} // namespace coarse_pinv
