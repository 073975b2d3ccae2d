// dense_eig.cpp -- see dense_eig.h
#include "dense_eig.h"
#include "../../../include/saena_c.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <numeric>
#include <vector>

namespace saena_host {

bool dense_cholesky(int n, const double *A, double *L) {
    const double rel = 256.0 * n * DBL_EPSILON;
    std::fill(L, L + (size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        const double ajj = A[(size_t)j * n + j];
        if (!(ajj > 0.0) || !std::isfinite(ajj)) return false;
        double d = ajj;
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > rel * ajj)) return false;
        const double ljj = std::sqrt(d);
        L[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double s = A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            s /= ljj;
            if (!std::isfinite(s)) return false;
            L[(size_t)i * n + j] = s;
        }
    }
    return true;
}

void dense_inv_lower_transposed(int n, const double *L, double *T) {
    // column c of L^-1 by forward substitution, stored as row c of T = (L^-1)^T
    std::fill(T, T + (size_t)n * n, 0.0);
    for (int c = 0; c < n; ++c)
        for (int i = c; i < n; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= L[(size_t)i * n + k] * T[(size_t)c * n + k];
            T[(size_t)c * n + i] = s / L[(size_t)i * n + i];
        }
}

int dense_sym_eig(int n, const double *A, double *w, double *V) {
    std::vector<double> a(A, A + (size_t)n * n), v((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
    double fro = 0.0;
    for (double x : a) { if (!std::isfinite(x)) return -1; fro += x * x; }
    const double floor_abs = DBL_EPSILON * DBL_EPSILON * std::sqrt(fro);
    int sweeps = 0;
    for (;; ++sweeps) {
        bool rotated = false;
        if (sweeps == JACOBI_MAX_SWEEPS) {
            for (int i = 0; i < n && !rotated; ++i)
                for (int j = i + 1; j < n; ++j) {
                    const double x = std::fabs(a[(size_t)i * n + j]);
                    if (x > floor_abs && x > DBL_EPSILON * std::sqrt(std::fabs(a[(size_t)i * n + i] * a[(size_t)j * n + j]))) { rotated = true; break; }
                }
            if (rotated) return -1;
            break;
        }
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q], app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q];
                if (std::fabs(apq) <= floor_abs || std::fabs(apq) <= DBL_EPSILON * std::sqrt(std::fabs(app * aqq))) continue;
                rotated = true;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {                  // columns p, q
                    const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
                    a[(size_t)k * n + p] = c * akp - s * akq;
                    a[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {                  // rows p, q
                    const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
                    a[(size_t)p * n + k] = c * apk - s * aqk;
                    a[(size_t)q * n + k] = s * apk + c * aqk;
                }
                a[(size_t)p * n + q] = 0.0; a[(size_t)q * n + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = c * vkp - s * vkq;
                    v[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
        if (!rotated) break;
    }
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * n + x] < a[(size_t)y * n + y]; });
    for (int k = 0; k < n; ++k) {
        w[k] = a[(size_t)order[(size_t)k] * n + order[(size_t)k]];
        for (int i = 0; i < n; ++i) V[(size_t)i * n + k] = v[(size_t)i * n + order[(size_t)k]];
    }
    return sweeps;
}

int dense_sym_geig(int n, const double *A, const double *B, double *w, double *V) {
    if (n < 1 || n > DENSE_EIG_MAXN) return -3;
    const size_t nn = (size_t)n * n;
    std::vector<double> L(nn), T(nn), C(nn), M(nn), Q(nn);
    if (!dense_cholesky(n, B, L.data())) return -1;
    dense_inv_lower_transposed(n, L.data(), T.data());       // T = L^-T, upper triangular
    // M = A T, C = T^T M = L^-1 A L^-T, symmetrised
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k <= j; ++k) s += A[(size_t)i * n + k] * T[(size_t)k * n + j];
            M[(size_t)i * n + j] = s;
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k <= i; ++k) s += T[(size_t)k * n + i] * M[(size_t)k * n + j];
            C[(size_t)i * n + j] = s;
        }
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double s = 0.5 * (C[(size_t)i * n + j] + C[(size_t)j * n + i]);
            C[(size_t)i * n + j] = s; C[(size_t)j * n + i] = s;
        }
    const int sweeps = dense_sym_eig(n, C.data(), w, Q.data());
    if (sweeps < 0) return -2;
    for (int i = 0; i < n; ++i)                               // V = T Q
        for (int k = 0; k < n; ++k) {
            double s = 0.0;
            for (int j = i; j < n; ++j) s += T[(size_t)i * n + j] * Q[(size_t)j * n + k];
            V[(size_t)i * n + k] = s;
        }
    return sweeps;
}

} // namespace saena_host

extern "C" {

static thread_local int g_geig_sweeps = 0;

int saena_debug_sym_geig(int n, const double *A, const double *B, double *w, double *V) {
    if (!A || !B || !w || !V) return -4;
    const int s = saena_host::dense_sym_geig(n, A, B, w, V);
    g_geig_sweeps = s > 0 ? s : 0;
    return s < 0 ? s : 0;
}

int saena_debug_sym_geig_sweeps(void) { return g_geig_sweeps; }

} // extern "C"
