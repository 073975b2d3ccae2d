// eigs_device.h -- what saena_amg_eigs (saena_c_api.cpp) and saena::amg::eigs (saena.cpp) share: the default start vectors and the
// trip of column-major host arrays through sgpu_eigs_LOBPCG, or -- with a second operator B -- through sgpu_eigs_LOBPCG_gen
// (saena_amg_eigs_gen, saena::amg::eigs_gen).
#pragma once
#include "../../../include/saena_gpu.h"

#include <cmath>
#include <cstddef>
#include <vector>

namespace saena_host {

// out: column-major n x K; column j is find_eig's LCG sequence over the row index, in (-1, 1), from a seed of its own
inline void default_eig_start(size_t n, int K, value_t *out) {
    for (int j = 0; j < K; ++j) {
        unsigned long long lcg = 88172645463325252ULL + 0x9E3779B97F4A7C15ULL * (unsigned long long)j;
        for (size_t i = 0; i < n; ++i) {
            lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
            out[(size_t)j * n + i] = ((lcg >> 11) * (1.0 / 9007199254740992.0)) * 2.0 - 1.0;
        }
    }
}

#ifdef SAENA_WITH_GPU
// x0_host (column-major n x K, or null for the default start) up, packed into a block vector, sgpu_eigs_LOBPCG (B null: A x = lambda x)
// or sgpu_eigs_LOBPCG_gen (A x = lambda B x), and the eigenvectors back into x_host the same way.
// -> the sgpu status (SGPU_ERR_NOCONV: the outputs are written all the same; sgpu_last_error has the text)
inline int eigs_host_arrays(sgpu_amg *h, size_t n, const value_t *x0_host, int K, int nev, int max_iter, value_t tol, int precond,
                            value_t *lambda, value_t *x_host, value_t *res, int *iters, sgpu_op *B = nullptr) {
    std::vector<value_t> start;
    if (!x0_host) {
        start.resize(n * (size_t)K);
        default_eig_start(n, K, start.data());
        x0_host = start.data();
    }
    value_t *cm = nullptr, *x = nullptr;
    int s = sgpu_vec_alloc(&cm, n * K);
    if (s == SGPU_OK) s = sgpu_vec_alloc(&x, n * K);
    if (s == SGPU_OK) s = sgpu_vec_upload(cm, x0_host, n * K);
    if (s == SGPU_OK) s = sgpu_block_pack(cm, x, n, K);
    // a hierarchy that knows the constant null space (set_null_space("constant")): lambda = 0 belongs to the spectrum, so the standard
    // problem is solved with the normalised constant vector locked -- the nev smallest NONZERO pairs, the first of them the Fiedler
    // vector.  The generalised problem passes the library's refusal through
    int kind = 0;
    if (s == SGPU_OK) s = sgpu_amg_get_null_space(h, &kind);
    if (s == SGPU_OK && kind == 1 && !B && n > 0) {
        value_t *q = nullptr;
        const size_t ld = n + (n & 1);
        s = sgpu_vec_alloc(&q, ld);
        if (s == SGPU_OK) s = sgpu_vec_fill(q, 1.0 / std::sqrt((value_t)n), ld);
        if (s == SGPU_OK) s = sgpu_eigs_LOBPCG_locked(h, nullptr, q, nullptr, ld, 1, x, K, nev, max_iter, tol, precond, lambda, res, iters, nullptr, 0, nullptr);
        if (q) sgpu_vec_free(q);
    } else if (s == SGPU_OK)
        s = B ? sgpu_eigs_LOBPCG_gen(h, B, x, K, nev, max_iter, tol, precond, lambda, res, iters, nullptr, 0)
              : sgpu_eigs_LOBPCG(h, x, K, nev, max_iter, tol, precond, lambda, res, iters, nullptr, 0);
    if (s == SGPU_OK || s == SGPU_ERR_NOCONV) {
        int s2 = sgpu_block_unpack(x, cm, n, K);
        if (s2 == SGPU_OK) s2 = sgpu_vec_download(x_host, cm, n * K);
        if (s2 != SGPU_OK) s = s2;
    }
    sgpu_vec_free(cm); sgpu_vec_free(x);
    return s;
}

// what saena_amg_eigs_many and saena::amg::eigs_many share: x0_host (column-major n x K, or null: the driver generates its start block
// on the device) up and packed, sgpu_eigs_LOBPCG_many on a device Q of nev columns (leading dimension n rounded up to even), and the
// *nlocked columns it locked back into q_host (column-major n x nev; the columns past *nlocked are not written).
// -> the sgpu status (SGPU_ERR_NOCONV: lambda, res and q_host hold the *nlocked pairs locked so far)
inline int eigs_many_host_arrays(sgpu_amg *h, size_t n, sgpu_op *B, int nev, int K, int sweep_nev, const value_t *x0_host, int max_iter, value_t tol,
                                 int precond, value_t *lambda, value_t *q_host, value_t *res, int *iters, int *nlocked, int *sweeps) {
    const size_t ld = n + (n & 1);
    int locked = 0;
    value_t *cm = nullptr, *x = nullptr, *q = nullptr;
    int s = sgpu_vec_alloc(&q, ld * (size_t)(nev > 0 ? nev : 1));
    if (s == SGPU_OK && x0_host && (K == 2 || K == 4 || K == 8)) {
        s = sgpu_vec_alloc(&cm, n * K);
        if (s == SGPU_OK) s = sgpu_vec_alloc(&x, n * K);
        if (s == SGPU_OK) s = sgpu_vec_upload(cm, x0_host, n * K);
        if (s == SGPU_OK) s = sgpu_block_pack(cm, x, n, K);
    }
    if (s == SGPU_OK) s = sgpu_eigs_LOBPCG_many(h, B, q, ld, nev, K, sweep_nev, x, max_iter, tol, precond, lambda, res, iters, &locked, sweeps);
    if (s == SGPU_OK || s == SGPU_ERR_NOCONV)
        for (int l = 0; l < locked; ++l) {
            const int s2 = sgpu_vec_download(q_host + (size_t)l * n, q + (size_t)l * ld, n);
            if (s2 != SGPU_OK) { s = s2; break; }
        }
    if (nlocked) *nlocked = locked;
    sgpu_vec_free(cm); sgpu_vec_free(x); sgpu_vec_free(q);
    return s;
}
#endif

} // namespace saena_host
