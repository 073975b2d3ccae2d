// kernels_eig.hip.h -- the tall-skinny kernels of sgpu_eigs_LOBPCG (sgpu_eig.hip.inc) on block vectors X[i * K + j], K in
// {2, 4, 8}, 16-byte aligned (gfx950, wave64).  Products are rounded, then added (-ffp-contract=off); no atomics, no scratch;
// a row of a block vector is read and written with K / 2 16-byte accesses.
//   * k_gram_block_partial<K> + k_gram_reduce: G[a][b] = sum_i X[i, a] Y[i, b], all K^2 entries from ONE read of X and Y.
//     Contract: entry (a, b) has the bits of sgpu_dot on column a of X and column b of Y -- row i goes to the thread
//     k_dot_partial gives element i, a thread adds its rows in order of its grid-stride trips, block_sum, then one workgroup per
//     entry adds the blocks' partial sums the way k_reduce_partials does.  An entry therefore depends on neither K nor (a, b),
//     and X == Y gives a bit-symmetric result (a product commutes).  The whole K x K tile lives in one lane: 64 fp64
//     accumulators at K = 8 (DESIGN.md section 12 has the register table).
//   * k_block_mix<K, NS>: Out[i, b] = sum_{s < NS} sum_{a ascending} S_s[i, a] C_s[a, b] (+ Add[i, b], last, when Add is given);
//     the sum starts from 0.0 in exactly that order.  The K x K coefficient matrices come from device memory and are staged in
//     LDS (NS K^2 doubles: too many for registers at K = 8, NS = 3), read back as broadcasts.  Row-local: Out may alias any
//     source and Add.  It serves the Rayleigh-Ritz updates, both orthonormalisation steps and the start-up rotation.
//   * k_eig_residual<K>: R = AX - X diag(lambda), lambda from device memory, and the partial sums of ||r_j||^2 in the same pass,
//     in k_dot_block_partial's order (reduce with k_reduce_partials_block): the norms have the bits of the block dot of R with itself.
//   * k_geig_residual<K>: the same for A x = lambda B x (sgpu_eigs_LOBPCG_gen): R = AX - BX diag(lambda), and ||r_j||^2 and
//     ||(BX)_j||^2 from one pass.
#pragma once
#include "kernels_block.hip.h"

namespace sk {

template <int K>
__device__ __forceinline__ void block_load_row(const double *p, size_t i, double (&v)[K]) {
#pragma unroll
    for (int h = 0; h < K / 2; ++h) {
        const sk_d2v t = *reinterpret_cast<const sk_d2v *>(p + i * K + 2 * h);
        v[2 * h] = t.x; v[2 * h + 1] = t.y;
    }
}
template <int K>
__device__ __forceinline__ void block_store_row(double *p, size_t i, const double (&v)[K]) {
#pragma unroll
    for (int h = 0; h < K / 2; ++h) {
        sk_d2v t; t.x = v[2 * h]; t.y = v[2 * h + 1];
        *reinterpret_cast<sk_d2v *>(p + i * K + 2 * h) = t;
    }
}

// partial[(block * K + a) * K + b] = the block's share of X_a . Y_b; launch it on the dot's grid (X may be Y)
template <int K>
__global__ __launch_bounds__(BLOCK) void k_gram_block_partial(const double *x, const double *y, size_t n, double *__restrict__ partial) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double s[K][K];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) s[a][b] = 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        double xv[K], yv[K];
        block_load_row<K>(x, i, xv);
        block_load_row<K>(y, i, yv);
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = 0; b < K; ++b) s[a][b] += xv[a] * yv[b];
    }
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const double t = block_sum(s[a][b], sh);
            if (threadIdx.x == 0) partial[((size_t)blockIdx.x * K + a) * K + b] = t;
        }
}

// out[slot * ne + e] = sum over the np blocks of partial[slot * slot_stride + block * ne + e]: one workgroup per entry (blockIdx.x =
// slot * ne + e), k_reduce_partials' order
__global__ __launch_bounds__(BLOCK) void k_gram_reduce(const double *__restrict__ partial, int np, int ne, size_t slot_stride, double *__restrict__ out) {
    __shared__ double sh[BLOCK / 64];
    const int slot = blockIdx.x / ne, e = blockIdx.x % ne;
    const double *p = partial + (size_t)slot * slot_stride;
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += BLOCK) s += p[(size_t)i * ne + e];
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

template <int K, int NS>
__global__ __launch_bounds__(BLOCK) void k_block_mix(const double *s0, const double *c0, const double *s1, const double *c1, const double *s2,
                                                     const double *c2, const double *add, double *out, size_t n) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    static_assert(NS >= 1 && NS <= 3, "NS");
    constexpr int KK = K * K;
    __shared__ __attribute__((aligned(16))) double lc[NS * KK];
    for (int t = threadIdx.x; t < NS * KK; t += BLOCK) lc[t] = (t < KK ? c0 : t < 2 * KK ? c1 : c2)[t % KK];
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        double acc[K], v[K];
        int z = 0;
        asm volatile("" : "+v"(z));               // opaque per row: the NS K^2 coefficient reads stay LDS reads inside the loop (hoisted, they
                                                  // take up to 384 registers at K = 8 and leave one wave per SIMD)
#pragma unroll
        for (int b = 0; b < K; ++b) acc[b] = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            block_load_row<K>(s == 0 ? s0 : s == 1 ? s1 : s2, i, v);
#pragma unroll
            for (int a = 0; a < K; ++a)
#pragma unroll
                for (int b = 0; b < K; ++b) acc[b] += v[a] * lc[z + s * KK + a * K + b];
        }
        if (add) {
            block_load_row<K>(add, i, v);
#pragma unroll
            for (int b = 0; b < K; ++b) acc[b] += v[b];
        }
        block_store_row<K>(out, i, acc);
    }
}

// launch it on the dot's grid; partial[block * K + j]
template <int K>
__global__ __launch_bounds__(BLOCK) void k_eig_residual(const double *__restrict__ ax, const double *__restrict__ x, const double *__restrict__ lambda,
                                                        double *__restrict__ r, size_t n, double *__restrict__ partial) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double lam[K], s[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { lam[j] = lambda[j]; s[j] = 0.0; }
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        double av[K], xv[K];
        block_load_row<K>(ax, i, av);
        block_load_row<K>(x, i, xv);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            av[j] = av[j] - xv[j] * lam[j];
            s[j] += av[j] * av[j];
        }
        block_store_row<K>(r, i, av);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double t = block_sum(s[j], sh);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * K + j] = t;
    }
}

// the residual of the generalised problem (sgpu_eig.hip.inc): R = AX - BX diag(lambda) with the bits of k_eig_residual called with
// BX in X's place, and in the same pass the partial sums of ||r_j||^2 (partial_r) AND of ||(BX)_j||^2 (partial_b), both in
// k_dot_block_partial's order: the bits of the block dot of R with R and of BX with BX.  Launch it on the dot's grid;
// partial_*[block * K + j].  It moves 24 n K bytes (two block vectors read, one written).
template <int K>
__global__ __launch_bounds__(BLOCK) void k_geig_residual(const double *__restrict__ ax, const double *__restrict__ bx, const double *__restrict__ lambda,
                                                         double *__restrict__ r, size_t n, double *__restrict__ partial_r, double *__restrict__ partial_b) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double lam[K], s[K], sb[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { lam[j] = lambda[j]; s[j] = 0.0; sb[j] = 0.0; }
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        double av[K], bv[K];
        block_load_row<K>(ax, i, av);
        block_load_row<K>(bx, i, bv);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            av[j] = av[j] - bv[j] * lam[j];
            s[j] += av[j] * av[j];
            sb[j] += bv[j] * bv[j];
        }
        block_store_row<K>(r, i, av);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double t = block_sum(s[j], sh);
        if (threadIdx.x == 0) partial_r[(size_t)blockIdx.x * K + j] = t;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double t = block_sum(sb[j], sh);
        if (threadIdx.x == 0) partial_b[(size_t)blockIdx.x * K + j] = t;
    }
}

} // namespace sk
