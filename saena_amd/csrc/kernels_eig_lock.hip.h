// kernels_eig_lock.hip.h -- the kernels hard locking adds to LOBPCG (sgpu_eig_lock.hip.inc): a block vector Y[i * K + b], K in
// {2, 4, 8}, against up to LOCK_MAX locked vectors (gfx950, wave64).  The locked set is COLUMN-MAJOR, column l at Q + l * ld, ld >= n
// and even (kernels_gmres.hip.h's convention: every column starts on a 16-byte boundary); block vectors are interleaved as everywhere
// else.  The house rules of kernels_eig.hip.h hold: products rounded, then added (-ffp-contract=off); no atomics; no scratch; a row
// of a block vector is read and written with K / 2 16-byte accesses (a lane reads ONE double of each locked column per row -- a wave
// reads 512 contiguous bytes of the column).
//   * k_lock_gram_partial<K, C> + k_gram_reduce: C[l][b] = sum_i Z[i, l] Y[i, b] for the C <= LOCK_C columns of one pass, from ONE
//     read of Y; C K accumulators in one lane (64 at K = 8, C = 8: k_gram_block_partial<8>'s register picture).  C is a template
//     parameter, as in k_gs_dots_partial: all C + K / 2 loads of a trip are issued before the first use.
//     Contract: entry (l, b) has the bits of k_gram_block_partial's entry for the same two columns -- the same row -> thread map
//     (launch it on the dot's grid), the same grid-stride trips, block_sum, and k_gram_reduce adds the blocks' partial sums.  An
//     entry therefore depends on neither L, K, the pass its column fell in, nor (l, b).
//     partial[(block * LOCK_C + c) * K + b]: a pass owns n_partials * LOCK_C * K doubles whatever C is, so that ONE k_gram_reduce
//     launch of L K workgroups (ne = LOCK_C K, a slot per pass) writes C[l][b] at out[l * K + b].
//   * k_lock_project<K>: W[i, b] <- (sum_{l ascending} Q[i, l] (-C[l][b]), from 0.0) + W[i, b], W added last: k_block_mix's order
//     with its Add operand.  C (at most LOCK_MAX K doubles, 4 KiB) is read from device memory, negated (exact), staged in LDS and read
//     back as broadcasts; the columns are walked LOCK_C at a time, the loads of a chunk issued together.  Row-local and in place.
//     One pass moves 8 n (L + 2 K) bytes.
//   * k_block_refill: column `col` of a block vector from the deterministic generator lock_hash(row, counter), exact in [-1, 1).
//   * k_block_col_get: column `col` of a block vector into a contiguous array (a locked column).
#pragma once
#include "kernels_eig.hip.h"

namespace sk {

constexpr int LOCK_C = 8;        // locked columns per Gram pass, and per chunk of the projection
constexpr int LOCK_MAX = 64;     // most locked columns

template <int K, int C>
__global__ __launch_bounds__(BLOCK) void k_lock_gram_partial(const double *__restrict__ z, size_t ld, const double *__restrict__ y, size_t n,
                                                             double *__restrict__ partial) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    static_assert(C >= 1 && C <= LOCK_C, "C");
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double s[C][K];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int b = 0; b < K; ++b) s[c][b] = 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        double zv[C], yv[K];
        block_load_row<K>(y, i, yv);
#pragma unroll
        for (int c = 0; c < C; ++c) zv[c] = z[(size_t)c * ld + i];
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int b = 0; b < K; ++b) s[c][b] += zv[c] * yv[b];
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const double t = block_sum(s[c][b], sh);
            if (threadIdx.x == 0) partial[((size_t)blockIdx.x * LOCK_C + c) * K + b] = t;
        }
}

// acc[b] += sum_{c < C ascending} q[c * ld + i] * lc[c * K + b]: the C loads first, then the products
template <int K, int C>
__device__ __forceinline__ void lock_chunk(const double *__restrict__ q, size_t ld, size_t i, const double *lc, double (&acc)[K]) {
    double qv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) qv[c] = q[(size_t)c * ld + i];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int b = 0; b < K; ++b) acc[b] += qv[c] * lc[c * K + b];
}

template <int K>
__global__ __launch_bounds__(BLOCK) void k_lock_project(const double *__restrict__ q, size_t ld, const double *__restrict__ coef, int L, double *w,
                                                        size_t n) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    __shared__ __attribute__((aligned(16))) double lc[LOCK_MAX * K];
    for (int t = threadIdx.x; t < L * K; t += BLOCK) lc[t] = -coef[t];
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * BLOCK;
    const int full = L / LOCK_C * LOCK_C, tail = L - full;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        double acc[K], v[K];
#pragma unroll
        for (int b = 0; b < K; ++b) acc[b] = 0.0;
        block_load_row<K>(w, i, v);
        for (int l = 0; l < full; l += LOCK_C) lock_chunk<K, LOCK_C>(q + (size_t)l * ld, ld, i, lc + l * K, acc);
        const double *qt = q + (size_t)full * ld, *lt = lc + full * K;
        switch (tail) {
        case 1: lock_chunk<K, 1>(qt, ld, i, lt, acc); break;
        case 2: lock_chunk<K, 2>(qt, ld, i, lt, acc); break;
        case 3: lock_chunk<K, 3>(qt, ld, i, lt, acc); break;
        case 4: lock_chunk<K, 4>(qt, ld, i, lt, acc); break;
        case 5: lock_chunk<K, 5>(qt, ld, i, lt, acc); break;
        case 6: lock_chunk<K, 6>(qt, ld, i, lt, acc); break;
        case 7: lock_chunk<K, 7>(qt, ld, i, lt, acc); break;
        default: break;
        }
#pragma unroll
        for (int b = 0; b < K; ++b) acc[b] += v[b];
        block_store_row<K>(w, i, acc);
    }
}

// the refill generator: a 64-bit mix (splitmix64's finaliser) of the row and a running column counter; its top 53 bits, as an
// integer below 2^53, times 2^-52, minus 1: every step exact, the value in [-1, 1)
__host__ __device__ inline double lock_hash(unsigned long long row, unsigned int counter) {
    unsigned long long z = row * 0x9E3779B97F4A7C15ull + ((unsigned long long)counter + 1ull) * 0xD1B54A32D192ED03ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(long long)(z >> 11) * 0x1p-52 - 1.0;
}

__global__ __launch_bounds__(BLOCK) void k_block_refill(double *__restrict__ x, size_t n, int K, int col, unsigned int counter) {
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) x[i * K + col] = lock_hash(i, counter);
}

__global__ __launch_bounds__(BLOCK) void k_block_col_get(const double *__restrict__ x, size_t n, int K, int col, double *__restrict__ dst) {
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) dst[i] = x[i * K + col];
}

} // namespace sk
