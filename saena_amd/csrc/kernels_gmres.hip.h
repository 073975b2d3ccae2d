// kernels_gmres.hip.h -- the orthogonalisation of restarted flexible GMRES (sgpu_gmres.hip.inc): pure vector streaming (gfx950, wave64).
//
// The Krylov basis V and the preconditioned vectors Z are column-major device arrays, column c at V + c * ld; ld is even, so every
// column starts on a 16-byte boundary whatever n is.  One Gram-Schmidt step is two kernels over the same C <= GS_C columns:
//   * k_gs_dots_partial: h[c] = V[:,c] . w for the C columns in ONE pass -- w is read once, C accumulators per thread;
//   * k_gs_update:       w -= sum_c h[c] V[:,c], ascending c, each product rounded, then subtracted (-ffp-contract=off).
// Both walk the rows in PAIRS with 16-byte loads and stores: thread t of block b owns the pairs b * 256 + t + k * 256 * gridDim
// (k = 0, 1, ...), the grid is min(GS_MAXBLK, ceil((n / 2) / 256)) blocks, and thread 0 of block 0 takes the last row of an odd n
// after its pairs.  The row -> thread map depends on n alone: a column's dot does not depend on how many columns ride with it,
// and the update's running value continues from chunk to chunk of columns, so the result does not depend on the chunking.
// Reductions are k_dot_partial's two stages: block_sum per workgroup into partial[c * GS_MAXBLK + block], then one workgroup
// per column adds the partials in a fixed order (k_gs_reduce).  No atomics, no LDS beyond block_sum's four doubles.
// The column count of a launch is a TEMPLATE parameter, 1 .. GS_C: with a run-time count every column's load sits behind its own
// branch and the compiler issues them one after the other (the register report showed 36 / 18 VGPRs for the dots / the update:
// no room for eight 16-byte loads in flight); with the count known all C + 1 loads of a trip are issued before the first is used.
#pragma once
#include "kernels.hip.h"

namespace sk {

constexpr int GS_C = 8;            // columns per pass
constexpr int GS_MAXBLK = 1024;    // most blocks of a pass, and the stride of a column's partial sums

// partial[c * GS_MAXBLK + block] = this block's share of V[:,c] . w, c < C
template <int C>
__global__ __launch_bounds__(BLOCK) void k_gs_dots_partial(const double *__restrict__ V, size_t ld, const double *__restrict__ w, size_t n,
                                                           double *__restrict__ partial) {
    static_assert(C >= 1 && C <= GS_C, "C");
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK, n2 = n >> 1;
    double s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0.0;
    for (size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x; p < n2; p += stride) {
        const sk_d2v wv = *reinterpret_cast<const sk_d2v *>(w + 2 * p);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const sk_d2v v = *reinterpret_cast<const sk_d2v *>(V + (size_t)c * ld + 2 * p);
            s[c] += v.x * wv.x;
            s[c] += v.y * wv.y;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double wl = w[n - 1];
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] += V[(size_t)c * ld + n - 1] * wl;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double t = block_sum(s[c], sh);
        if (threadIdx.x == 0) partial[(size_t)c * GS_MAXBLK + blockIdx.x] = t;
    }
}

// out[c] = sum over the np blocks of partial[c * GS_MAXBLK + block]: one workgroup per column, k_reduce_partials' order
__global__ __launch_bounds__(BLOCK) void k_gs_reduce(const double *__restrict__ partial, int np, double *__restrict__ out) {
    __shared__ double sh[BLOCK / 64];
    const double *pc = partial + (size_t)blockIdx.x * GS_MAXBLK;
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += BLOCK) s += pc[i];
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// w -= sum_{c < C} h[c] V[:,c] in ascending c, the coefficients read from device memory.  NORM: partial[block] = this block's
// share of the NEW w . w with the dots' row -> thread map (launch it on the dots' grid; k_gs_reduce with one workgroup finishes it).
// With the coefficients negated it is u += Z y.
template <int C, bool NORM>
__global__ __launch_bounds__(BLOCK) void k_gs_update(const double *__restrict__ V, size_t ld, const double *__restrict__ h, double *__restrict__ w,
                                                     size_t n, double *__restrict__ partial) {
    static_assert(C >= 1 && C <= GS_C, "C");
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK, n2 = n >> 1;
    double hc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) hc[c] = h[c];
    double s = 0.0;
    for (size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x; p < n2; p += stride) {
        sk_d2v wv = *reinterpret_cast<const sk_d2v *>(w + 2 * p);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const sk_d2v v = *reinterpret_cast<const sk_d2v *>(V + (size_t)c * ld + 2 * p);
            wv.x = wv.x - hc[c] * v.x;
            wv.y = wv.y - hc[c] * v.y;
        }
        *reinterpret_cast<sk_d2v *>(w + 2 * p) = wv;
        if constexpr (NORM) { s += wv.x * wv.x; s += wv.y * wv.y; }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double wl = w[n - 1];
#pragma unroll
        for (int c = 0; c < C; ++c) wl = wl - hc[c] * V[(size_t)c * ld + n - 1];
        w[n - 1] = wl;
        if constexpr (NORM) s += wl * wl;
    }
    if constexpr (NORM) {
        const double t = block_sum(s, sh);
        if (threadIdx.x == 0) partial[blockIdx.x] = t;
    }
}

// v = w / sqrt(nrm2[0]), the scalar read from device memory (IEEE sqrt and division: the host forms the same value); v may be w
__global__ __launch_bounds__(BLOCK) void k_gs_scale(const double *__restrict__ nrm2, const double *w, double *v, size_t n) {
    const double d = sqrt(nrm2[0]);
    const size_t stride = (size_t)gridDim.x * BLOCK, n2 = n >> 1;
    for (size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x; p < n2; p += stride) {
        sk_d2v wv = *reinterpret_cast<const sk_d2v *>(w + 2 * p);
        wv.x = wv.x / d;
        wv.y = wv.y / d;
        *reinterpret_cast<sk_d2v *>(v + 2 * p) = wv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) v[n - 1] = w[n - 1] / d;
}

} // namespace sk
