// kernels_lanczos.hip.h -- the vector work of sgpu_op_eig_max (sgpu_lanczos.hip.inc): pure streaming (gfx950, wave64).
//
// The Lanczos recurrence of amg_hierarchy::find_eig (host/amg_setup.cpp) on D^-1/2 A D^-1/2, with the operator's own apply between
// the kernels below.  Per step:
//   t = isd .* v                      (k_lz_start before step 0, k_lz_shift afterwards)
//   w = A t                           (the runtime's apply, plain epilogue)
//   w = isd .* w, a = w . v           (k_lz_scale_dot + k_reduce_partials)
//   w -= a v + b vprev, b2 = w . w    (k_lz_update_dot + k_reduce_partials)
//   vnext = w / b, t = isd .* vnext   (k_lz_shift; vprev <- v is a rotation of the three buffers on the host, nothing is copied)
// Every product is rounded before it is added (-ffp-contract=off), in find_eig's order: a v + b vprev is formed, then subtracted.
//
// The two kernels that leave partial sums walk the rows with k_dot_partial's element-to-thread assignment -- thread t of block b
// owns the rows b * 256 + t + k * 256 * gridDim, one 8-byte element per thread and trip, a wave reads 512 contiguous bytes -- on
// k_dot_partial's grid, and k_reduce_partials adds the blocks' sums in a fixed order: the two scalars of a step depend on n and on
// the vectors alone, never on the run or the process.  No atomics.  Pairs of rows per thread would change that assignment, so the
// 16-byte accesses are kept for the two kernels without a sum (k_lz_start, k_lz_shift): every scratch vector comes from hipMalloc
// and is 16-byte aligned whatever n is; thread 0 of block 0 takes the last row of an odd n.
#pragma once
#include "kernels.hip.h"

namespace sk {

// isd = sqrt(|inv_diag|), t = isd .* v  (IEEE sqrt: the host forms the same isd)
__global__ __launch_bounds__(BLOCK) void k_lz_start(const double *__restrict__ inv_diag, const double *__restrict__ v, double *__restrict__ isd,
                                                    double *__restrict__ t, size_t n) {
    const size_t stride = (size_t)gridDim.x * BLOCK, n2 = n >> 1;
    for (size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x; p < n2; p += stride) {
        const sk_d2v dg = *reinterpret_cast<const sk_d2v *>(inv_diag + 2 * p), vv = *reinterpret_cast<const sk_d2v *>(v + 2 * p);
        sk_d2v s, o;
        s.x = sqrt(fabs(dg.x)); s.y = sqrt(fabs(dg.y));
        o.x = s.x * vv.x; o.y = s.y * vv.y;
        *reinterpret_cast<sk_d2v *>(isd + 2 * p) = s;
        *reinterpret_cast<sk_d2v *>(t + 2 * p) = o;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double s = sqrt(fabs(inv_diag[n - 1]));
        isd[n - 1] = s;
        t[n - 1] = s * v[n - 1];
    }
}

// w = isd .* w; partial[block] = this block's share of the NEW w . v (launch it with the dot's grid)
__global__ __launch_bounds__(BLOCK) void k_lz_scale_dot(const double *__restrict__ isd, const double *__restrict__ v, double *__restrict__ w, size_t n,
                                                        double *__restrict__ partial) {
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const double wi = w[i] * isd[i];
        w[i] = wi;
        s += wi * v[i];
    }
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// w -= a v + b vprev with a = S[0] (the device scalar k_reduce_partials left) and b from the host; partial[block] = this block's
// share of the NEW w . w (launch it with the dot's grid)
__global__ __launch_bounds__(BLOCK) void k_lz_update_dot(const double *__restrict__ S, double b, const double *__restrict__ v,
                                                         const double *__restrict__ vprev, double *__restrict__ w, size_t n,
                                                         double *__restrict__ partial) {
    __shared__ double sh[BLOCK / 64];
    const double a = S[0];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const double wi = w[i] - (a * v[i] + b * vprev[i]);
        w[i] = wi;
        s += wi * wi;
    }
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// vnext = w / b (IEEE division), t = isd .* vnext
__global__ __launch_bounds__(BLOCK) void k_lz_shift(const double *__restrict__ w, double b, const double *__restrict__ isd, double *__restrict__ vnext,
                                                    double *__restrict__ t, size_t n) {
    const size_t stride = (size_t)gridDim.x * BLOCK, n2 = n >> 1;
    for (size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x; p < n2; p += stride) {
        const sk_d2v wv = *reinterpret_cast<const sk_d2v *>(w + 2 * p), s = *reinterpret_cast<const sk_d2v *>(isd + 2 * p);
        sk_d2v vn, o;
        vn.x = wv.x / b; vn.y = wv.y / b;
        o.x = s.x * vn.x; o.y = s.y * vn.y;
        *reinterpret_cast<sk_d2v *>(vnext + 2 * p) = vn;
        *reinterpret_cast<sk_d2v *>(t + 2 * p) = o;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double vn = w[n - 1] / b;
        vnext[n - 1] = vn;
        t[n - 1] = isd[n - 1] * vn;
    }
}

} // namespace sk
