// kernels_coarse_cg.hip.h -- the device-resident coarsest CG (sgpu_coarse_cg.hip.inc; sgpu_amg_params.coarse_solver = 2) for a
// coarsest level of more than CG_MAXN rows (gfx950, wave64).
//
// solve_coarsest_CG's recurrence, step for step as k_coarse_cg (kernels.hip.h) states it, with the vectors in HBM and every scalar in
// device memory.  The host enqueues a FIXED sequence -- 2 + 3 (max_iter - 1) launches whatever the data -- and reads nothing back, so
// the sequence sits inside a captured graph:
//   k_dcg_start    res = dir = rhs; PR[block] = partial sums of rhs . rhs
//   k_dcg_setup    (one workgroup) dot = sum PR; thres = dot tol tol; stop if dot < tol tol; iters = 1
//   iteration it = 1 .. max_iter - 1:
//     k_dcg_matvec   mt = A dir over the plain CSR arrays, G lanes per row; PA[block] = partial sums of dir . mt
//     k_dcg_update   factor = dot / sum PA; u += factor dir; res -= factor mt; PR[block] = partial sums of the new res . res
//     k_dcg_dir      dot' = sum PR; stop if dot' < thres; else dir = res + (dot' / dot) dir, iters = it + 1 (the cap: it)
//
// Launch boundaries are the only synchronisation: no atomics, no grid barrier, no cooperative launch, no spin.  What makes that enough:
//   * a sum over partials is formed by EVERY workgroup that needs it, in k_reduce_partials' order (thread t adds partials t, t + 256, ...,
//     then block_sum), so all workgroups of a launch hold the same bits of factor / dot' without one of them publishing it;
//   * no workgroup reads a scalar that a workgroup of the SAME launch writes.  dot lives in two slots by iteration parity: the kernels
//     of iteration `it` read S[DCG_DOT + (it & 1)], k_dcg_dir's block 0 writes the other one.  The stop flag is two words: F[DCG_STOP] is
//     written by k_dcg_dir (and k_dcg_setup) and read by k_dcg_matvec and k_dcg_update; F[DCG_STOP_DIR] is what k_dcg_dir itself reads, and
//     it is written by block 0 of the NEXT k_dcg_matvec, once;
//   * once its flag is set a kernel returns before it touches a vector, a partial sum or a scalar: the remaining launches of the
//     sequence cost a launch each.  (This is why the product is a kernel of its own and not the operator's tuned form: that form
//     cannot be told to stop.)
// Every product is rounded before it is added (-ffp-contract=off).  The partial sums of res . res follow k_dot_partial's
// element-to-thread assignment on k_dot_partial's grid; those of dir . mt follow the product's row-to-lane assignment (the lane that
// writes row r adds dir[r] mt[r]).  Both depend on n, G and the grid alone: two runs give the same bits.
#pragma once
#include "kernels.hip.h"

namespace sk {

enum { DCG_THRES = 0, DCG_DOT = 1, DCG_NSCALAR = 4 };             // S: thres | dot[2] | (pad)
enum { DCG_STOP = 0, DCG_STOP_DIR = 1, DCG_ITERS = 2, DCG_NFLAG = 4 };   // F (ints): the two stop words | the iteration count

// sum(partial[0..np)) in k_reduce_partials' order, returned to every thread of the workgroup
__device__ __forceinline__ double dcg_sum_all(const double *__restrict__ partial, int np, double *sh, double *bc) {
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += BLOCK) s += partial[i];
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) *bc = t;
    __syncthreads();
    return *bc;
}

__global__ __launch_bounds__(BLOCK) void k_dcg_start(const double *__restrict__ rhs, double *__restrict__ res, double *__restrict__ dir, size_t n,
                                                     double *__restrict__ PR) {
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const double r = rhs[i];
        res[i] = r;
        dir[i] = r;
        s += r * r;
    }
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) PR[blockIdx.x] = t;
}

// one workgroup: the scalars of a new solve (it owns them all: nothing else runs in this launch)
__global__ __launch_bounds__(BLOCK) void k_dcg_setup(const double *__restrict__ PR, int np, double tol, int max_iter, double *__restrict__ S,
                                                     int *__restrict__ F) {
    __shared__ double sh[BLOCK / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += BLOCK) s += PR[i];
    const double dot = block_sum(s, sh);
    if (threadIdx.x == 0) {
        const int stop = dot < tol * tol ? 1 : 0;                  // the early out: max_iter = 0, the count stays 1
        S[DCG_THRES] = dot * tol * tol;
        S[DCG_DOT + 1] = dot;                                      // iteration 1 reads slot 1
        S[DCG_DOT + 0] = 0.0;
        F[DCG_STOP] = stop;
        F[DCG_STOP_DIR] = stop;
        F[DCG_ITERS] = (!stop && max_iter == 1) ? 0 : 1;           // `if (i == max_iter && max_iter != 0) i--` with no iteration run
    }
}

struct DcgMatvecArgs {
    const int    *row_ptr;
    const int    *col;
    const double *val;
    int           n;
    const double *dir;
    double       *mt;
    double       *PA;         // gridDim.x partial sums of dir . mt
    int          *F;
};

// mt = A dir, G lanes per row (lane l of a row's group adds its entries l, l + G, ...; group_sum), 256 / G rows per workgroup and trip
template <int G>
__global__ __launch_bounds__(BLOCK) void k_dcg_matvec(const DcgMatvecArgs a) {
    static_assert(G == 1 || G == 4 || G == 16 || G == 64, "G");
    if (a.F[DCG_STOP]) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && !a.F[DCG_STOP_DIR]) a.F[DCG_STOP_DIR] = 1;   // (k_dcg_dir reads it; nothing in this launch does)
        return;
    }
    __shared__ double sh[BLOCK / 64];
    constexpr int RPP = BLOCK / G;
    const int g = threadIdx.x / G, l = threadIdx.x % G;
    const long stride = (long)gridDim.x * RPP;
    double acc = 0.0;
    for (long r = (long)blockIdx.x * RPP + g; r < a.n; r += stride) {
        double s = 0.0;
        int k = a.row_ptr[r] + l;
        const int e = a.row_ptr[r + 1];
        for (; k < e - 3 * G; k += 4 * G) {                         // four entries' loads in flight; the sum keeps the lane's order
            const double v0 = a.val[k], v1 = a.val[k + G], v2 = a.val[k + 2 * G], v3 = a.val[k + 3 * G];
            const int c0 = a.col[k], c1 = a.col[k + G], c2 = a.col[k + 2 * G], c3 = a.col[k + 3 * G];
            const double x0 = a.dir[c0], x1 = a.dir[c1], x2 = a.dir[c2], x3 = a.dir[c3];
            s += v0 * x0; s += v1 * x1; s += v2 * x2; s += v3 * x3;
        }
        for (; k < e; k += G) s += a.val[k] * a.dir[a.col[k]];
        s = group_sum<G>(s);
        if (l == 0) {
            a.mt[r] = s;
            acc += a.dir[r] * s;
        }
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) a.PA[blockIdx.x] = t;
}

// factor = dot / (dir . mt); u += factor dir; res -= factor mt; PR[block] = this block's share of the NEW res . res
__global__ __launch_bounds__(BLOCK) void k_dcg_update(const double *__restrict__ PA, int npa, const double *__restrict__ S, const int *__restrict__ F, int it,
                                                      const double *__restrict__ dir, const double *__restrict__ mt, double *__restrict__ u,
                                                      double *__restrict__ res, size_t n, double *__restrict__ PR) {
    if (F[DCG_STOP]) return;
    __shared__ double sh[BLOCK / 64];
    __shared__ double bc;
    const double factor = S[DCG_DOT + (it & 1)] / dcg_sum_all(PA, npa, sh, &bc);
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        u[i] += factor * dir[i];
        const double ri = res[i] - factor * mt[i];
        res[i] = ri;
        s += ri * ri;
    }
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) PR[blockIdx.x] = t;
}

// dot' = res . res; converged (dot' < thres): raise the stop flag, the count stays `it`; else dir = res + (dot' / dot) dir and the
// count becomes it + 1 -- or stays `it` at the cap, solve_coarsest_CG's `i--`
__global__ __launch_bounds__(BLOCK) void k_dcg_dir(const double *__restrict__ PR, int np, double *__restrict__ S, int *__restrict__ F, int it, int max_iter,
                                                   const double *__restrict__ res, double *__restrict__ dir, size_t n) {
    if (F[DCG_STOP_DIR]) return;
    __shared__ double sh[BLOCK / 64];
    __shared__ double bc;
    const double dot = dcg_sum_all(PR, np, sh, &bc);
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    if (dot < S[DCG_THRES]) {
        if (lead) F[DCG_STOP] = 1;
        return;
    }
    const double factor = dot / S[DCG_DOT + (it & 1)];
    if (lead) {
        S[DCG_DOT + ((it + 1) & 1)] = dot;
        F[DCG_ITERS] = it + 1 == max_iter ? it : it + 1;
    }
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) dir[i] = res[i] + factor * dir[i];
}

} // namespace sk
