// kernels_block.hip.h -- block vectors: K right-hand sides through one pass over the operator (gfx950, wave64).
//
// A block vector holds K columns over n rows, interleaved: X[i * K + j], K in {2, 4, 8}, 16-byte aligned.  The operator is
// what the scalar kernels stream almost alone (12 B per stored entry against 16 B per ROW of vectors), so one launch reads
// every stored entry once and applies it to all K columns:
//   * a workgroup owns one row block of the 16 KiB plan (kernels.hip.h: <= CAP entries and <= MAXROWS rows, a longer row
//     alone) and stages the block's (val, col) stream in LDS with the coalesced 16-byte loads of k_csr_stream -- 12 B of
//     LDS per entry whatever K is (staging the K products instead would take 8 K bytes per entry: 64 KiB at K = 8);
//   * G lanes per row walk the row in LDS; per entry a lane gathers the K values of x with K / 2 16-byte loads (one
//     gather lane carries 16 B of x, not 8) into K register accumulators: product rounded, then added (-ffp-contract=off);
//   * G = 1 adds a row's products in stored order (the reference's sequential sum, any row length); G > 1 gives lane l the
//     entries l, l + G, ... of the row and combines the lanes with group_sum -- the orders of k_csr_stream;
//   * column j's arithmetic never reads column j': a NaN in one column stays there, and the K instantiations perform the
//     same operations per column, so a column's bits do not depend on K or on its position in the block;
//   * an operator with a remote part: the rows that own remote entries are masked out of this launch (BlockArgs::skip) and
//     computed whole by k_csr_boundary_block once the block halo -- K columns through one exchange, packed by k_pack_block --
//     has arrived;
//   * the epilogues are those of epilogue<> (kernels.hip.h) per column; inv_diag is shared by the columns, rhs / u / d / y
//     are block vectors read and written 16 B at a time.
#pragma once
#include "kernels.hip.h"

namespace sk {

struct BlockArgs {
    const int    *row_ptr;   // [M+1]
    const int    *col;       // padded by >= 8
    const double *val;       // padded by >= 8
    const int    *blk_row;   // [nblk+1], the 16 KiB plan
    int           nblk;
    const double *x;         // block vector over the columns of the operator
    double       *y;         // block vector over its rows
    const double *rhs;       // block
    const double *inv_diag;  // [M], shared by the columns
    const double *u;         // block (the smoother's input iterate)
    double       *d;         // block (Chebyshev direction)
    double        c0, c1;
    const unsigned *skip;    // bitmask of rows this launch must NOT write (boundary rows, owned by k_csr_boundary_block), or nullptr
};

constexpr int BLK_CH = CAP + 8;   // entries staged per pass: a row block's CAP entries plus the alignment slack of its start

// one pair of columns (2h, 2h + 1) of row r: epilogue<EPI>'s arithmetic per column
template <int K, int EPI>
__device__ __forceinline__ void block_epilogue2(const BlockArgs &a, int r, int h, double s0, double s1) {
    const size_t o = (size_t)r * K + 2 * h;
    sk_d2v out;
    if constexpr (EPI == EPI_SPMV) {
        out.x = s0; out.y = s1;
    } else if constexpr (EPI == EPI_RESIDUAL) {
        const sk_d2v b = *reinterpret_cast<const sk_d2v *>(a.rhs + o);
        out.x = s0 - b.x; out.y = s1 - b.y;
    } else if constexpr (EPI == EPI_JACOBI) {
        const sk_d2v b = *reinterpret_cast<const sk_d2v *>(a.rhs + o), u = *reinterpret_cast<const sk_d2v *>(a.u + o);
        const double w = a.inv_diag[r] * a.c0;
        double t0 = s0 - b.x, t1 = s1 - b.y;
        t0 *= w; t1 *= w;
        out.x = u.x - t0; out.y = u.y - t1;
    } else if constexpr (EPI == EPI_CHEBY0 || EPI == EPI_CHEBYK) {
        const sk_d2v b = *reinterpret_cast<const sk_d2v *>(a.rhs + o), u = *reinterpret_cast<const sk_d2v *>(a.u + o);
        const double w = a.c0 * a.inv_diag[r];
        sk_d2v dd;
        dd.x = w * (b.x - s0); dd.y = w * (b.y - s1);
        if constexpr (EPI == EPI_CHEBYK) {
            const sk_d2v dp = *reinterpret_cast<const sk_d2v *>(a.d + o);
            dd.x = (a.c1 * dp.x) + dd.x; dd.y = (a.c1 * dp.y) + dd.y;
        }
        *reinterpret_cast<sk_d2v *>(a.d + o) = dd;
        out.x = u.x + dd.x; out.y = u.y + dd.y;
    } else {                                                          // EPI_SUB
        const sk_d2v y = *reinterpret_cast<const sk_d2v *>(a.y + o);
        out.x = y.x - s0; out.y = y.y - s1;
    }
    *reinterpret_cast<sk_d2v *>(a.y + o) = out;
}

// every lane of a row group holds the row's K sums: the epilogue, a column pair per lane
template <int K, int EPI, int G>
__device__ __forceinline__ void block_write_row(const BlockArgs &a, int r, int l, double (&acc)[K]) {
    if constexpr (G == 1) {
#pragma unroll
        for (int h = 0; h < K / 2; ++h) block_epilogue2<K, EPI>(a, r, h, acc[2 * h], acc[2 * h + 1]);
    } else {                                                          // G >= 4 >= K / 2: lane h writes the pair h
#pragma unroll
        for (int h = 0; h < K / 2; ++h)
            if (l == h) block_epilogue2<K, EPI>(a, r, h, acc[2 * h], acc[2 * h + 1]);
    }
}

// the G lanes of a row group hold their partial sums: combine them and write the row -- unless the launch's mask names it (a
// boundary row: summed like any other, so the lanes stay in step, but its epilogue is the halo kernel's: EPI_SUB reads y)
template <int K, int EPI, int G>
__device__ __forceinline__ void block_finish_row(const BlockArgs &a, int r, int l, double (&acc)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = group_sum<G>(acc[j]);       // (every lane of the group ends with the sum)
    if (a.skip && ((a.skip[r >> 5] >> (r & 31)) & 1u)) return;
    block_write_row<K, EPI, G>(a, r, l, acc);
}

// entries k0 + m G (< k1) of the staged stream: acc[j] += val * x[col][j]
template <int K, int G>
__device__ __forceinline__ void block_walk(const double *lv, const int *lc, const double *__restrict__ x, int k0, int k1, double (&acc)[K]) {
    for (int k = k0; k < k1; k += G) {
        const double v = lv[k];
        const sk_d2v *xp = reinterpret_cast<const sk_d2v *>(x + (size_t)lc[k] * K);
#pragma unroll
        for (int h = 0; h < K / 2; ++h) {
            const sk_d2v xv = xp[h];
            acc[2 * h]     += v * xv.x;
            acc[2 * h + 1] += v * xv.y;
        }
    }
}

// entries [cb, cb + n) of the operator's stream to LDS; cb is a multiple of 4 (16-byte loads; the arrays are padded by 8)
__device__ __forceinline__ void block_stage(const BlockArgs &a, double *lv, int *lc, int cb, int n) {
    const int nq = (n + 3) >> 2;
    for (int q = threadIdx.x; q < nq; q += BLOCK) {
        const int idx = cb + 4 * q;
        const double2 v01 = ld_stream_d2(a.val + idx, 0);
        const double2 v23 = ld_stream_d2(a.val + idx + 2, 0);
        const int4    c   = ld_stream_i4(a.col + idx, 0);
        *reinterpret_cast<double2 *>(&lv[4 * q])     = v01;
        *reinterpret_cast<double2 *>(&lv[4 * q + 2]) = v23;
        *reinterpret_cast<int4 *>(&lc[4 * q])        = c;
    }
}

template <int K, int EPI, int G>
__global__ __launch_bounds__(BLOCK) void k_csr_block(const BlockArgs a) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    static_assert(G == 1 || G == 4 || G == 16 || G == 64, "G");
    static_assert(BLK_CH % 4 == 0, "chunks start on a quad");
    __shared__ __attribute__((aligned(16))) double lv[BLK_CH];
    __shared__ __attribute__((aligned(16))) int    lc[BLK_CH];
    const int tid = threadIdx.x;
    const int b   = xcd_remap(blockIdx.x, a.nblk);
    const int r0 = a.blk_row[b], r1 = a.blk_row[b + 1];
    const int p0 = a.row_ptr[r0], p1 = a.row_ptr[r1];
    const int a0 = p0 & ~3;
    const int g = tid / G, l = tid % G;
    double acc[K];

    if (r1 - r0 > 1 || p1 - a0 <= BLK_CH) {                          // ---- the block's stream fits one pass (plan: <= CAP entries)
        block_stage(a, lv, lc, a0, p1 - a0);
        __syncthreads();
        constexpr int ROWS_PER_PASS = BLOCK / G;
        for (int r = r0 + g; r < r1; r += ROWS_PER_PASS) {
            const int s = a.row_ptr[r] - a0, e = a.row_ptr[r + 1] - a0;
#pragma unroll
            for (int j = 0; j < K; ++j) acc[j] = 0.0;
            block_walk<K, G>(lv, lc, a.x, s + l, e, acc);
            block_finish_row<K, EPI, G>(a, r, l, acc);
        }
        return;
    }
    // ---- one row longer than a pass: staged chunk by chunk, walked by the first group with the same lane -> entry map
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    for (int cb = a0; cb < p1; cb += BLK_CH) {                        // (cb, p1: uniform over the workgroup)
        if (cb != a0) __syncthreads();                                // the chunk before is consumed
        const int n = p1 - cb < BLK_CH ? p1 - cb : BLK_CH;
        block_stage(a, lv, lc, cb, n);
        __syncthreads();
        if (g == 0) {
            int k = p0 + l;                                           // lane l owns entries p0 + l + m G
            if (k < cb) k += ((cb - k + G - 1) / G) * G;
            block_walk<K, G>(lv, lc, a.x, k - cb, n, acc);
        }
    }
    if (g == 0) block_finish_row<K, EPI, G>(a, r0, l, acc);
}

// ---- boundary rows of a block apply: k_csr_boundary (kernels.hip.h) on K columns.  G lanes own one row that has remote entries: lane l
// adds the local entries l, l + G, ... of the row (x + col * K), then its halo entries l, l + G, ... (halo + h_col * K: the receive
// buffer is a block vector over the halo positions), into the K register accumulators of k_csr_block -- product rounded, then added;
// group_sum, one epilogue.  G = 1: the reference's order, the local loop first and the remote contributions after it in ascending
// receive position.  Rows are walked from global memory whatever their length: no LDS, no long-row path ----
struct BlockBoundaryArgs {
    BlockArgs     b;         // the local CSR (row_ptr / col / val), x and the epilogue operands; blk_row and skip unused
    const int    *rows;      // [nrows] boundary rows, ascending
    int           nrows;
    const int    *h_ptr;     // [nrows+1] CSR over the halo positions, one row per boundary row
    const int    *h_col;     // halo position
    const double *h_val;
    const double *halo;      // receive buffer (fp64 wire), [recvSize * K]
    const float  *halo_f;    // receive buffer of the fp32 wire, or nullptr
};

typedef float sk_f2v __attribute__((ext_vector_type(2)));

template <int K, int EPI, int G>
__global__ __launch_bounds__(BLOCK) void k_csr_boundary_block(const BlockBoundaryArgs a) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    static_assert(G == 1 || G == 4 || G == 16 || G == 64, "G");
    constexpr int RPB = BLOCK / G;
    const int i = blockIdx.x * RPB + threadIdx.x / G, l = threadIdx.x % G;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    int r = 0;
    if (i < a.nrows) {
        r = a.rows[i];
        block_walk<K, G>(a.b.val, a.b.col, a.b.x, a.b.row_ptr[r] + l, a.b.row_ptr[r + 1], acc);
        const int q1 = a.h_ptr[i + 1];
        if (a.halo_f) {
            for (int k = a.h_ptr[i] + l; k < q1; k += G) {
                const double v = a.h_val[k];
                const sk_f2v *xp = reinterpret_cast<const sk_f2v *>(a.halo_f + (size_t)a.h_col[k] * K);
#pragma unroll
                for (int h = 0; h < K / 2; ++h) {
                    const sk_f2v xv = xp[h];
                    acc[2 * h]     += v * (double)xv.x;
                    acc[2 * h + 1] += v * (double)xv.y;
                }
            }
        } else {
            block_walk<K, G>(a.h_val, a.h_col, a.halo, a.h_ptr[i] + l, q1, acc);
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = group_sum<G>(acc[j]);
    if (i < a.nrows) block_write_row<K, EPI, G>(a.b, r, l, acc);
}

// ---- halo pack of a block vector: send[t * K + j] = X[vIndex[t] * K + j], one lane per column pair (a 16-byte load; a 16-byte
// store, 8 bytes on the float wire).  as_float: the doubles rounded through float, as k_pack's (the test hook's send buffer on an
// fp32-wire operator).  Segment i of the wire is sendCount[i] * K values at sendDispl[i] * K ----
template <int K>
__global__ __launch_bounds__(BLOCK) void k_pack_block(const double *__restrict__ X, const int *__restrict__ vIndex, double *__restrict__ send, int n, int as_float) {
    constexpr int H = K / 2;
    const size_t np = (size_t)n * H, stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < np; i += stride) {
        const size_t t = i / H, h = i % H;
        sk_d2v v = *reinterpret_cast<const sk_d2v *>(X + (size_t)vIndex[t] * K + 2 * h);
        if (as_float) { v.x = (double)(float)v.x; v.y = (double)(float)v.y; }
        *reinterpret_cast<sk_d2v *>(send + t * K + 2 * h) = v;
    }
}
template <int K>
__global__ __launch_bounds__(BLOCK) void k_pack_block_f32(const double *__restrict__ X, const int *__restrict__ vIndex, float *__restrict__ send, int n) {
    constexpr int H = K / 2;
    const size_t np = (size_t)n * H, stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < np; i += stride) {
        const size_t t = i / H, h = i % H;
        const sk_d2v v = *reinterpret_cast<const sk_d2v *>(X + (size_t)vIndex[t] * K + 2 * h);
        sk_f2v f; f.x = (float)v.x; f.y = (float)v.y;
        *reinterpret_cast<sk_f2v *>(send + t * K + 2 * h) = f;
    }
}

// ---- the K dots of a block pCG after their sum over the ranks: dst[j] = src[j] on the columns of `active`; a frozen column's
// scalar keeps its bits (an all-reduce in place would multiply a stale slot by the rank count) ----
__global__ void k_copy_masked(const double *__restrict__ src, double *__restrict__ dst, int K, unsigned active) {
    const int j = threadIdx.x;
    if (j < K && ((active >> j) & 1u)) dst[j] = src[j];
}

// ---- column-major n x K  <->  block (device to device) ----
__global__ __launch_bounds__(BLOCK) void k_block_pack(const double *__restrict__ cols, double *__restrict__ blk, size_t n, int K) {
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
        for (int h = 0; h < K / 2; ++h) {
            sk_d2v v; v.x = cols[(size_t)(2 * h) * n + i]; v.y = cols[(size_t)(2 * h + 1) * n + i];
            *reinterpret_cast<sk_d2v *>(blk + i * K + 2 * h) = v;
        }
}
__global__ __launch_bounds__(BLOCK) void k_block_unpack(const double *__restrict__ blk, double *__restrict__ cols, size_t n, int K) {
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
        for (int h = 0; h < K / 2; ++h) {
            const sk_d2v v = *reinterpret_cast<const sk_d2v *>(blk + i * K + 2 * h);
            cols[(size_t)(2 * h) * n + i] = v.x; cols[(size_t)(2 * h + 1) * n + i] = v.y;
        }
}

// ---- K dot products, k_dot_partial's scheme per column: row i goes to the thread k_dot_partial gives element i, so a
// column's partial sums (and its result) depend on n alone, not on K.  partial[block * K + j]; no atomics ----
template <int K>
__global__ __launch_bounds__(BLOCK) void k_dot_block_partial(const double *__restrict__ x, const double *__restrict__ y, size_t n,
                                                             double *__restrict__ partial) {
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double s[K];
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
#pragma unroll
        for (int h = 0; h < K / 2; ++h) {
            const sk_d2v xv = *reinterpret_cast<const sk_d2v *>(x + i * K + 2 * h), yv = *reinterpret_cast<const sk_d2v *>(y + i * K + 2 * h);
            s[2 * h] += xv.x * yv.x; s[2 * h + 1] += xv.y * yv.y;
        }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double t = block_sum(s[j], sh);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * K + j] = t;
    }
}
// out[j] = sum over the np blocks of partial[block * K + j]: one workgroup per column, k_reduce_partials' order; a column
// outside `active` keeps what out[j] holds
__global__ __launch_bounds__(BLOCK) void k_reduce_partials_block(const double *__restrict__ partial, int np, int K, double *__restrict__ out, unsigned active) {
    __shared__ double sh[BLOCK / 64];
    const int j = blockIdx.x;
    if (!((active >> j) & 1u)) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += BLOCK) s += partial[(size_t)i * K + j];
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) out[j] = t;
}

// ---- centring per column (k_sum_partial / k_center on a block vector): partial[block * K + j] = the block's share of the sum of
// column j, k_sum_partial's order, so that after k_reduce_partials_block column j has the bits of the scalar kernels on that
// column alone; then y_ij = x_ij - S[j] / n.  Y may be X ----
template <int K>
__global__ __launch_bounds__(BLOCK) void k_sum_block_partial(const double *__restrict__ x, size_t n, double *__restrict__ partial) {
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double s[K];
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
#pragma unroll
        for (int h = 0; h < K / 2; ++h) {
            const sk_d2v xv = *reinterpret_cast<const sk_d2v *>(x + i * K + 2 * h);
            s[2 * h] += xv.x; s[2 * h + 1] += xv.y;
        }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double t = block_sum(s[j], sh);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * K + j] = t;
    }
}
template <int K>
__global__ __launch_bounds__(BLOCK) void k_center_block(const double *S, const double *x, double *y, size_t n) {
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double mean[K];
#pragma unroll
    for (int j = 0; j < K; ++j) mean[j] = S[j] / (double)n;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
#pragma unroll
        for (int h = 0; h < K / 2; ++h) {
            sk_d2v v = *reinterpret_cast<const sk_d2v *>(x + i * K + 2 * h);
            v.x -= mean[2 * h]; v.y -= mean[2 * h + 1];
            *reinterpret_cast<sk_d2v *>(y + i * K + 2 * h) = v;
        }
}

// ---- the k_axpby_block family: per-column coefficients from device scalars, bit j of `active` = column j takes part;
// a column that does not is neither read for writing nor written ----
// pCG update (k_pcg_update_dev per column): alpha_j = num[j] / den[j]; u -= alpha p; r -= alpha h on the active columns;
// partial[block * K + j] = the block's share of r.r of every column (a frozen column's r is only read)
template <int K>
__global__ __launch_bounds__(BLOCK) void k_pcg_update_block(const double *__restrict__ num, const double *__restrict__ den, const double *__restrict__ p,
                                                            const double *__restrict__ h, double *__restrict__ u, double *__restrict__ r, size_t n,
                                                            unsigned active, double *__restrict__ partial) {
    __shared__ double sh[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double alpha[K], s[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { alpha[j] = ((active >> j) & 1u) ? num[j] / den[j] : 0.0; s[j] = 0.0; }
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double ri = r[i * K + j];
            if ((active >> j) & 1u) {
                u[i * K + j] -= alpha[j] * p[i * K + j];
                ri = ri - alpha[j] * h[i * K + j];
                r[i * K + j] = ri;
            }
            s[j] += ri * ri;
        }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double t = block_sum(s[j], sh);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * K + j] = t;
    }
}
// pCG direction (k_pcg_direction_dev per column): beta_j = num[j] / den[j]; p = 1 z + beta p on the active columns
template <int K>
__global__ __launch_bounds__(BLOCK) void k_pcg_direction_block(const double *__restrict__ num, const double *__restrict__ den, const double *__restrict__ z,
                                                               double *__restrict__ p, size_t n, unsigned active) {
    const size_t stride = (size_t)gridDim.x * BLOCK;
    double beta[K];
#pragma unroll
    for (int j = 0; j < K; ++j) beta[j] = ((active >> j) & 1u) ? num[j] / den[j] : 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
#pragma unroll
        for (int j = 0; j < K; ++j)
            if ((active >> j) & 1u) p[i * K + j] = 1.0 * z[i * K + j] + beta[j] * p[i * K + j];
}

// ---- coarsest level, direct: u = Ainv rhs for K columns, C of them per pass (C * n <= DS_CAP doubles of LDS); k_dense_solve's
// wave per row and lane -> column map, so a column's sum does not depend on K or C ----
constexpr int DS_CAP = 4096;
template <int C>
__global__ __launch_bounds__(CG_BLOCK) void k_dense_solve_block(const double *__restrict__ Ainv, const double *__restrict__ rhs,
                                                                double *__restrict__ u, int n, int K) {
    __shared__ double r[DS_CAP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j0 = 0; j0 < K; j0 += C) {
        if (j0) __syncthreads();
        for (int t = threadIdx.x; t < n * C; t += CG_BLOCK) r[t] = rhs[(size_t)(t / C) * K + j0 + (t % C)];
        __syncthreads();
        for (int i = wave; i < n; i += CG_BLOCK / 64) {
            double s[C];
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] = 0.0;
            for (int j = lane; j < n; j += 64) {
                const double av = Ainv[(size_t)i * n + j];
#pragma unroll
                for (int c = 0; c < C; ++c) s[c] += av * r[j * C + c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double t = group_sum<64>(s[c]);
                if (lane == 0) u[(size_t)i * K + j0 + c] = t;
            }
        }
    }
}

} // namespace sk
