/*
 * saena_gpu_debug.h -- test, rehearsal and bench scaffolding exported by libsaena_amd.so.
 *
 * NOT part of the drop-in boundary (that is include/saena_gpu.h): nothing a Saena maintainer binds
 * lives here.  These entry points exist so that the multi-rank code of the library can be validated
 * on ONE GPU (RCCL refuses several ranks on one device) and so that bench.py can keep a measured line
 * when an optional later leg dies.  tests/, bench.py and the perf scripts are the only callers.
 */
#ifndef SAENA_GPU_DEBUG_H
#define SAENA_GPU_DEBUG_H

#include "saena_gpu.h"
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Halo path on a single GPU: sgpu_debug_pack runs the pack kernel (saena_matrix_matvec.cpp:25-26) and
 * downloads the send buffer; sgpu_debug_inject_halo uploads the receive buffer and makes the following
 * applies use the remote part without any exchange.  Tests route the buffers between operators on the host. */
int sgpu_debug_pack(sgpu_op *op, const value_t *v, value_t *send_host);
int sgpu_debug_inject_halo(sgpu_op *op, const value_t *recv_host);
/* Their block twins (K = 2, 4, 8 columns; X: a device block vector X[i * K + j] over the operator's columns).  The wire layout of
 * a block halo: segment i of the send buffer is sendCount[i] * K values at sendDispl[i] * K, send[t * K + j] = X[vIndex[t] * K + j];
 * the receive buffer is a block vector over the halo positions, recv[p * K + j].  pack_block downloads the vIndexSize * K doubles of
 * the send buffer (rounded through float on an fp32-wire operator, as sgpu_debug_pack's); inject_halo_block uploads recvSize * K
 * doubles and makes the following block applies WITH THIS K run the interior and boundary kernels on one stream, no exchange. */
int sgpu_debug_pack_block(sgpu_op *op, const value_t *X, int K, value_t *send_host);
int sgpu_debug_inject_halo_block(sgpu_op *op, int K, const value_t *recv_host);
/* An operator with remote entries applied in a context that has neither a communicator nor a host transport nor
 * an injected halo is an error (SGPU_ERR_STATE): the result would silently miss the remote part.  allow != 0
 * lifts that for this operator: only its local part is applied (plan/launch tests whose numbers mean nothing). */
int sgpu_debug_allow_local_only(sgpu_op *op, int allow);
/* diagnostic: time of the x[col] gather alone over the local part, mode 0 = production lane mapping (4 consecutive
 * nnz per lane), 1 = 64 consecutive nnz per gather instruction */
int sgpu_debug_gather_probe(sgpu_op *op, int mode, const value_t *x, int reps, float *ms);

/* bench.py (configs[4], "stresses load-balance of wavefront CSR"): the spread of work over the row blocks of the tile kernels' plan
 * (big = 0: 16 KiB tiles of <= 2048 products / 256 rows, 1: 32 KiB tiles).  out[0..7] = blocks, fewest / most entries in a block,
 * entries in all, fewest / most rows in a block, rows longer than the tile (a block of their own: the long-row path), longest row.
 * big = 2: the x-in-LDS plan of variants 10 / 12 / 16 once one of them was set: out[0..4] = chunks, most windows of a chunk, columns
 * per window, 1 where the partial row sums live in LDS behind the window (0: in global memory), most rows in a chunk; the rest 0. */
int sgpu_debug_block_plan(const sgpu_op *op, int big, long *out);

/* bench.py: the streaming ceiling of a byte mix on this device -- a kernel that reads `read_bytes` with wave-coalesced 16-byte
 * loads and writes `write_bytes` with 8-byte stores and does nothing else (no gathers, no LDS), `reps` launches back to back after
 * 3 warm-up launches, plain and non-temporal loads / stores: *us = the fastest of the four forms, *mode = which (bit 0: non-temporal
 * loads, bit 1: non-temporal stores), *bytes_moved = the bytes one launch actually moves (the read stream is rounded to whole
 * 16-byte loads per written double).  A sweep over an operator that stores those bytes cannot be faster: time(ceiling) /
 * time(kernel) is `roofline.frac_of_measured`, <= 1 whether the working set is cache- or HBM-resident. */
int sgpu_debug_stream_ceiling(size_t read_bytes, size_t write_bytes, int reps, float *us, int *mode, size_t *bytes_moved);

/* Host-routed transport (validation without one GPU per rank): the context of rank `rank` of `nranks` is created
 * WITHOUT an RCCL communicator; every halo exchange is staged through host memory and handed to `exchange`, every
 * scalar reduction to `allreduce_sum`.  All library code above the transport (plans, interior/boundary kernels,
 * V-cycle, solve*, coarse levels agglomerated onto fewer ranks ...) is the multi-rank code.  exchange: send/recv are
 * packed host buffers of `elem_bytes`-sized elements, peers in ascending rank order. */
typedef int (*sgpu_host_exchange_fn)(void *user, const void *send, const int *send_rank, const int *send_count, int nsend,
                                     void *recv, const int *recv_rank, const int *recv_count, int nrecv, int elem_bytes);
typedef int (*sgpu_host_allreduce_fn)(void *user, double *v, int n);
int sgpu_debug_init_host_transport(int device_id, int rank, int nranks, sgpu_host_exchange_fn exchange,
                                   sgpu_host_allreduce_fn allreduce_sum, void *user);

/* bench.py only: from now on a fatal signal in this process (SIGSEGV/SIGBUS/SIGABRT/SIGFPE/SIGILL -- the HIP runtime
 * aborts on a GPU fault) writes `line` (may be empty) to stdout, a one-line reason to stderr, and ends the process
 * with status 128 + signal: the line measured before an optional later leg is kept, and the failure still reaches
 * the launcher as a failure.  SIGTERM is not trapped.  NULL restores the default handlers.  `line` is copied. */
int sgpu_debug_on_fatal_print(const char *line);

/* the exchange chain sgpu_init measured on the communicator (pack -> grouped send/recv with the neighbouring rank -> a kernel
 * on the received data; microseconds, the maximum over the ranks); 0 without a communicator.  The agglomeration of coarse
 * levels and the one- / two-stream thresholds of a multi-rank apply start from it. */
int sgpu_debug_chain_us(double *us);
/* tests (tests/rccl_mirror.py): how the next scalar apply of `op` (sgpu_spmv, the residuals, a smoother sweep ...) orders its halo
 * exchange against its rows, for an apply whose peers are already connected (the first exchange with a peer always takes events).
 * Computed by the predicate apply() itself branches on, from the operator's current form and the context:
 *   0 no exchange (no halo, an injected halo, or no transport)   1 host transport   2 one stream (also: the dense form with a halo)
 *   3 two streams, flags polled by kernels   4 two streams, stream value operations   5 two streams, events */
int sgpu_debug_exchange_mode(const sgpu_op *op, int *mode);
/* number of kernel launches + graph launches + RCCL group calls the library has enqueued since sgpu_init
 * (tests: "fewer launches per V-cycle"); counts host-side enqueues, not GPU work */
int sgpu_debug_launch_count(long *launches);

/* tests (tests/test_gpu_plan_storage.py): which storage groups of the operator's local part hold device memory, and how many bytes
 * all of the library's owned device and pinned arrays hold in this process (vectors from sgpu_vec_alloc belong to the caller and
 * are not counted).  op may be NULL (the mask is then 0).  *group_mask, bit set = the group holds at least one array:
 *    0 csr (row pointers, columns, values, row-block plans)     1 dense rows
 *    2, 3 16-bit compressed columns of the 16 / 32 KiB plan      4, 5 column-major-in-block copies of the 16 / 32 KiB plan
 *    6 sliced-ELLPACK values      7 sliced-ELLPACK column codes   8 row patterns (k_sellp's ids and tables)
 *    9 value codes (k_vidx)      10, 11, 12 x-window tables for workgroups of 256 / 512 / 1024 rows
 *   13 row-paired values (k_sellp2)   14 row patterns with x in LDS (k_sellpx)   15 row templates (k_rowt)
 *   16 x-in-LDS chunk plan       17 x-in-LDS columns              18 sliced ELLPACK in LDS windows (k_sellx) */
int sgpu_debug_op_storage(const sgpu_op *op, unsigned *group_mask, long long *live_bytes);

/* one line describing the device of the context (name, architecture, compute units, clocks, L2, memory), for bench
 * lines and logs: the same kernel ran 1 055-1 213 us on different boxes of one pool.  `buf` receives at most len-1
 * characters and a terminator. */
int sgpu_debug_device_info(char *buf, int len);

/* measurement scripts (tests/perf_block.py): sgpu_time_kernel for the block kernel -- `reps` back-to-back launches inside the
 * library between two events of their own; kind 0: Y = A X, 1: one Jacobi sweep X -> Y -- and the same for whole V-cycles,
 * K = 0: the scalar sgpu_vcycle on (U, RHS), K = 2, 4, 8: sgpu_vcycle_block (one call before the interval captures the graph). */
int sgpu_debug_time_block(sgpu_op *op, int kind, const value_t *X, const value_t *RHS, value_t *Y, int K, int reps, float *ms_per_launch);
int sgpu_debug_time_vcycle(sgpu_amg *h, value_t *U, const value_t *RHS, int K, int reps, float *ms_per_cycle);

/* tests (tests/test_gpu_block_solver_layer.py): the block dot and the two block pCG updates as sgpu_solve_pCG_block launches them
 * (its K switch and its grids), on the caller's block vectors X[i * K + j] of n rows.  The hierarchy is taken for its per-K state
 * alone (the partial sums of the dots): n is the caller's and need not be the hierarchy's size.  Every pointer is a device
 * pointer; num / den / out_dev / rr_dev hold K doubles.  Bit j of `active` = column j takes part: the others are not written,
 * and neither are their out_dev[j] / rr_dev[j].
 *   dot:        out_dev[j] = X_j . Y_j
 *   pcg_update: alpha_j = num[j] / den[j]; U_j -= alpha_j P_j; R_j -= alpha_j H_j; rr_dev[j] = R_j . R_j
 *   direction:  beta_j = num[j] / den[j]; P_j = Z_j + beta_j P_j */
int sgpu_debug_block_dot(sgpu_amg *h, const value_t *X, const value_t *Y, size_t n, int K, unsigned active, value_t *out_dev);
int sgpu_debug_block_pcg_update(sgpu_amg *h, const value_t *num, const value_t *den, const value_t *P, const value_t *H,
                                value_t *U, value_t *R, size_t n, int K, unsigned active, value_t *rr_dev);
int sgpu_debug_block_pcg_direction(sgpu_amg *h, const value_t *num, const value_t *den, const value_t *Z, value_t *P,
                                   size_t n, int K, unsigned active);

/* tests (tests/test_gpu_gmres.py): the two Gram-Schmidt launch helpers of sgpu_solve_FGMRES on the caller's arrays.  V: device,
 * column-major, column c at V + c * ld, ld even and >= n, 16-byte aligned; w: device, n rows, 16-byte aligned; ncols <= 65.
 *   dots:   out_host[c] = V[:,c] . w
 *   update: w -= sum_c h_host[c] V[:,c], ascending c, product rounded then subtracted; *norm2_out_host (may be NULL) = the new w . w
 * time_gs (tests/perf_gmres.py): ms per run of `reps` back-to-back runs, kind 0: dots, 1: update with the norm (zero coefficients). */
int sgpu_debug_gs_dots(const value_t *V, size_t ld, int ncols, const value_t *w, size_t n, value_t *out_host);
int sgpu_debug_gs_update(const value_t *V, size_t ld, int ncols, const value_t *h_host, value_t *w, size_t n, value_t *norm2_out_host);
int sgpu_debug_time_gs(int kind, const value_t *V, size_t ld, int ncols, value_t *w, size_t n, int reps, float *ms_per_run);

/* tests (tests/test_gpu_eig_kernels.py): the launch helpers of sgpu_eigs_LOBPCG on the caller's block vectors X[i * K + j] of n rows
 * (16-byte aligned device pointers; the hierarchy is taken for its per-K partial sums alone: n is the caller's).
 *   block_gram:   out_dev[a * K + b] = X_a . Y_b, K^2 doubles, every entry with the bits of sgpu_dot on the two columns
 *   block_mix:    Out[i, b] = sum_{s < ns} sum_a S_s[i, a] C_s[a, b] (+ Add[i, b] when Add is not NULL), ns = 1, 2 or 3; C_s: device,
 *                 K x K row-major; sources beyond ns are ignored; Out may alias any source and Add
 *   eig_residual: R = AX - X diag(lambda_dev), rr_dev[j] = ||r_j||^2 (K doubles)
 *   eig_stop:     the next sgpu_eigs_LOBPCG with this K returns SGPU_ERR_NOCONV right after the orthonormalisation step of iteration
 *                 index `iteration` (0-based), before the Rayleigh-Ritz update: eig_vector then shows W, AW, P, AP as that step left them
 *   eig_vector:   after a solve, a copy of one of the solver's own block vectors (which: 0 AX, 1 R, 2 W, 3 AW, 4 P, 5 AP) into dst
 * time_eig (tests/perf_eig.py): ms per run of `reps` back-to-back runs, kind 0: block_gram of (X, Y), 1: block_mix of ns sources
 * (X, Y, X; zero coefficients) into Out, 2: eig_residual of (AX = X, X = Y) into Out.
 * The generalised solve (sgpu_eigs_LOBPCG_gen; tests/test_gpu_geig_kernels.py, tests/test_gpu_geig.py): eig_stop stops it the same
 * way, and after it eig_vector also gives which = 6 BX, 7 BW, 8 BP (SGPU_ERR_STATE before the first generalised solve with this K).
 *   geig_residual: R = AX - BX diag(lambda_dev), rr_dev[j] = ||r_j||^2 and bb_dev[j] = ||(BX)_j||^2 (K doubles each) from one pass
 *   time_geig (tests/perf_geig.py): ms per run of `reps` back-to-back runs of geig_residual with both reductions. */
int sgpu_debug_block_gram(sgpu_amg *h, const value_t *X, const value_t *Y, size_t n, int K, value_t *out_dev);
int sgpu_debug_block_mix(int K, int ns, const value_t *S0, const value_t *C0, const value_t *S1, const value_t *C1, const value_t *S2,
                         const value_t *C2, const value_t *Add, value_t *Out, size_t n);
int sgpu_debug_eig_residual(sgpu_amg *h, const value_t *AX, const value_t *X, const value_t *lambda_dev, value_t *R, size_t n, int K, value_t *rr_dev);
int sgpu_debug_eig_stop(sgpu_amg *h, int K, int iteration);
int sgpu_debug_eig_vector(sgpu_amg *h, int K, int which, value_t *dst);
int sgpu_debug_time_eig(sgpu_amg *h, int kind, int ns, const value_t *X, const value_t *Y, value_t *Out, size_t n, int K, int reps, float *ms_per_run);
int sgpu_debug_geig_residual(sgpu_amg *h, const value_t *AX, const value_t *BX, const value_t *lambda_dev, value_t *R, size_t n, int K,
                             value_t *rr_dev, value_t *bb_dev);
int sgpu_debug_time_geig(sgpu_amg *h, const value_t *AX, const value_t *BX, value_t *R, size_t n, int K, int reps, float *ms_per_run);

/* tests (tests/test_gpu_eig_lock_kernels.py): the launch helpers of hard locking (sgpu_eigs_LOBPCG_locked) on the caller's device
 * arrays.  Z and Q: L <= 64 column-major columns, column l at Z + l * ld, ld even and >= n; Y and W: block vectors, 16-byte aligned.
 *   lock_gram: out_dev[l * K + b] = Z[:, l] . Y[:, b] (L K doubles), through the hierarchy's lock partial sums
 *   lock_project: W <- W - Q C, C_dev (L x K, row-major) in device memory
 *   block_refill: column col of X from the refill generator with this counter value
 *   time_lock (tests/perf_eig_many.py): ms per run of `reps` back-to-back runs, kind 0: lock_gram of (Q, Y), 1: lock_project of Q
 *   into Y with zero coefficients. */
int sgpu_debug_lock_gram(sgpu_amg *h, const value_t *Z, size_t ld, int L, const value_t *Y, size_t n, int K, value_t *out_dev);
int sgpu_debug_lock_project(const value_t *Q, size_t ld, const value_t *C_dev, int L, value_t *W, size_t n, int K);
int sgpu_debug_block_refill(value_t *X, size_t n, int K, int col, unsigned counter);
int sgpu_debug_time_lock(sgpu_amg *h, int kind, const value_t *Q, size_t ld, int L, value_t *Y, size_t n, int K, int reps, float *ms_per_run);

/* tests (tests/test_gpu_lanczos.py): begin = 1 opens a capture on the compute stream (thread-local mode), begin = 0 ends it and
 * discards the graph -- for the entry points that must refuse to run inside a capture.  Nothing is launched in between by the tests. */
int sgpu_debug_capture(int begin);

/* measurement scripts (tests/perf_coarse_cg.py): ms per launch of the device coarsest CG's product kernel (coarse_solver = 2, a
 * coarsest level past 1 024 rows) on the hierarchy's coarsest operator, y = A x with the partial sums of x . y, `reps` back-to-back
 * launches between two events after one warm-up launch: what sgpu_time_kernel(op, 0, ...) measures for the operator's tuned form.
 * x, y: device vectors of the coarsest level's rows.  SGPU_ERR_STATE where the hierarchy runs no device CG on this rank. */
int sgpu_debug_dcg_matvec_time(sgpu_amg *h, const value_t *x, value_t *y, int reps, float *ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* SAENA_GPU_DEBUG_H */
