/*
 * saena_gpu.h -- C ABI of libsaena_amd.so, the MI355X (gfx950) implementation of
 * the Saena V-cycle hot path.
 *
 * This is the drop-in boundary.  The reference (paralab/Saena) has no plugin
 * or FFI layer; its seam is the member-function level of the distributed
 * operators that saena_object::vcycle calls on host row-slices
 * (SURVEY.md section 8b).  Each entry point below names the reference
 * interface it replaces (file:line in the reference checkout).  All functions
 *   - take plain pointers and sizes (no C++/torch types),
 *   - return 0 on success or a negative sgpu_status (never exit()/abort(),
 *     unlike the reference, which prints and calls exit(EXIT_FAILURE)),
 *   - are, like the reference operators, NOT re-entrant per handle: one host
 *     thread drives one rank = one GPU.
 *
 * Typedefs mirror include/data_struct.h:36-38 of the reference.
 */
#ifndef SAENA_GPU_H
#define SAENA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int    index_t;   /* data_struct.h:36 */
typedef long   nnz_t;     /* data_struct.h:37 */
typedef double value_t;   /* data_struct.h:38 */

typedef enum {
    SGPU_OK            =  0,
    SGPU_ERR_ARG       = -1,   /* bad argument / inconsistent descriptor     */
    SGPU_ERR_HIP       = -2,   /* a HIP runtime call failed                  */
    SGPU_ERR_RCCL      = -3,   /* an RCCL call failed                        */
    SGPU_ERR_STATE     = -4,   /* sgpu_init not called / already finalized   */
    SGPU_ERR_NOMEM     = -5,
    SGPU_ERR_NOCONV    = -6    /* solver hit max_iter without converging     */
} sgpu_status;

/* text of the last error on this thread's context ("" if none) */
const char *sgpu_last_error(void);

/* ---- context: one process = one rank = one GPU ---------------------------
 * Replaces MPI_Init/MPI_Comm_rank/size + the communicator stored in every
 * reference operator (saena_matrix.h:73 `MPI_Comm comm`).
 * rccl_unique_id: 128-byte ncclUniqueId produced by sgpu_get_unique_id on
 * rank 0 and handed to all ranks by the caller (any side channel); may be
 * NULL when nranks == 1.  Creates the compute stream and the halo stream. */
#define SGPU_UNIQUE_ID_BYTES 128
int sgpu_get_unique_id(void *out128);
int sgpu_init(int device_id, int rank, int nranks, const void *rccl_unique_id);
int sgpu_finalize(void);
int sgpu_rank(void);
int sgpu_nranks(void);
int sgpu_device_sync(void);          /* both streams idle                   */
int sgpu_barrier(void);              /* device sync + RCCL all-reduce of 1 int */

/* ---- device vectors (row slices of length local M) -----------------------
 * The reference passes raw host `value_t*` slices owned by the caller
 * (saena_matrix.h:304).  Here vectors live in HBM; these helpers replace
 * saena_aligned_alloc/saena_free (aux_functions.h:299-310). */
int sgpu_vec_alloc(value_t **dev, size_t n);
int sgpu_vec_free(value_t *dev);
int sgpu_vec_upload(value_t *dev, const value_t *host, size_t n);
int sgpu_vec_download(value_t *host, const value_t *dev, size_t n);
int sgpu_vec_fill(value_t *dev, value_t a, size_t n);            /* fill(), saena_object_solve.cpp:1249,2640 */
int sgpu_vec_copy(value_t *dst, const value_t *src, size_t n);
/* y = a*x + b*y (covers solve_pCG's updates, saena_object_solve.cpp:2593-2596,2665-2667) */
int sgpu_vec_axpby(value_t a, const value_t *x, value_t b, value_t *y, size_t n);
/* dotProduct (aux_functions.h:116-123): local dot on the GPU + all-reduce over ranks */
int sgpu_dot(const value_t *x, const value_t *y, size_t n, value_t *out);
/* y = x - mean(x) over n rows; y may be x.  The sum has sgpu_dot's order of summation (the dot of x with a vector of ones), one
 * division forms the mean, one subtraction per row: three launches, no atomics, the same bits from call to call.  Without mean_host
 * nothing comes down and the call can be captured; with it one host synchronisation returns the mean that was subtracted -- how a
 * caller learns how inconsistent the right-hand side of a singular system is (sgpu_amg_create_null_space).  One rank: with more the
 * mean would be this rank's alone, SGPU_ERR_ARG.  n = 0: nothing is launched, *mean_host = 0. */
int sgpu_vec_center(const value_t *x, value_t *y, size_t n, value_t *mean_host /*may be NULL*/);

/* ---- distributed sparse operator ----------------------------------------
 * One descriptor carries, for THIS rank, exactly the arrays the reference
 * operators hold after set_off_on_diagonal (saena_matrix_setup.cpp:793-1098),
 * prolong_matrix::findLocalRemote (prolong_matrix.cpp:18-378) or
 * restrict_matrix::transposeP (restrict_matrix.cpp:10-494), under the same
 * names.  Host pointers; the library copies what it needs (caller keeps
 * ownership) and re-lays the data out for the GPU:
 *   local  CSR (no row pointers, global columns) -> CSR with row_ptr, columns
 *          rebased by col_offset, plus a row-block plan for the kernel;
 *   remote CSC over the receive buffer -> CSR over the halo buffer, restricted
 *          to the rows that have remote entries (no atomics, deterministic);
 *   vIndex / send / recv plan -> persistent device send+recv buffers.       */
typedef struct {
    index_t        M;                 /* local rows                (saena_matrix.h:77)  */
    index_t        N_local;           /* local length of the input vector = split_col[rank+1]-split_col[rank] */
    index_t        col_offset;        /* split[rank] of the COLUMN partition: the kernel reads v[col - col_offset]
                                         (saena_matrix_matvec.cpp:56, restrict_matrix.cpp:662, prolong_matrix.cpp:538) */
    nnz_t          nnz_l_local;
    const index_t *nnzPerRow_local;   /* [M]                                            */
    const index_t *col_local;         /* [nnz_l_local], GLOBAL column ids, row-major; within a row the columns are DISTINCT
                                         and ASCENDING (the reference's row-major sort).  sgpu_op_create checks it and
                                         returns SGPU_ERR_ARG naming the row and the position; nothing is built */
    const value_t *val_local;
    nnz_t          nnz_l_remote;
    index_t        col_remote_size;   /* == recvSize                                    */
    const index_t *nnzPerCol_remote;  /* [col_remote_size], in receive-buffer order     */
    const index_t *row_remote;        /* [nnz_l_remote] local row; inside one receive column the rows may come in any
                                         order but each at most once (checked: SGPU_ERR_ARG)                  */
    const value_t *val_remote;
    int            numRecvProc, numSendProc;
    const int     *recvProcRank, *recvProcCount;   /* [numRecvProc], ascending rank     */
    const int     *sendProcRank, *sendProcCount;   /* [numSendProc], ascending rank     */
    index_t        vIndexSize;
    const index_t *vIndex;            /* [vIndexSize] local ids, grouped by destination rank (ascending) */
    const value_t *inv_diag;          /* [M] or NULL (R, P)        (saena_matrix.h, inverse_diag :1562)  */
    int            halo_fp32;         /* 1: halo travels as float  (matvec_sparse_float, saena_matrix_matvec.cpp:448-550) */
} sgpu_op_desc;

typedef struct sgpu_op sgpu_op;       /* opaque */

int sgpu_op_create(const sgpu_op_desc *desc, sgpu_op **out);
int sgpu_op_destroy(sgpu_op *op);
/* sizes / plan facts for reporting */
int sgpu_op_info(const sgpu_op *op, index_t *M, index_t *N_local, nnz_t *nnz_local, nnz_t *nnz_remote,
                 int *n_row_blocks, int *lanes_per_row);
/* kernel variant override (tuning/tests): lanes_per_row in {0=auto,1,2,4,...,64} */
int sgpu_op_set_lanes_per_row(sgpu_op *op, int lanes);
/* kernel variant of the local part: 0 k_csr_stream with 16 KiB tiles, 1 with 32 KiB tiles, 2 k_csr_vector
 * (no LDS staging), 3 / 4 k_csr_cc16 (16-bit compressed column ids, 10 B/nnz; the slot/offset split is chosen per
 * operator) on the 16 / 32 KiB plan, refused when a block touches more than 256 column segments of 256 columns;
 * 5 k_dense_rows: dense row-major storage (saena_matrix_dense, the reference's `switch_to_dense`; with a halo:
 * k_dense_rows_halo), at most 8192 rows and 64 M entries per rank; 6 k_csr_wave (long rows streamed by a wave);
 * 7 / 8 k_csr_cm: compressed columns with the entries of a row block in column order (12 B/nnz, fewer L1 requests on
 * rows of a few hundred entries) on the 16 / 32 KiB plan; 9 k_sell: sliced ELLPACK, a lane per row, 16-bit column codes
 * (operators whose slices of 64 rows pad to at most 12 % more entries; with SAENA_SELL_SORTED=1 also, as "k_sell<sorted>",
 * operators that pad to at most 5 % once their rows are sorted by length inside windows of 2048 rows -- opt-in: it
 * lost to the tile kernels wherever it was measured); 10 k_csr_xlds: the input vector staged in LDS
 * in windows of 20224 columns, one workgroup per CU (row chunks that reach over at most 8 windows; 4-64 lanes per row
 * piece, sgpu_op_set_lanes_per_row); 11 k_sellp: k_sell's values without a column stream -- a 16-bit id per row into a
 * table of (length, columns relative to the row) patterns held in LDS, 8 B per entry + 2 B per row (operators that
 * qualify for 9 and whose rows follow few enough patterns for a table of 4096 ints: stencils on structured grids, band
 * matrices; or, "k_sellp<wide>", where the patterns that every group of 1024 consecutive rows follows fit 8192 ints -- a
 * table per workgroup: the first smoothed-aggregation level of a structured grid; or, "k_sellp<rowbase>", where the rows repeat
 * relative to their FIRST COLUMN, kept per row -- the level-0 restriction / prolongation of a structured grid, the loops of
 * src/restrict_matrix.cpp:674-724 / src/prolong_matrix.cpp:550-614; the local loop of src/saena_matrix_matvec.cpp:68-80 with the same sequential row sum); 12 k_sellx: sliced
 * ELLPACK inside the (row chunk, column window) blocks of the x-in-LDS plan, a lane per row piece (rows of a few hundred
 * entries; at most 25 % padding); 13 k_rowt: row templates -- rows that repeat (length, relative columns, values) served
 * from a table in LDS, a 16-bit template id per row and nothing else of the operator (constant-coefficient stencils; never
 * chosen by the autotune unless SAENA_ROW_TEMPLATES=1); 14 k_sellp2: k_sellp with a lane per TWO adjacent rows in
 * slices of 128 rows -- the input vector is read, and the output written, 16 B at a time (operators that qualify for 11
 * and whose row pairs share a length; what the autotune keeps on fine levels larger than the Infinity Cache).
 * 15 k_sellpx: k_sellp with the windows of x that a workgroup of 512 rows reaches staged in LDS and a 16-bit table per
 * workgroup (operators that qualify for 11 and whose pattern offsets fall into at most 16 clusters that fit 80 KiB of LDS
 * together with the table); 16 k_csr_xldsr: k_csr_xlds with FOUR consecutive rows per group step (4 / 8 / 16 lanes per
 * group) -- irregular operators of a few dozen entries per row, where one row per step leaves the kernel waiting on the
 * latency of a row (BASELINE configs[4] scaled to 1 M rows); 17 k_vidx: k_sellp with its values as 8-bit codes into a
 * dictionary per workgroup of 256 rows -- 1 B per entry instead of 8, the same products and row sums (operators that qualify for
 * 11 with ONE pattern table and hold at most 256 distinct values, as bit patterns, in every group of 256 rows: constant-
 * coefficient stencils and their level-0 transfers; "k_vidx<rowbase>" on the rowbase table; SAENA_NO_VALUE_INDEX=1 keeps it
 * out of the autotune).  Variant 17 has a second LAUNCH MODE, sgpu_op_set_x_windows below: the same stored operator, x gathered
 * from LDS windows; sgpu_op_set_variant(17) alone selects direct gathers and both modes report 17, "k_vidx".
 * Only 12 and 13 still depend on the host copy of the values, which the library keeps only until the plan-time autotune
 * (SGPU_ERR_ARG afterwards); every form returns SGPU_ERR_ARG where it does not apply */
int sgpu_op_set_variant(sgpu_op *op, int variant);
int sgpu_op_get_variant(const sgpu_op *op, int *variant, const char **kernel_name);
/* x-window launch mode of variant 17 (k_vidxw): a workgroup of rows_per_workgroup in {256, 512, 1024} consecutive rows loads the
 * few windows of x its rows reach ONCE into LDS and gathers from there (the 7-point level: three windows instead of seven loads
 * per row); 0 turns it off (direct gathers).  Results are bit-identical in both modes.  SGPU_ERR_ARG, with a message that names
 * the "x windows", where the mode does not apply -- the operator is not on variant 17, rowbase or per-workgroup pattern tables,
 * more than 16 windows, LDS positions beyond 16 bits, more than 64 KiB of LDS -- and the operator stays as it was.  The autotune
 * times the mode next to direct gathers wherever it offers 17 (SAENA_NO_X_WINDOWS=1 leaves it out) and the plan cache remembers it.
 * sgpu_op_get_x_windows: the rows per workgroup in use, 0 = direct gathers (or another variant). */
int sgpu_op_set_x_windows(sgpu_op *op, int rows_per_workgroup);
int sgpu_op_get_x_windows(const sgpu_op *op, int *rows_per_workgroup);
/* which kernel the x-window mode runs on this operator: 0 the general k_vidxw (or the mode is off), 1 k_vidxw_fast, the common path
 * as a kernel of its own (workgroups of 256 / 512 rows, one slice width, one dictionary length, at most four trips; launches
 * without a halo of the product, the residual and the Jacobi sweep; SAENA_VIDXW_FAST=0, read when the windows are built, keeps
 * the general kernel), 2 k_vidxw_fast with dictionaries of at most two values in scalar registers.  Once the operator was
 * launched in the mode: what its LAST launch ran (a halo launch or another epilogue of an eligible operator runs k_vidxw).
 * Results are bit-identical whichever runs. */
int sgpu_op_get_x_window_kernel(const sgpu_op *op, int *kernel);
/* bits per entry of the code stream variant 17 reads on this operator: 8 for k_vidx, k_vidxw and k_vidxw_fast on the 8-bit codes,
 * 1 where k_vidxw_fast with scalar dictionaries (kernel 2) reads the codes packed to one bit per entry (every code is 0 or 1 there;
 * SAENA_VIDXW_BITS=0, read when the windows are built, keeps the 8-bit codes); 0: the operator is not on variant 17.  Once the
 * operator was launched in the mode: what its LAST launch read.  Results are bit-identical in both formats. */
int sgpu_op_get_x_window_code_width(const sgpu_op *op, int *bits_per_entry);
/* how k_vidxw_fast reads its rows on this operator: 1 as LANE MASKS -- where the dictionaries stay in scalar registers, the codes
 * are bits, no pattern is longer than eight positions and every pattern is an ordered subset of the longest one (stencil-like
 * operators), a slice of 64 rows is 128 bytes of 64-bit masks, two bits per (row, slot), read as scalars; no pattern id, no code
 * and no table is loaded (such a launch still reports a code width of 1) -- 0 through the pattern table (every other operator, the
 * mode off, another variant; SAENA_VIDXW_MASKS=0, read when the windows are built, keeps the table rows).  Once the operator was
 * launched in the mode: what its LAST launch read.  Results are bit-identical in both formats. */
int sgpu_op_get_x_window_row_format(const sgpu_op *op, int *format);
/* time the (variant, lanes) candidates that apply to this operator and keep the fastest (plan-time autotune; no
 * collective).  Call it right after sgpu_op_create: operators of up to 768 entries per row hold a host copy of their
 * values (8 B per entry) for the re-ordered forms from the create until this call -- or until sgpu_op_destroy. */
int sgpu_op_autotune(sgpu_op *op);

/* All vector arguments below are DEVICE pointers to this rank's slices.
 * Calls enqueue on the context's compute stream and return without waiting
 * unless stated otherwise; sgpu_device_sync() or any download waits.       */

/* w = A v.  saena_matrix::matvec -> matvec_sparse (saena_matrix_matvec.cpp:9-113);
 * restrict_matrix::matvec (restrict_matrix.cpp:612-744); prolong_matrix::matvec
 * (prolong_matrix.cpp:489-624). */
int sgpu_spmv(sgpu_op *op, const value_t *v, value_t *w);
/* res = A u - rhs.  saena_matrix::residual (saena_matrix.tpp:16-23) */
int sgpu_residual(sgpu_op *op, const value_t *u, const value_t *rhs, value_t *res);
/* res = rhs - A u.  saena_matrix::residual_negative (saena_matrix.tpp:26-33; the GMRES drivers of saena_object_solve.cpp:3848-4291).
 * Computed as 1 * 1 * (rhs - A u) through sgpu_residual_multiply: the same bits, signs of zeros included. */
int sgpu_residual_negative(sgpu_op *op, const value_t *u, const value_t *rhs, value_t *res);
/* res = c * w o (rhs - A u), evaluated as (c w_i) (rhs_i - (A u)_i).  saena_matrix::residual_multiply (saena_matrix.tpp:35-43: the
 * Chebyshev steps of saena_matrix.cpp:1099,1119 with w = inv_diag); fused into the operator's kernel.  res must not alias u, rhs or w. */
int sgpu_residual_multiply(sgpu_op *op, const value_t *u, const value_t *rhs, value_t *res, const value_t *w, value_t c);
/* iter damped-Jacobi sweeps, u in/out.  saena_matrix::jacobi (saena_matrix.cpp:1044-1071).
 * omega is the reference's float(2.0/3) promoted to double unless overridden. */
int sgpu_jacobi(sgpu_op *op, int iter, value_t omega, value_t *u, const value_t *rhs);
/* iter Chebyshev steps, u in/out.  saena_matrix::chebyshev (saena_matrix.cpp:1074-1131),
 * eig_max = eig_max_of_invdiagXA (saena_matrix.h:183). */
int sgpu_chebyshev(sgpu_op *op, int iter, value_t eig_max, value_t *u, const value_t *rhs);
/* *eig_max = the Chebyshev smoother's eig_max_of_invdiagXA of this operator, estimated on the device: saena_object::find_eig
 * (saena_object.cpp:572-592, lamlan_saena.h:38-59) as the host setup restates it -- min(steps, M) Lanczos steps on
 * D^-1/2 A D^-1/2 from a fixed start vector, 1.0001 x the largest eigenvalue of the tridiagonal matrix -- with the recurrence run
 * through the operator's current SpMV form and streaming kernels with fused partial sums.  steps: 1..64, or 0 for the setup's 20.
 * The value agrees with the host setup's within 1e-12 relative (not bit for bit: the dots are summed in another order) and is the
 * same bits from call to call and from process to process.  What sgpu_amg_create and sgpu_amg_set_operator expect in eig_max[l].
 * SGPU_ERR_ARG, with the reason in sgpu_last_error() and before anything is launched: a null argument, steps outside 0..64, M == 0,
 * an operator with a remote part or a context of more than one rank, an operator that is not square or has no inv_diag, a capture
 * open on the compute stream.  The call owns its work space (five vectors of M doubles) and frees it before it returns; it waits for
 * the compute stream once per step.  The operator is left as a plain sgpu_spmv leaves it: plan, plan cache, x-window mode and every
 * captured graph untouched. */
int sgpu_op_eig_max(sgpu_op *op, int steps, value_t *eig_max);
/* u -= P e: prolong_matrix::matvec followed by the correction loop of
 * saena_object::vcycle (saena_object_solve.cpp:1325,1360-1361), fused. */
int sgpu_prolong_correct(sgpu_op *P, const value_t *e_coarse, value_t *u);

/* Host-slice forms with the reference's exact signatures' meaning
 * (`const value_t *v, value_t *w` on host memory): upload, run, download,
 * wait.  PCIe-inclusive; for integration behind an unchanged caller. */
int sgpu_spmv_host(sgpu_op *op, const value_t *v_host, value_t *w_host);
int sgpu_jacobi_host(sgpu_op *op, int iter, value_t omega, value_t *u_host, const value_t *rhs_host);
int sgpu_chebyshev_host(sgpu_op *op, int iter, value_t eig_max, value_t *u_host, const value_t *rhs_host);

/* ---- multigrid hierarchy --------------------------------------------------
 * Replaces the Grid array of saena_object (include/grid.h:11-78) for the solve
 * phase: level l holds A[l] and, for l < nlevels-1, P[l] (fine rows) and R[l]
 * (coarse rows).  Work vectors (res, uCorr, res_coarse, uCorrCoarse) are
 * allocated here, once (Grid::allocate_mem, grid.cpp:165-172). */
typedef struct {
    int     preSmooth, postSmooth;        /* saena.hpp:151-155 */
    int     smoother;                     /* 0 "jacobi", 1 "chebyshev" (saena_object.tpp:5-16) */
    value_t jacobi_omega;                 /* 0 => float(2.0/3) */
    int     coarse_solver;                /* 1 (default) direct: dense inverse factored once on the host, like the reference's
                                             default direct_solver "SuperLU" (saena_object.h:165, saena_object_solve.cpp:793-958);
                                             0 CG (solve_coarsest_CG, saena_object_solve.cpp:14-114);
                                             2 device CG: value 0's LDS-resident CG, the same bits, on a coarsest level of at most
                                             1 024 rows; on a larger one that lives whole on one rank, the same recurrence with
                                             its vectors in device memory and its scalars on the device -- a fixed sequence of
                                             2 + 3 (CG_coarsest_max_iter - 1) launches without a host round trip, so the V-cycle
                                             is captured and sgpu_vcycle_block, sgpu_solve_pCG_block, sgpu_solve_FGMRES and
                                             sgpu_eigs_LOBPCG take the hierarchy.  Under 0 and 1 such a level is solved by a
                                             host-driven CG loop (no graph capture; those four entry points return SGPU_ERR_ARG).
                                             A coarsest level that is row-partitioned over the ranks takes the distributed
                                             host-driven CG under every value */
    int     CG_coarsest_max_iter;         /* 150   saena_object.h:156 */
    value_t CG_coarsest_tol;              /* 1e-12 saena_object.h:155 */
    int     solver_max_iter;              /* saena::options */
    value_t solver_tol;
    int     use_graph;                    /* 1 (default): capture the V-cycle once per (u, rhs) pair and replay it as a
                                             hipGraph.  One rank: the whole V-cycle.  Several ranks: the levels whose
                                             operators exchange a halo on this rank launch eagerly (the exchange is an RCCL
                                             group), the communication-free tail below them is one captured graph */
} sgpu_amg_params;

typedef struct sgpu_amg sgpu_amg;         /* opaque */

int sgpu_amg_default_params(sgpu_amg_params *p);
/* eig_max[l] = eig_max_of_invdiagXA of A[l] (only read for chebyshev; may be NULL) */
int sgpu_amg_create(int nlevels, sgpu_op *const *A, sgpu_op *const *P, sgpu_op *const *R,
                    const value_t *eig_max, const sgpu_amg_params *params, sgpu_amg **out);
/* A hierarchy that knows its null space.  null_space 0 is sgpu_amg_create (which is this call with 0: every bit and every launch as
 * before).  null_space 1, "constants": every level's operator is symmetric and annihilates the constant vector -- a pressure
 * Poisson problem with Neumann or periodic boundaries, a graph Laplacian.  Such a hierarchy solves A u = rhs - mean(rhs) and returns
 * the solution of zero mean, whatever the mean of rhs is (a caller learns it from sgpu_vec_center).  One rank, fp64.  The property is
 * fixed for the life of the hierarchy: sgpu_amg_params does not change and there is no setter.
 *   coarsest level, coarse_solver 1: the host stores the pseudo-inverse instead of the inverse -- the same Gauss-Jordan elimination
 *     on A_c + (s / n) 1 1^T, s the mean of A_c's diagonal, then every column and then every row of the result centred -- and the
 *     dense solve kernels run as they are, without an extra launch;
 *   coarsest level, the CG solvers (coarse_solver 0 and 2, and 1's fallback past 1 024 rows): the coarse right-hand side is centred
 *     first (three small launches; in the level's own buffer, or into a work vector where the right-hand side is the caller's).  CG
 *     from a zero iterate stays in the complement of constants, so nothing is centred after it;
 *   sgpu_solve, sgpu_solve_pCG, sgpu_solve_CG, sgpu_solve_smoother, sgpu_solve_pCG_block iterate on the centred right-hand side:
 *     res_hist[0] = ||rhs - mean(rhs)|| and the threshold is relative to it; u is centred once before they return.  Nothing is
 *     centred per iteration on level 0;
 *   sgpu_vcycle and sgpu_vcycle_block centre only at the coarsest level: they are the preconditioner, not a solve of the singular
 *     system, and return whatever mean the smoothers leave;
 *   sgpu_solve_FGMRES is refused (SGPU_ERR_ARG, "symmetric solvers only"), as are sgpu_eigs_LOBPCG, sgpu_eigs_LOBPCG_gen and
 *     sgpu_eigs_LOBPCG_many (lambda = 0 is in the spectrum).  sgpu_eigs_LOBPCG_locked is accepted and unchanged: with the normalised
 *     constant vector as its one locked column it returns the smallest nonzero pairs;
 *   sgpu_amg_set_operator repeats the check below for a new operator of level 0 or of the coarsest level and recomputes the
 *     pseudo-inverse.
 * Creation with 1 is refused with SGPU_ERR_ARG when the context has more than one rank ("one rank"), and when the operator of level 0
 * or of the coarsest level has max_i |(A 1)_i| / max_i |a_ii| > 1e-10 (computed once through sgpu_spmv on a vector of ones and a
 * download; the message names the level and the value).  The smoothed-aggregation setup keeps constants on every level to 1e-14; a
 * pinned row or a reaction term is orders above the threshold.  Any other value of null_space is SGPU_ERR_ARG.  Not covered: more than
 * one rank, null spaces other than constants (a disconnected graph passes the check above and is NOT detected), nonsymmetric singular operators.
 * A right-hand side that is constant is a zero right-hand side: rule 2 of "Degenerate right-hand sides" below. */
int sgpu_amg_create_null_space(int nlevels, sgpu_op *const *A, sgpu_op *const *P, sgpu_op *const *R,
                               const value_t *eig_max, const sgpu_amg_params *params, int null_space, sgpu_amg **out);
/* kind: the null_space the hierarchy was created with (0 for sgpu_amg_create) */
int sgpu_amg_get_null_space(const sgpu_amg *h, int *kind);
int sgpu_amg_destroy(sgpu_amg *h);       /* does not destroy the operators */
/* saena_object::vcycle (saena_object_solve.cpp:961-1431) on level 0.  On a hierarchy created with null_space 1 only the coarsest
 * solve is restricted to the complement of constants: neither rhs nor u is centred on level 0 */
int sgpu_vcycle(sgpu_amg *h, value_t *u, const value_t *rhs);
/* ---- Degenerate right-hand sides: one contract for every solve ---------------
 * sgpu_solve, sgpu_solve_smoother, sgpu_solve_CG, sgpu_solve_pCG, sgpu_solve_pCG_block (per column) and sgpu_solve_FGMRES, at every
 * rank count they support, with use_graph 0 and 1.  ||r_0||^2 is the dot of the initial residual (of the centred right-hand side
 * under null_space 1), summed over the ranks: every rank holds the same bits, takes the same branch and returns together.
 *  1. Zero.  ||r_0||^2 == 0: u = 0 (every entry +0), *iters = 0, res_hist[0] = 0.0, SGPU_OK.  After the initial residual and its dot
 *     no V-cycle, smoother sweep or matrix product is launched.
 *  2. Constant, null_space 1.  With n rows, m the mean the centring computed (its sum / n) and k the roundings on the longest path
 *     of that sum (tests/solver_ref.dot_roundings(n): the grid of sgpu_dot), a right-hand side with
 *         ||rhs - m||^2 <= n (k u |m|)^2,   u = 2^-53,
 *     is a zero right-hand side and returns rule 1's result: its centred part is not above the rounding error of its own mean
 *     (DESIGN 20 derives the bound: the centred entries of c 1 are at most k u |m| each).  The mean comes down with ||r_0||^2, in front
 *     of the same synchronisation.  Per column in the block solve.
 *  3. Non-finite.  The solve stops at the first ||r_k||^2 that is not finite (a NaN or Inf in rhs, a breakdown p.Ap = 0), k = 0
 *     included: SGPU_ERR_NOCONV, sgpu_last_error() says "non-finite residual at iteration k", *iters = k (the iterations completed),
 *     res_hist[k] holds the non-finite value and nothing further is launched (u is not centred either); for k = 0, u = 0.  In the
 *     block solve that column is frozen at that iteration (u = 0 for k = 0) and counts as failed; the other columns go on to their own
 *     thresholds with the bits they have without it, and the message names the first such column.  sgpu_solve_FGMRES tests k = 0 this
 *     way; later its Hessenberg column is not finite and it stops with its breakdown message, *iters = k.
 *  4. Nothing else moves.  For a finite non-zero right-hand side every bit of u and res_hist, every iteration count and every launch
 *     count is as without these rules: they test values the loops already hold on the host and add neither a launch nor a
 *     synchronisation.
 * res_hist is written up to entry min(*iters, hist_cap - 1) and never past hist_cap - 1; *iters does not depend on hist_cap; iters
 * and res_hist may be NULL. */
/* saena_object::solve (saena_object_solve.cpp:1883-2014): u is zeroed, then V-cycles until
 * ||r||^2 < ||r0||^2 tol^2.  res_hist[k] = ||r_k||, k = 0..iters (capacity hist_cap). */
int sgpu_solve(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters, value_t *res_hist, int hist_cap);
/* saena_object::solve_pCG (saena_object_solve.cpp:2389-2801) */
int sgpu_solve_pCG(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters, value_t *res_hist, int hist_cap);
/* saena_object::set_solve_params (called by every saena::amg::solve* before the solve, saena.cpp:751-790):
 * replaces the iteration limit, tolerance, smoother (0 jacobi, 1 chebyshev) and sweep counts of an existing
 * hierarchy.  Captured V-cycle graphs are dropped when the V-cycle shape changes. */
int sgpu_amg_set_solve_params(sgpu_amg *h, int solver_max_iter, double solver_tol, int smoother, int preSmooth, int postSmooth);
/* Replace A of one level by an operator of the same size (saena::amg::update1 / update2, src/saena_object_lazy.cpp:7-77: other
 * values, possibly another pattern).  One rank; P, R and every other level stay.  In this order: the arguments are checked --
 * level in 0..nlevels-1, A_new square with the level's M and without a remote part, inv_diag present unless this is the coarsest
 * level, eig_max > 0 under Chebyshev on a non-coarsest level, a context of one rank: anything else is SGPU_ERR_ARG; both streams are
 * waited for; EVERY captured graph of the hierarchy is dropped (the scalar cache, the multi-rank tail, the block caches, FGMRES's and
 * LOBPCG's: they hold raw pointers into the outgoing operator), so the next call of each captures again; on the coarsest level with
 * coarse_solver 1 the dense inverse is recomputed (a singular operator is SGPU_ERR_ARG; under coarse_solver 2 no inverse exists and
 * the device CG's work space is kept); the Chebyshev direction of A_new is
 * allocated, for the scalar V-cycle and for every block work space the hierarchy already has (a capture must not allocate); then
 * A[level] and eig_max[level] are swapped.  After any error the hierarchy is as it was: the old operator, the old inverse.  The work
 * vectors of the hierarchy and the block, FGMRES and LOBPCG work spaces stay (the sizes are equal); only their graphs go.  The old
 * operator is neither destroyed nor touched: as with sgpu_amg_create the caller owns the operators, and destroys the old one after
 * this call returns.  No stored SpMV form is refreshed in place: A_new comes from sgpu_op_create and the plan cache or autotune. */
int sgpu_amg_set_operator(sgpu_amg *h, int level, sgpu_op *A_new, value_t eig_max);
/* saena_object::profile_matvecs (saena_object.cpp:618-638): average time of `iter` matvecs with A of every level;
 * us_per_level[nlevels] receives microseconds (this rank, HIP events around the launches, halo included). */
int sgpu_amg_profile_matvecs(sgpu_amg *h, int iter, double *us_per_level);
/* saena_object::solve_smoother (saena_object_solve.cpp:2017-2117): preSmooth sweeps of the configured
 * smoother on A[0] per iteration, no coarse-grid correction */
int sgpu_solve_smoother(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters, value_t *res_hist, int hist_cap);
/* saena_object::solve_CG (saena_object_solve.cpp:2119-2387): plain CG on A[0], no V-cycle */
int sgpu_solve_CG(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters, value_t *res_hist, int hist_cap);
/* solve_coarsest_CG on the last level only (for tests) */
int sgpu_coarsest_solve(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters);

/* ---- block vectors: K right-hand sides through one pass over the operator --
 * A block vector of K columns over n rows is ONE device allocation of n*K doubles (sgpu_vec_alloc) with the columns
 * interleaved, X[i*K + j]; K is 2, 4 or 8, anything else is SGPU_ERR_ARG on every entry point below.  Outside the
 * library blocks travel column-major (n x K, column j at cols[j*n]); pack / unpack convert, device to device.
 * fp64 only.  The block apply, V-cycle and pCG run on any number of ranks: under a communicator (RCCL) or a host transport
 * the K columns of an operator's halo travel through ONE exchange (the scalar plan with every segment K times as long, on
 * the wire type halo_fp32 names), and the dots of the pCG are summed over the ranks.  An operator with a remote part in a
 * context that has neither is refused with SGPU_ERR_ARG ("remote part"), as is a hierarchy whose coarsest level is
 * row-partitioned over the ranks.  pack / unpack are local.
 * Every column of a block result is what the scalar entry point computes for that column alone: bit for bit the
 * reference's sequential row sum at one lane per row, within the tile kernels' bounds above that; column j never
 * reads column j'.  None of this touches the scalar path (no plan, autotune choice, plan-cache entry or scalar graph):
 * the block kernel reads the plain CSR arrays every operator keeps. */
int sgpu_block_pack(const value_t *cols_colmajor, value_t *blk, size_t n, int K);
int sgpu_block_unpack(const value_t *blk, value_t *cols_colmajor, size_t n, int K);
/* sgpu_vec_center per column of an interleaved block vector: Y = X - the column means of X, Y may be X; column j gets the bits of
 * sgpu_vec_center on that column alone.  Device only, capturable; one rank.  X and Y must be 16-byte aligned (what sgpu_vec_alloc
 * returns is): the kernels move pairs of columns; anything else is SGPU_ERR_ARG. */
int sgpu_block_center(const value_t *X, value_t *Y, size_t n, int K);
/* lanes per row of the block kernel: 0 = from the operator's mean row length (the default), or 1, 4, 16, 64.
 * (sgpu_op_set_lanes_per_row steers the scalar forms and does not reach the block kernel, nor this the scalar forms.) */
int sgpu_op_set_block_lanes(sgpu_op *op, int lanes);
int sgpu_op_get_block_lanes(const sgpu_op *op, int *lanes);
int sgpu_spmv_block(sgpu_op *op, const value_t *X, value_t *Y, int K);
int sgpu_residual_block(sgpu_op *op, const value_t *U, const value_t *RHS, value_t *RES, int K);
int sgpu_jacobi_block(sgpu_op *op, int iter, value_t omega, value_t *U, const value_t *RHS, int K);
int sgpu_chebyshev_block(sgpu_op *op, int iter, value_t eig_max, value_t *U, const value_t *RHS, int K);
int sgpu_prolong_correct_block(sgpu_op *P, const value_t *E_coarse, value_t *U, int K);
/* sgpu_vcycle on K columns: the same steps on block vectors (work vectors made at the first call with this K, freed with
 * the hierarchy; with use_graph captured once per (U, RHS, K)).  A hierarchy whose coarsest level needs the host-driven CG
 * (more rows than the LDS-resident solvers hold) is refused with SGPU_ERR_ARG.  As sgpu_vcycle, a hierarchy created with
 * null_space 1 centres only at the coarsest level (every column on its own). */
int sgpu_vcycle_block(sgpu_amg *h, value_t *U, const value_t *RHS, int K);
/* sgpu_solve_pCG's recurrence on K columns in lockstep, every column with its own scalars and threshold.  A column stops
 * at the iteration at which its ||r||^2 drops below its own threshold and is not written again; iters[j] and
 * res_hist[j*hist_cap + k] are those of a scalar solve of column j, a zero, constant or non-finite column included ("Degenerate
 * right-hand sides" above).  SGPU_ERR_NOCONV if any column is still above its threshold after solver_max_iter iterations or
 * met a non-finite residual (all other iterates stay valid).  One host synchronisation per iteration. */
int sgpu_solve_pCG_block(sgpu_amg *h, value_t *U, const value_t *RHS, int K,
                         int *iters /*[K]*/, value_t *res_hist /*[K][hist_cap]*/, int hist_cap);

/* ---- restarted flexible GMRES ------------------------------------------------
 * For operators that are not symmetric positive definite, where sgpu_solve_pCG is not defined.  Right-preconditioned and flexible
 * (the preconditioned vectors are stored), so a V-cycle that is not a fixed linear map -- the CG coarsest solver, a Chebyshev
 * smoother -- is a valid preconditioner.  restart: 1..64 inner iterations per cycle; precond 1: one V-cycle from a zero iterate,
 * exactly what sgpu_solve_pCG applies; precond 0: none (plain restarted GMRES).  u starts from zero.  res_hist[0] = ||r_0||,
 * res_hist[k] = the Givens estimate of ||r_k|| after inner iteration k; the threshold is ||r_0||^2 tol^2 as in sgpu_solve_pCG.  At
 * the end of every cycle rhs - A u is recomputed; only that recomputed norm (*true_res, may be NULL) declares convergence, and
 * another cycle starts when the estimate was optimistic.  *iters counts inner iterations (at most solver_max_iter).  A zero
 * right-hand side returns u = 0, 0 iterations, SGPU_OK.  SGPU_ERR_NOCONV: not converged within solver_max_iter, or a breakdown
 * (u holds the last completed cycle).  One rank; a hierarchy that needs the host-driven coarsest CG or an operator with a remote
 * part is refused with SGPU_ERR_ARG.  The work space (2 restart + 3 vectors) is allocated at the first call with a given restart
 * length and freed with the hierarchy; sgpu_solve_pCG's vectors and the cache of captured V-cycles are not touched.  One host
 * synchronisation per inner iteration. */
int sgpu_solve_FGMRES(sgpu_amg *h, value_t *u, const value_t *rhs, int restart, int precond,
                      int *iters, value_t *res_hist, int hist_cap, value_t *true_res);

/* ---- LOBPCG: the smallest eigenpairs of the level-0 operator ------------------
 * Standard problem A x = lambda x for the symmetric positive definite level-0 operator of a hierarchy, by LOBPCG on a block of K
 * vectors (K = 2, 4 or 8), preconditioned by one block V-cycle from a zero iterate -- exactly what sgpu_solve_pCG_block applies
 * (precond 1), or by nothing (precond 0: W = R).  X is a block vector X[i*K + j] (16-byte aligned): on entry the start vectors, which
 * must be linearly independent; on return the eigenvectors, orthonormal, columns in ascending order of lambda.  The caller asks for the
 * nev smallest pairs, 1 <= nev <= K; columns nev .. K-1 are guard vectors: iterated and returned, not required to converge.  nev
 * should end at a gap of the spectrum, not inside a cluster of equal eigenvalues: the convergence of column j is governed by the gap
 * to the first eigenvalue outside the block, and a cluster cut in two converges slowly.
 * Column j is converged when ||A x_j - lambda_j x_j|| < tol lambda_j; converged columns stay in the Rayleigh-Ritz basis and stop
 * contributing search directions (soft locking).  The solve ends when columns 0 .. nev-1 are converged; then A X is recomputed and only
 * the recomputed norms declare convergence -- when they contradict the carried ones and iterations remain, the iteration goes on.
 * lambda[K], res[K] (may be NULL; the last recomputed ||r_j||) and res_hist[j*hist_cap + k] (may be NULL; ||r_j|| at the start of
 * iteration k) are host arrays; *iters = completed iterations.
 * SGPU_ERR_ARG: K outside {2, 4, 8}, nev outside 1..K, fewer than 3 K rows, more than one rank, an operator with a remote part, a
 * hierarchy that needs the host-driven coarsest CG, linearly dependent start vectors.  SGPU_ERR_NOCONV: not converged after max_iter
 * iterations (X, lambda, res are those of the last iteration); a breakdown (the preconditioned residuals of the active columns are
 * linearly dependent; X and lambda of the last completed iteration stay valid); a Ritz value <= 0 (the operator is not SPD).
 * The work space (six block vectors) is allocated at the first call with a given K and freed with the hierarchy; the V-cycle runs
 * through one fixed pair of them in a captured graph of its own, outside the block cache of eight.  Three host synchronisations per
 * iteration, each of at most 12 K^2 + K doubles.  The generalised problem A x = lambda B x: sgpu_eigs_LOBPCG_gen below. */
int sgpu_eigs_LOBPCG(sgpu_amg *h, value_t *X, int K, int nev, int max_iter, value_t tol, int precond,
                     value_t *lambda /*[K] host*/, value_t *res /*[K] host: recomputed ||r_j||*/, int *iters,
                     value_t *res_hist /*[K][hist_cap]*/, int hist_cap);

/* ---- LOBPCG: the generalised problem A x = lambda B x --------------------------
 * As sgpu_eigs_LOBPCG, with a second symmetric positive definite operator B of the size of the level-0 operator A (a mass matrix,
 * consistent or lumped; one rank, no remote part): every inner product of the algorithm is the B-inner product, and B X, B W, B P are
 * carried next to A X, A W, A P (one more block SpMV, with B, per iteration).  The preconditioner is the same block V-cycle of A, in
 * the same captured graph as the standard solve's: a generalised call neither drops nor recaptures it.
 * On return X is B-orthonormal (X^T B X = I) and lambda ascends.  Column j is converged when
 * ||A x_j - lambda_j B x_j|| < tol lambda_j ||B x_j|| -- the relative backward error, which does not change when B is rescaled and is
 * sgpu_eigs_LOBPCG's criterion for B = I.  At the end of the solve A X and B X are recomputed and only the recomputed norms declare
 * convergence; res[j] (may be NULL) is the last recomputed ||A x_j - lambda_j B x_j||, res_hist as above.
 * B is applied by eager launches only and never enters a captured graph; nothing keeps a pointer to it after the call returns: the
 * caller may destroy it, or pass another B to the next call on the same hierarchy.
 * SGPU_ERR_ARG: everything sgpu_eigs_LOBPCG refuses; a null B; a B whose rows or columns differ from A's; a B with a remote part or a
 * halo plan; a start Gram matrix X^T B X that is not numerically positive definite (dependent start vectors, or a B that is not
 * positive definite).  SGPU_ERR_NOCONV: as sgpu_eigs_LOBPCG, and a W^T B W, an S^T B S or a Ritz value that shows that B or A is not
 * SPD.  The extra work space (three block vectors, the partial sums and the K sums of ||B x_j||^2) is allocated at the first
 * generalised call with a given K and freed with the hierarchy; a process that only calls sgpu_eigs_LOBPCG allocates none of it.
 * Three host synchronisations per iteration, of at most 12 K^2 + 2 K doubles. */
int sgpu_eigs_LOBPCG_gen(sgpu_amg *h, sgpu_op *B, value_t *X, int K, int nev, int max_iter, value_t tol, int precond,
                         value_t *lambda /*[K] host*/, value_t *res /*[K] host: recomputed ||A x_j - lambda_j B x_j||*/, int *iters,
                         value_t *res_hist /*[K][hist_cap]*/, int hist_cap);

/* ---- LOBPCG with hard locking: more than K eigenpairs ---------------------------
 * sgpu_eigs_LOBPCG_locked is the block solve above constrained to the B-orthogonal complement of `nlocked` <= 64 locked vectors: the
 * standard problem with B = NULL, the generalised one otherwise.  The locked set is COLUMN-MAJOR on the device, column l at
 * Q + l * ld, ld >= n and even; BQ (read only when B is given) holds B Q the same way.  The loop is the unconstrained one with two
 * additions: X <- X - Q (Z^T X) twice before the start orthonormalisation, and W <- W - Q (Z^T W) once right after W = M R (Z = Q, or
 * BQ); the convergence rule, soft locking, the recomputed norms at the end, the breakdown handling and the three host
 * synchronisations per iteration are unchanged (the coefficients Z^T W never visit the host).  *leading (may be NULL): how many
 * leading columns 0 .. leading-1 are converged on the recomputed norms; 0 when the solve ended without recomputing them.
 * With nlocked = 0 no lock kernel is launched and X, lambda, res, iters, res_hist have the bits of sgpu_eigs_LOBPCG (B = NULL) or
 * sgpu_eigs_LOBPCG_gen.  The V-cycle runs through the same captured graph; a locked call neither drops nor recaptures it.
 * SGPU_ERR_ARG, besides what those two refuse: nlocked outside 0..64, ld < n or odd, a null Q with nlocked > 0, a null BQ with B given
 * and nlocked > 0, n < nlocked + 3 K.
 *
 * sgpu_eigs_LOBPCG_many sweeps it: while fewer than nev (1..64) pairs are locked, a constrained solve for min(sweep_nev, nev - locked)
 * pairs (1 <= sweep_nev <= K; 0: K / 2, half the block as guard vectors); ALL leading converged columns are locked (copied into Q,
 * and their B x into an array the driver owns), the others stay in the block as the next start vectors, the freed columns are
 * refilled from a deterministic generator on the device.  X0: K start columns (block vector, device), or NULL for generated ones.
 * max_iter bounds the TOTAL iterations over all sweeps, *iters reports that total.  On return lambda[nev], res[nev] (may be NULL; the
 * recomputed norms at locking time) and the columns of Q (device, nev columns of ld) are in ascending order of lambda (a stable sort;
 * Q is permuted on the device) and Q is B-orthonormal.  There is no locking inside a sweep and no final Rayleigh-Ritz over Q.
 * SGPU_ERR_NOCONV: max_iter ran out (or a sweep broke down); the *nlocked_out pairs locked so far are valid, sorted among themselves.
 * SGPU_ERR_ARG: nev outside 1..64, sweep_nev outside 0..K, ld < n or odd, n < nev + 3 K, and what the block solves refuse.
 * Work space: the lock partial sums and the coefficient buffer (about 4 MiB) are made at the first locked call and freed with the
 * hierarchy; the driver's block, B Q and permutation copy are freed at return.  A process that calls neither allocates none of it. */
int sgpu_eigs_LOBPCG_locked(sgpu_amg *h, sgpu_op *B /*or NULL*/, const value_t *Q, const value_t *BQ, size_t ld, int nlocked,
                            value_t *X, int K, int nev, int max_iter, value_t tol, int precond,
                            value_t *lambda /*[K] host*/, value_t *res /*[K] host*/, int *iters,
                            value_t *res_hist /*[K][hist_cap]*/, int hist_cap, int *leading);
int sgpu_eigs_LOBPCG_many(sgpu_amg *h, sgpu_op *B /*or NULL*/, value_t *Q /*device, nev columns of ld*/, size_t ld, int nev, int K,
                          int sweep_nev, const value_t *X0 /*device block vector, or NULL*/, int max_iter, value_t tol, int precond,
                          value_t *lambda /*[nev] host*/, value_t *res /*[nev] host*/, int *iters, int *nlocked_out, int *sweeps_out);

/* ---- measurement -----------------------------------------------------------
 * Runs `reps` back-to-back launches of one kernel on the compute stream,
 * bracketed by hipEvents recorded on that same stream; *ms_per_launch is the
 * mean.  kind: 0 spmv, 1 jacobi sweep, 2 residual, 3 chebyshev step. */
int sgpu_time_kernel(sgpu_op *op, int kind, const value_t *x, const value_t *rhs, value_t *y,
                     int reps, float *ms_per_launch);
/* algorithmic bytes of one launch of `kind` on this operator */
int sgpu_algorithmic_bytes(const sgpu_op *op, int kind, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* SAENA_GPU_H */
