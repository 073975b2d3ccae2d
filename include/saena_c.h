/*
 * saena_c.h -- flat C view of the host-side mirror of Saena's public surface
 * (include/saena.hpp in this repository; reference: include/saena.hpp:14-265).
 *
 * The reference's users write C++ (saena::matrix A(comm); A.set(...);
 * A.assemble(); saena::amg s; s.set_matrix(&A,&opts); s.solve_pCG(u,&opts)).
 * This header exposes the same steps with plain pointers so that ctypes / cgo
 * style callers -- and this repository's tests and bench.py -- can drive them.
 * Host-only functions live in libsaena_host.so (no GPU needed) and again in
 * libsaena_amd.so; functions marked [GPU] exist only in libsaena_amd.so.
 * All return 0 on success, negative on error (saena_last_error() has the text).
 */
#ifndef SAENA_C_H
#define SAENA_C_H

#include "saena_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *saena_last_error(void);

/* ---- communicator for the setup-time exchanges (the reference: MPI_Comm) ---- */
typedef struct saena_comm saena_comm;
typedef int (*saena_cb_allgather)(void *user, const void *send, void *recv, size_t bytes);
typedef int (*saena_cb_alltoallv)(void *user, const void *send, const size_t *scounts, const size_t *sdispls,
                                  void *recv, const size_t *rcounts, const size_t *rdispls);
typedef int (*saena_cb_allreduce_i64)(void *user, long *v, int n);
typedef int (*saena_cb_allreduce_f64)(void *user, double *v, int n);

saena_comm *saena_comm_self(void);
saena_comm *saena_comm_callbacks(int rank, int nranks, void *user, saena_cb_allgather, saena_cb_alltoallv,
                                 saena_cb_allreduce_i64, saena_cb_allreduce_f64);
saena_comm *saena_comm_rccl(void);            /* [GPU] the sgpu_init() communicator */
/* the ranks of ONE node through POSIX shared memory (host/shm_comm.h): native, no interpreter and no device in the loop;
 * collective over the job's ranks, `name` fresh for every job (no '/'); NULL + saena_last_error() on failure */
saena_comm *saena_comm_shm(const char *name, int rank, int nranks);
void        saena_comm_free(saena_comm *);
/* the exchange chain of a multi-rank apply that the agglomeration of coarse levels starts from, microseconds: measured by the
 * GPU runtime on the job's communicator at sgpu_init (0: nothing measured, the model's constant applies) */
double      saena_measured_chain_us(void);
/* the communicator's collectives, exported for its tests (counts and displacements in bytes, one per rank) */
int saena_comm_test_alltoallv(saena_comm *, const void *send, const size_t *scounts, const size_t *sdispls, void *recv,
                              const size_t *rcounts, const size_t *rdispls);
int saena_comm_test_allreduce_f64(saena_comm *, double *v, int n);
int saena_comm_test_allreduce_i64(saena_comm *, long *v, int n);

/* ---- saena::matrix (reference include/saena.hpp:14-73) ---- */
typedef struct saena_matrix_h saena_matrix_h;
saena_matrix_h *saena_matrix_new(saena_comm *comm);
void  saena_matrix_free(saena_matrix_h *A);
int   saena_matrix_set(saena_matrix_h *A, index_t i, index_t j, value_t val);                       /* saena.hpp:29 */
int   saena_matrix_set_many(saena_matrix_h *A, const index_t *row, const index_t *col, const value_t *val, nnz_t n); /* :30 */
int   saena_matrix_read_file(saena_matrix_h *A, const char *name, const char *input_type /* "" */);     /* saena.hpp:25-26 */
int   saena_matrix_write_bin(saena_matrix_h *A, const char *name);
int   saena_matrix_write_mtx(saena_matrix_h *A, const char *name);   /* saena.hpp:53 writeMatrixToFile: "<name>-r<rank>.mtx" */
int   saena_matrix_set_remove_boundary(saena_matrix_h *A, int remove_bound);                        /* :44 */
/* resolution of the nnz-balanced row partition of assemble(): 0 = the reference's nparts^2 row buckets
   (src/saena_matrix_repart.cpp:43-170; max / mean rows 1.25 at 4 ranks, 1.125 at 8 on a uniform operator), n > 0 = at least n
   buckets -- opt-in, NOT the reference's partition (also: SAENA_FINE_PARTITION_BUCKETS) */
int   saena_matrix_set_partition_buckets(saena_matrix_h *A, int n_buckets);
int   saena_matrix_add_duplicates(saena_matrix_h *A, int add);                                      /* :47 */
int   saena_matrix_set_eig(saena_matrix_h *A, double eig);                                          /* :38 (value form) */
/* [GPU] the value saena_matrix_set_eig takes, estimated on the device (sgpu_op_eig_max, include/saena_gpu.h: the setup's Lanczos
 * recurrence, `steps` of them, 0 = the setup's 20) for an assembled matrix on one rank; within 1e-12 relative of what the host setup
 * computes.  Nothing is stored: pass the value to saena_matrix_set_eig and saena_amg_update(A, 1) runs no host Lanczos.  The device
 * operator is made for the call (sgpu_op_create) and destroyed. */
int   saena_matrix_estimate_eig(saena_matrix_h *A, int steps, double *eig_max);
int   saena_matrix_assemble(saena_matrix_h *A);                                                     /* :49 */
int   saena_matrix_assemble_with_split(saena_matrix_h *A, const index_t *split);
index_t saena_matrix_get_num_rows(saena_matrix_h *A);                                               /* :57 */
index_t saena_matrix_get_num_local_rows(saena_matrix_h *A);                                         /* :58 */
nnz_t   saena_matrix_get_nnz(saena_matrix_h *A);                                                    /* :59 */
nnz_t   saena_matrix_get_local_nnz(saena_matrix_h *A);                                              /* :60 */
int   saena_matrix_get_split(saena_matrix_h *A, index_t *split_out /* nranks+1 */);
/* this rank's arrays in the reference's storage layout; pointers stay valid while A lives */
int   saena_matrix_get_desc(saena_matrix_h *A, sgpu_op_desc *out);
/* remaining layout arrays not part of sgpu_op_desc, for layout tests: col_remote[nnz_l_remote], nnzPerProcScan[nranks+1] */
int   saena_matrix_get_layout_extra(saena_matrix_h *A, const index_t **col_remote, const nnz_t **nnzPerProcScan);
/* global column id of every slot of the receive (halo) buffer, [col_remote_size] -- vElement_remote (saena_matrix.h:57) */
int   saena_matrix_get_halo_columns(saena_matrix_h *A, const index_t **vElement_remote);

/* generators (reference src/aux_functions2.cpp:254-373, :629-700, :1296-1381) */
int   saena_laplacian3D(saena_matrix_h *A, index_t mx, index_t my, index_t mz);
/* rhs of the assembled interior system, this rank's slice (length get_num_local_rows) */
int   saena_laplacian3D_set_rhs(saena_matrix_h *A, index_t mx, index_t my, index_t mz, value_t *rhs_local);
int   saena_band_matrix(saena_matrix_h *A, index_t M, unsigned int bandwidth);

/* saena::amg::matmat (reference saena.hpp:313, saena_object_setup_matmat.cpp:1164-1487): C = A B on the host,
 * A and B assembled, one rank in this round; C (a fresh handle's contents are replaced) is assembled on return */
int   saena_matmat(saena_matrix_h *A, saena_matrix_h *B, saena_matrix_h *C);

/* ---- tests: the sparse product of the setup from plain arrays, and which path served it ----
 * C = A B with A (a_rows x b_rows) and B (b_rows x b_cols) in CSR (64-bit row pointers), through the code the setup
 * multiplies with.  row_offset: global id of row 0 of A (an entry survives iff |c_ij| > 1e-14 or i + row_offset == j).
 * B in one piece (b_col1 == NULL), or in two as the distributed setup holds it: entries [0, b_split) at b_col / b_val,
 * entries [b_split, b_ptr[b_rows]) at b_col1 / b_val1, b_split a row boundary.
 * PRECONDITION, checked here (an error, nothing runs): the columns of every row of B are distinct and ascending and
 * below b_cols, the columns of A are rows of B.  Rows of A may repeat a column and come in any order.
 * mode 0: what the setup does (the device kernel from 200 000 stored entries on where libsaena_amd.so has a context,
 *         the host kernel when it declines or below);
 *      1: the host kernel, whatever is installed;
 *      2: [GPU] the device kernel whatever the size; a missing or declining device kernel is an error, not a host product.
 * *c_nnz = entries of C; saena_debug_spgemm_result copies C out: c_ptr[a_rows + 1], c_col / c_val[*c_nnz], rows ascending
 * by column.
 * saena_debug_spgemm_stats: counters of the LAST product into last[], their sums over every product (the setup's
 * included) since saena_debug_spgemm_stats_reset into total[]; either may be NULL; returns the number of counters, in
 * this order (host.SPGEMM_STATS): host kernel rows on the dense accumulator, on the hash accumulator, rehash steps;
 * device rows on light, medium, medium-try kept, medium-try abandoned, LDS accumulator, HBM accumulator; chunks; column
 * windows of the LDS accumulator; 1 if the device kernel declined; 1 if the result is the device kernel's. */
int  saena_debug_spgemm(int mode, index_t a_rows, index_t b_rows, index_t b_cols, const nnz_t *a_ptr, const index_t *a_col,
                        const value_t *a_val, const nnz_t *b_ptr, const index_t *b_col, const value_t *b_val, nnz_t b_split,
                        const index_t *b_col1, const value_t *b_val1, index_t row_offset, nnz_t *c_nnz);
int  saena_debug_spgemm_result(nnz_t *c_ptr, index_t *c_col, value_t *c_val);
int  saena_debug_spgemm_stats(long *last, long *total);
void saena_debug_spgemm_stats_reset(void);

/* ---- tests: the filter of the setup on a CSR block from plain arrays ----
 * Rows [row_offset, row_offset + n) of a level (64-bit row pointers, global column ids, the columns of every row distinct
 * and ascending -- checked here): off-diagonal entries with |v| <= thre leave the row and their sum, added up in row order,
 * is added to the diagonal once; a diagonal that ends below 1e-14 in magnitude becomes 1.0; a row without a diagonal entry
 * gets one of value 1.0 at its place in column order.  *c_nnz = entries kept; saena_debug_filter_result copies the block
 * out: c_ptr[n + 1], c_col / c_val[*c_nnz]. */
int  saena_debug_filter(index_t n, const nnz_t *ptr, const index_t *col, const value_t *val, double thre, index_t row_offset,
                        nnz_t *c_nnz);
int  saena_debug_filter_result(nnz_t *c_ptr, index_t *c_col, value_t *c_val);

/* ---- transfer operators (prolong_matrix / restrict_matrix) ---- */
typedef struct saena_transfer_h saena_transfer_h;
/* rows/cols are GLOBAL ids of this rank's fine rows; split_row = fine partition, split_col = coarse partition */
saena_transfer_h *saena_prolong_new(saena_comm *comm, index_t Mbig, index_t Nbig, const index_t *split_row,
                                    const index_t *split_col, const index_t *row, const index_t *col,
                                    const value_t *val, nnz_t n);
saena_transfer_h *saena_restrict_from_prolong(saena_transfer_h *P);       /* restrict_matrix::transposeP */
void  saena_transfer_free(saena_transfer_h *T);
int   saena_transfer_get_desc(saena_transfer_h *T, sgpu_op_desc *out);
nnz_t saena_transfer_get_local_nnz(saena_transfer_h *T);

/* ---- saena::options + saena::amg (reference include/saena.hpp:127-265) ---- */
typedef struct {
    int    solver_max_iter;      /* saena.hpp:151-155 defaults: 100, 1e-8, "chebyshev", 3, 3, "jacobi", 0.3, true, 10, 3, */
    double relative_tol;         /*                             1e-14, 1e-8, 1, 2, false, 0.1, 5000                       */
    int    smoother;             /* 0 "jacobi", 1 "chebyshev" */
    int    preSmooth, postSmooth;
    float  connStrength;
    int    dynamic_levels;
    int    max_level;
    int    float_level;
    double filter_thre, filter_max;
    int    filter_start, filter_rate;
    int    switch_to_dense;      /* saena.hpp:146-148: store levels denser than dense_thre (and smaller than dense_sz_thre rows) */
    float  dense_thre;           /* as dense row-major arrays -- saena_matrix_dense; off in every options file of the reference */
    int    dense_sz_thre;
} saena_options_c;
int saena_options_default(saena_options_c *o);
int saena_options_from_file(const char *xml_name, saena_options_c *o);   /* saena::options(const string&), saena.cpp:444-546 */

typedef struct saena_amg_h saena_amg_h;
saena_amg_h *saena_amg_new(void);
void  saena_amg_free(saena_amg_h *S);
/* saena::amg::set_matrix (saena.hpp:202): smoothed-aggregation setup on the host */
int   saena_amg_set_matrix(saena_amg_h *S, saena_matrix_h *A, const saena_options_c *opts);
/* saena::amg::update1 / update2 (saena.hpp, src/saena_object_lazy.cpp:7-77): A_new -- assembled, as many rows as the matrix of
 * set_matrix, its values and even its pattern free -- becomes level 0 of the hierarchy S already holds.  One rank.
 * mode 1: nothing else changes.  mode 2: every coarse operator is rebuilt as R A P over the kept aggregates and transfer
 * operators (the setup's own products, filter schedule and eig_max estimate); the number of levels stays.  The caller keeps A_new
 * alive and may free the old matrix.  [GPU] After saena_amg_to_device the refreshed levels (level 0; every level for mode 2)
 * get new device operators, made as to_device makes them and installed with sgpu_amg_set_operator; saena_amg_device_op(S, l, 0)
 * returns new handles for them, (S, l, 1 | 2) the same P and R as before.  Refused, with the hierarchy on the host and on the
 * device exactly as it was: no set_matrix yet, a hierarchy over more than one rank ("one rank"), A_new not assembled or of
 * another size, another mode, a coarsest operator the direct solve cannot factor. */
int   saena_amg_update(saena_amg_h *S, saena_matrix_h *A_new, int mode);
/* Opt-in, before saena_amg_set_matrix or saena_amg_update: on != 0 lets the one-rank setup and the updates take every level's eig_max
 * (Chebyshev smoother) from the device estimate instead of the host Lanczos loop -- the same recurrence, equal within 1e-12 relative,
 * not bit for bit.  Also on with SAENA_DEVICE_EIG=1 in the environment (read at every call).  Off by default.  Where no device context
 * exists (libsaena_host.so, no sgpu_init), over several ranks, or when the device declines (memory), the host loop runs as before.  A
 * value set with saena_matrix_set_eig is kept either way. */
int   saena_amg_set_device_eig(saena_amg_h *S, int on);
/* Before saena_amg_to_device: how the device hierarchy solves its coarsest level (sgpu_amg_params.coarse_solver, include/saena_gpu.h).
 * name: "direct" (the default: dense inverse), "cg" (solve_coarsest_CG) or "device_cg" (that CG, and on a coarsest level of more than
 * 1 024 rows the device-resident CG instead of the host-driven loop the other two run there: the V-cycle stays a captured graph and
 * the block, FGMRES and LOBPCG solves take the hierarchy); any other name is refused (-1).  SAENA_COARSE_SOLVER=direct|cg|device_cg in
 * the environment, read by saena_amg_to_device, overrides it for drivers compiled unchanged.  Exported like every other symbol
 * (host/exports.map hides the operator new wrappers only). */
int   saena_amg_set_coarse_solver(saena_amg_h *S, const char *name);
/* Before saena_amg_to_device, one rank: name "constant" makes the device hierarchy one that knows the constant null space
 * (sgpu_amg_create_null_space with 1, include/saena_gpu.h): the solves solve A u = rhs - mean(rhs) and return the solution of zero
 * mean; saena_amg_eigs returns the smallest nonzero pairs (the normalised constant vector is locked); saena_amg_eigs_gen,
 * saena_amg_eigs_many and saena_amg_solve_pFGMRES pass the library's refusal through, and saena_amg_to_device its refusal of an
 * operator that does not annihilate constants or of more than one rank.  "none" (the default) is the hierarchy as it always was; any
 * other name is refused (-1).  Assemble such a matrix after saena_matrix_set_remove_boundary(A, 0). */
int   saena_amg_set_null_space(saena_amg_h *S, const char *name);
int   saena_amg_num_levels(saena_amg_h *S);                               /* max_level + 1 */
/* coarse id of every fine row of `level` (the reference's `aggregate` after aggregate_index_update, src/saena_object_setup1.cpp:
 * 2103-2260); one-rank setups keep it, for the pins of the setup (tests/test_sa_pins.py).  out: rows of that level */
int saena_amg_level_aggregates(saena_amg_h *, int level, index_t *out, index_t *n_aggregates);
int   saena_amg_level_info(saena_amg_h *S, int level, index_t *rows, nnz_t *nnzA, nnz_t *nnzP, double *eig_max);
int   saena_amg_level_split(saena_amg_h *S, int level, index_t *split_out /* nranks+1 */);   /* row partition of a level */
/* which: 0 = A_l, 1 = P_l, 2 = R_l (this rank's share when the communicator has more than one rank) */
int   saena_amg_level_desc(saena_amg_h *S, int level, int which, sgpu_op_desc *out);
/* [GPU] upload every level (sgpu_op_create) and build the device hierarchy (sgpu_amg_create) */
int   saena_amg_to_device(saena_amg_h *S);
sgpu_amg *saena_amg_device_handle(saena_amg_h *S);                        /* [GPU] valid after to_device */
sgpu_op  *saena_amg_device_op(saena_amg_h *S, int level, int which);      /* [GPU] */
/* [GPU] saena::amg::solve / solve_pCG (saena.hpp:220,224) on HOST slices of this rank: rhs in, u out */
int   saena_amg_solve(saena_amg_h *S, const value_t *rhs_host, value_t *u_host, int *iters, value_t *res_hist, int hist_cap);
int   saena_amg_solve_pCG(saena_amg_h *S, const value_t *rhs_host, value_t *u_host, int *iters, value_t *res_hist, int hist_cap);
/* [GPU] solve_pCG for K = 2, 4 or 8 right-hand sides through one pass over every operator (sgpu_solve_pCG_block; any number of ranks:
 * the K columns of every halo cross in one exchange, the dots are summed over the ranks):
 * rhs_host / u_host are column-major n x K (column j at [j*n]), iters[K], res_hist[K][hist_cap] */
int   saena_amg_solve_pCG_block(saena_amg_h *S, const value_t *rhs_host, value_t *u_host, int K, int *iters, value_t *res_hist, int hist_cap);
/* [GPU] restarted flexible GMRES for operators that are not symmetric positive definite (sgpu_solve_FGMRES; one rank): restart in
 * 1..64, precond 1 = one V-cycle per iteration, 0 = none; iters counts inner iterations, res_hist[k] is the residual estimate */
int   saena_amg_solve_pFGMRES(saena_amg_h *S, const value_t *rhs_host, value_t *u_host, int restart, int precond, int *iters, value_t *res_hist, int hist_cap);
/* [GPU] the nev smallest eigenpairs of the assembled (symmetric positive definite) matrix by LOBPCG on K = 2, 4 or 8 vectors
 * (sgpu_eigs_LOBPCG; one rank), precond 1 = one block V-cycle per iteration, 0 = none.  x0_host: column-major n x K start vectors,
 * or NULL for the default start (a fixed LCG sequence over the row index in (-1, 1), one stream per column).  lambda[K] ascending,
 * x_host column-major n x K (the eigenvectors; columns nev .. K-1 are guard vectors), res[K] = ||A x_j - lambda_j x_j|| (may be NULL).
 * nev should end at a gap of the spectrum, not inside a cluster of equal eigenvalues.  SGPU_ERR_NOCONV: the outputs are still written */
int   saena_amg_eigs(saena_amg_h *S, const value_t *x0_host, int K, int nev, int max_iter, value_t tol, int precond,
                     value_t *lambda, value_t *x_host, value_t *res, int *iters);
/* [GPU] the same for the generalised problem A x = lambda B x (sgpu_eigs_LOBPCG_gen; one rank): B is an assembled symmetric positive
 * definite matrix of A's size (a mass matrix, consistent or lumped); its device operator is made for the call and destroyed before it
 * returns.  On return the columns of x_host are B-orthonormal, lambda ascends, res[K] = ||A x_j - lambda_j B x_j|| (may be NULL);
 * column j is converged when that norm is below tol lambda_j ||B x_j||.  The preconditioner is the V-cycle of A, as above.
 * A LUMPED (diagonal) B must be assembled after saena_matrix_set_remove_boundary(B, 0): saena_matrix_assemble otherwise takes every
 * single-entry row for a boundary node and removes it; a B whose rows differ from A's is refused (-1) with a message that says so */
int   saena_amg_eigs_gen(saena_amg_h *S, saena_matrix_h *B, const value_t *x0_host, int K, int nev, int max_iter, value_t tol, int precond,
                         value_t *lambda, value_t *x_host, value_t *res, int *iters);
/* [GPU] more than K eigenpairs (sgpu_eigs_LOBPCG_many; one rank): the nev <= 64 smallest pairs of A x = lambda x (B NULL) or
 * A x = lambda B x (B as in saena_amg_eigs_gen) by sweeps of the block solve on K = 2, 4 or 8 vectors with converged vectors locked.
 * sweep_nev: pairs asked of one sweep, 1..K, or 0 for K / 2.  x0_host: column-major n x K start vectors, or NULL for generated ones.
 * max_iter bounds the TOTAL iterations over all sweeps; *iters is that total, *sweeps the number of sweeps.  lambda[nev] ascending,
 * q_host column-major n x nev (B-orthonormal), res[nev] (may be NULL) the recomputed residual norms at locking time; *nlocked pairs
 * are written: nev, or fewer with SGPU_ERR_NOCONV (the pairs locked so far are valid) */
int   saena_amg_eigs_many(saena_amg_h *S, saena_matrix_h *B, int nev, int K, int sweep_nev, const value_t *x0_host, int max_iter, value_t tol,
                          int precond, value_t *lambda, value_t *q_host, value_t *res, int *iters, int *nlocked, int *sweeps);

/* ---- tests: the dense generalised symmetric eigenproblem of the Rayleigh-Ritz step (host/dense_eig.cpp) ----
 * A v = w B v for symmetric A and symmetric positive definite B of order 1 <= n <= 24, row-major: w[n] ascending, V[i * n + k] =
 * component i of vector k, V^T B V = I.  Cholesky of B with a relative pivot test, then cyclic Jacobi on L^-1 A L^-T.
 * -1: B is not numerically positive definite (reported, not factored), -2: the Jacobi iteration failed, -3: n out of range,
 * -4: null argument.  saena_debug_sym_geig_sweeps: the Jacobi sweeps the last successful call on this thread took. */
int   saena_debug_sym_geig(int n, const double *A, const double *B, double *w, double *V);
int   saena_debug_sym_geig_sweeps(void);

#ifdef __cplusplus
}
#endif
#endif
