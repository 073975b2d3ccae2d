// saena.hpp -- the public C++ surface of Saena, kept for the MI355X path.
//
// Mirrors the reference's include/saena.hpp:14-265 (classes saena::matrix, saena::vector,
// saena::options, saena::amg and the generator functions of include/aux_functions2.h:12-43) with
// the same method names, argument meaning and defaults, and the index_t / nnz_t / value_t typedefs
// of include/data_struct.h:36-38, so that a driver such as experiments/Poisson.cpp ports by
// replacing `MPI_Comm` with `saena::comm` -- or, unchanged, by including include/saena_mpi.hpp instead
// (MPI_Comm overloads; tests/test_cpp_surface.py compiles the reference's flow against it).  Only the members on (or feeding) the V-cycle hot path
// are provided (update1 / update2 of the lazy-update path among them); update3, PETSc bridges etc. are out of scope; solve_GMRES / solve_pGMRES mirror the reference's compiled-out bodies.
//
// Differences from the reference, all at the boundary:
//   * the communicator is the GPU runtime's (one process = one rank = one MI355X, RCCL), wrapped
//     in saena::comm; saena::init()/finalize() replace MPI_Init/MPI_Finalize;
//   * matvec / solve / solve_pCG run on the GPU through the C ABI of include/saena_gpu.h; there is
//     no CPU fallback (calls fail with a message when no MI355X is visible);
//   * errors throw std::runtime_error instead of printf + exit(EXIT_FAILURE).
#pragma once
#include <string>
#include <vector>

typedef int    index_t;   // Saena index type    (data_struct.h:36)
typedef long   nnz_t;     // Saena nonzero type  (data_struct.h:37)
typedef double value_t;   // Saena value type    (data_struct.h:38)

namespace saena_host { class saena_matrix; class amg_hierarchy; struct Comm; }
struct sgpu_op;
struct sgpu_amg;

namespace saena {

// replaces MPI_Init / MPI_Comm_rank / MPI_Comm_size / MPI_Finalize
// rccl_unique_id: 128 bytes from saena::unique_id() on rank 0 (any side channel), nullptr when nranks == 1
void init(int device_id = 0, int rank = 0, int nranks = 1, const void *rccl_unique_id = nullptr);
void unique_id(void *out128);
void finalize();
// Several ranks on ONE card (validation; include/saena_mpi.hpp uses it under SAENA_MPI_HOST_TRANSPORT=1): the context of rank `rank` of
// `nranks` WITHOUT an RCCL communicator -- RCCL refuses two ranks on one device.  The device path's halo exchanges and scalar
// reductions go through `exchange` / `allreduce_sum` (sgpu_debug_init_host_transport, include/saena_gpu_debug.h), the host setup's
// collectives through the four callbacks of saena_comm_callbacks (include/saena_c.h).  Everything above the transport is the
// multi-rank code.
struct host_transport {
    void *user;
    int (*exchange)(void *user, const void *send, const int *send_rank, const int *send_count, int nsend,
                    void *recv, const int *recv_rank, const int *recv_count, int nrecv, int elem_bytes);
    int (*allreduce_sum)(void *user, double *v, int n);
    int (*allgather)(void *user, const void *send, void *recv, size_t bytes);
    int (*alltoallv)(void *user, const void *send, const size_t *scounts, const size_t *sdispls, void *recv, const size_t *rcounts, const size_t *rdispls);
    int (*allreduce_i64)(void *user, long *v, int n);
    int (*allreduce_f64)(void *user, double *v, int n);
};
void init_host_transport(int device_id, int rank, int nranks, const host_transport &t);

class comm {
public:
    comm();                       // the world communicator of saena::init()
#ifdef SAENA_MPI_HPP
    // include/saena_mpi.hpp (source compatibility with drivers of the reference, which pass MPI_Comm): brings the GPU runtime up over
    // the MPI job the first time it is used -- rank / size from the communicator, device = rank within the node, the RCCL unique id
    // broadcast with MPI_Bcast -- and stands for the world communicator afterwards.  Member FUNCTIONS only: the layout is the library's.
    comm(MPI_Comm c);
    operator MPI_Comm() const;
#define SAENA_HPP_HAS_MPI 1
#endif
    int rank() const;
    int size() const;
    saena_host::Comm *impl() const { return c_; }
private:
    saena_host::Comm *c_;
};

class vector;

class matrix {
public:
    matrix();
    explicit matrix(comm c);
    ~matrix();
    matrix(const matrix &B);              // copy constructor: the host-side matrix is copied, the device operator is created again on first use
    matrix &operator=(const matrix &B);

    int read_file(const char *name);
    int read_file(const char *name, const std::string &input_type);
    void set_comm(comm c);
    int set(index_t i, index_t j, value_t val);                                  // set individual value
    int set(index_t *row, index_t *col, value_t *val, nnz_t nnz_local);          // set multiple values
    int set(index_t i, index_t j, unsigned int size_x, unsigned int size_y, value_t *val);   // set contiguous block
    int set(index_t i, index_t j, unsigned int *di, unsigned int *dj, value_t *val, nnz_t nnz_local);   // set generic block

    void set_eig(const std::string &opts_fname);   // reads the optional eig="..." attribute of the options XML
    void set_eig(double eig);
    // NOT in the reference: the value set_eig(double) takes, estimated on the device (sgpu_op_eig_max: the setup's Lanczos recurrence,
    // `steps` of them, through this matrix's device operator, which is created if it does not exist yet).  One rank.  Nothing is stored:
    // A.set_eig(A.estimate_eig()) before amg::update1(&A) leaves the update without its host Lanczos loop.
    double estimate_eig(int steps = 20);
    void set_remove_boundary(bool remove_bound);
    // NOT in the reference: resolution of assemble()'s nnz-balanced row partition (0 = the reference's nparts^2 buckets)
    void set_partition_buckets(int n_buckets);
    bool add_dup = true;                           // if false replace the duplicate, otherwise add the values together
    int  add_duplicates(bool add);

    int assemble(bool scale = false, bool use_dense = false);
    int assemble_band_matrix(bool use_dense = false);
    int assemble_writeToFile(const char *folder_name = "");      // assemble(), then writeMatrixToFile(folder_name)
    int writeMatrixToFile(const std::string &name = "") const;   // "<name>-r<rank>.mtx", MatrixMarket coordinate real general
    // Knobs of the reference's CPU implementation that have no counterpart on this path; accepted so that drivers
    // written against the reference compile and run unchanged (reference saena.cpp:115-140,205-214):
    void set_p_order(int) {}                        // p-multigrid order of the Nektar++ coupling (out of scope)
    void set_prodim(int) {}
    void set_num_threads(const int &) {}            // OpenMP threads of the CPU kernels
    int  set_shrink(bool) { return 0; }             // coarse levels are placed by amg_hierarchy::shrink_rows here
    int  print(int ran, std::string name = "");     // this rank's entries (ran < 0: every rank), like print_entry

    saena_host::saena_matrix *get_internal_matrix();
    comm    get_comm();
    index_t get_num_rows();
    index_t get_num_local_rows();
    nnz_t   get_nnz();
    nnz_t   get_local_nnz();
    std::vector<index_t> get_orig_split();
    std::vector<index_t> get_split();

    // w = A v on this rank's slices (GPU)
    void matvec(std::vector<value_t> &v, std::vector<value_t> &w);
    void matvec(saena::vector &v, saena::vector &w);

    int  erase();
    int  erase_lazy_update() { return erase(); }        // (reference saena.hpp:67-68: erase variants of its lazy-update path; one erase here)
    int  erase_no_shrink_to_fit() { return erase(); }
    void destroy();

    sgpu_op *device_op();          // created on first use (sgpu_op_create)
private:
    comm c_;
    saena_host::saena_matrix *m_pImpl;
    sgpu_op *dev_ = nullptr;
    bool use_dense_ = false;       // assemble(scale, use_dense = true): the device operator as dense rows
};

class vector {
public:
    vector();
    explicit vector(comm c);
    void set_comm(comm c);
    int set_idx_offset(index_t offset);
    int set(index_t i, value_t val);                                   // set individual value
    int set(const index_t *idx, const value_t *val, index_t size);     // set multiple values
    int set(const value_t *val, index_t size, index_t offset);         // contiguous values starting at global index offset
    int set(const value_t *val, index_t size);                         // contiguous values starting at idx_offset
    int set_dup_flag(bool add);
    int assemble();
    void get_vec(value_t *&vec);        // this rank's values in ascending index order (owned by the vector)
    index_t get_size() const { return (index_t)val_.size(); }
    index_t first_index() const { return idx_.empty() ? 0 : idx_.front(); }
    const std::vector<index_t> &indices() const { return idx_; }
    comm get_comm() { return c_; }
    // return_vec (saena.cpp:357: the solution back in the order the entries were set): the entries are kept in ascending index order here
    // and solve* returns u in the matrix's row order, so this is a copy (u2 allocated when null)
    int return_vec(value_t *&u1, value_t *&u2) {
        if (!u2) u2 = static_cast<value_t *>(std::malloc(std::max<size_t>(1, val_.size()) * sizeof(value_t)));
        if (u1 != u2) for (size_t i = 0; i < val_.size(); ++i) u2[i] = u1[i];
        return 0;
    }
    int print_entry(int ran);           // (index, value) of this rank's entries when ran < 0 or ran == rank (saena_vector.cpp:504)
private:
    comm c_;
    index_t ofst_ = 0;
    bool add_dup_ = false;
    std::vector<index_t> idx_;
    std::vector<value_t> val_;
    bool assembled_ = false;
};

class options {
private:
    int    solver_max_iter;
    double relative_tol;
    std::string smoother;
    int    preSmooth;
    int    postSmooth;
    std::string PSmoother;
    float  connStrength;
    bool   dynamic_levels;
    int    max_level;
    int    float_level;
    double filter_thre;
    double filter_max;
    int    filter_start;
    int    filter_rate;
    bool   switch_to_dense;
    float  dense_thre;
    int    dense_sz_thre;
    std::string petsc_solver;
public:
    explicit options(int max_iter = 100, double relative_tol = 1e-8, std::string smoother = "chebyshev",
                     int preSmooth = 3, int postSmooth = 3, std::string PSmoother = "jacobi", float connStrength = 0.3,
                     bool dynamic_lev = true, int max_lev = 10, int float_lev = 3,
                     double fil_thr = 1e-14, double fil_max = 1e-8, int fil_st = 1, int fil_rate = 2,
                     bool switch_to_den = false, float dense_thr = 0.1, int dense_sz_thr = 5000);
    explicit options(const std::string &name);       // parameters from an xml file
    void set(int max_iter = 100, double relative_tol = 1e-8, std::string smoother = "chebyshev",
             int preSmooth = 3, int postSmooth = 3, std::string PSmoother = "jacobi", float connStrength = 0.3,
             bool dynamic_lev = true, int max_lev = 10, int float_lev = 3,
             double fil_thr = 1e-14, double fil_max = 1e-8, int fil_st = 1, int fil_rate = 2,
             bool switch_to_den = false, float dense_thr = 0.1, int dense_sz_thr = 5000);
    void set_from_file(const std::string &name);
    void set_solve_params(int max_iter = 100, double relative_tolerance = 1e-8, std::string smoother = "chebyshev",
                          int preSmooth = 3, int postSmooth = 3);
    void set_max_iter(int v) { solver_max_iter = v; }
    void set_relative_tolerance(double v) { relative_tol = v; }
    void set_smoother(std::string v) { smoother = std::move(v); }
    void set_preSmooth(int v) { preSmooth = v; }
    void set_postSmooth(int v) { postSmooth = v; }
    int         get_max_iter() const { return solver_max_iter; }
    double      get_tol() const { return relative_tol; }
    std::string get_smoother() const { return smoother; }
    int         get_preSmooth() const { return preSmooth; }
    int         get_postSmooth() const { return postSmooth; }
    std::string get_PSmoother() const { return PSmoother; }
    float       get_connStr() const { return connStrength; }
    bool        get_dynamic_levels() const { return dynamic_levels; }
    int         get_max_lev() const { return max_level; }
    int         get_float_lev() const { return float_level; }
    double      get_filter_thre() const { return filter_thre; }
    double      get_filter_max() const { return filter_max; }
    int         get_filter_start() const { return filter_start; }
    int         get_filter_rate() const { return filter_rate; }
    bool        get_switch_dense() const { return switch_to_dense; }
    float       get_dense_thre() const { return dense_thre; }
    int         get_dense_sz_thre() const { return dense_sz_thre; }
    std::string get_petsc_solver() const { return petsc_solver; }
};

class amg {
public:
    amg();
    ~amg();
    amg(const amg &) = delete;
    amg &operator=(const amg &) = delete;

    void set_dynamic_levels(const bool &dl = true);
    int set_matrix(saena::matrix *A, saena::options *opts);   // smoothed-aggregation setup (host) + upload
    // A matrix of the same size with other values (its pattern may differ too) through the hierarchy set_matrix built (reference
    // saena.hpp:236-237; one rank, more throw "one rank").  update1: A_new replaces the finest operator, nothing else changes.
    // update2: every coarse operator is rebuilt as R A P over the kept aggregates, P and R -- the setup without its strength graph,
    // aggregation, smoothed P and transpose; the number of levels stays.  The caller keeps A_new alive and may destroy the old
    // matrix; the right-hand side stays set.  After a throw the hierarchy is as it was.
    // update3, the reference's local-difference approximation of update2, is not provided.
    // NOT in the reference, opt-in, before set_matrix / update1 / update2: eig_max of every level (Chebyshev smoother) from the device
    // estimate instead of the host Lanczos loop, on one rank -- the same recurrence, equal within 1e-12 relative, not bit for bit.
    // Also on with SAENA_DEVICE_EIG=1.  Where the device declines, the host loop runs; a value set with matrix::set_eig is kept.
    void set_device_eig(bool on);
    // NOT in the reference, before set_matrix: how the coarsest level is solved (sgpu_amg_params.coarse_solver).  "direct" (the
    // default): the dense inverse; "cg": solve_coarsest_CG; "device_cg": the same CG, and where the coarsest level has more than
    // 1 024 rows (set_multigrid_max_level cut the hierarchy off, coarsening stalled) the device-resident CG instead of the host-driven
    // loop the other two fall back to there: the V-cycle stays one captured graph and solve_pCG_block, solve_pFGMRES and eigs take
    // the hierarchy.  Any other name throws.  SAENA_COARSE_SOLVER=direct|cg|device_cg in the environment, read by set_matrix,
    // overrides it for drivers compiled unchanged.
    void set_coarse_solver(const std::string &name);
    // NOT in the reference, before set_matrix, one rank: "constant" tells the solver that the matrix annihilates constants (pure Neumann
    // or periodic Poisson, a graph Laplacian; assemble it after matrix::set_remove_boundary(false)).  The solves then solve
    // A u = rhs - mean(rhs) and return the solution of zero mean, whatever the mean of the right-hand side; eigs returns the nev
    // smallest NONZERO eigenpairs (the constant vector is locked: the first is the Fiedler vector).  set_matrix throws when the matrix
    // or the coarsest operator has max|A 1| / max|a_ii| > 1e-10 (a pinned row, a reaction term) or with more than one rank;
    // solve_pFGMRES, eigs_gen and eigs_many throw on such a solver.  "none" (the default) is the solver as it always was; any other
    // name throws.  Null spaces other than constants and nonsymmetric singular matrices are not covered.
    void set_null_space(const std::string &name);
    int update1(saena::matrix *A_new);
    int update2(saena::matrix *A_new);
    int set_rhs(saena::vector &rhs);                          // note: this function copies the rhs
    int set_rhs(const value_t *rhs_local, index_t size);      // already partitioned like A (interior numbering)

    // before calling solve, u may be nullptr; after, it holds this rank's slice of the solution
    // (allocated here when null; free it with saena::free_vector)
    int solve(value_t *&u, saena::options *opts);
    int solve_pCG(value_t *&u, saena::options *opts, bool print_info = true);
    int solve_CG(value_t *&u, saena::options *opts);          // CG without the multigrid preconditioner
    // nrhs = 2, 4 or 8 right-hand sides through one pass over every operator (any number of ranks: the K columns of a
    // halo cross in one exchange): rhs_local and u are column-major,
    // size x nrhs (column j at [j * size]), partitioned like A; u is allocated (size * nrhs) when null.  Every column is solved
    // as solve_pCG solves it alone, with its own iteration count and history; returns 1 if any column did not converge
    int set_rhs_block(const value_t *rhs_local, index_t size, int nrhs);
    int solve_pCG_block(value_t *&u, saena::options *opts);
    const std::vector<value_t> &residual_history_block(int j) const { return hist_blk_.at((size_t)j); }
    int solve_smoother(value_t *&u, saena::options *opts);    // the smoother alone (preSmooth sweeps per iteration)
    // C = A B (host SpGEMM, one rank in this round); C is erased first and assembled unless assemble == false
    void matmat(saena::matrix *A, saena::matrix *B, saena::matrix *C, bool assemble = true, bool print_timing = false);
    void profile_matvecs();                                   // average matvec time of every level's A
    void profile_matvecs_breakdown() { profile_matvecs(); }   // (saena.hpp:261: the same loop with the reference's CPU phases split out; one kernel per matvec here)
    int solve_pCG_profile(value_t *&u, saena::options *opts);  // solve_pCG with its timing printed (the reference prints a per-phase profile)
    int solve_petsc(value_t *&u, saena::options *opts);        // PETSc bridge: out of scope -- prints why and returns 1 (kept so that drivers compile)
    // The reference declares both (saena.hpp:230-231) and compiles their bodies OUT (`#if 0`, saena_object_solve.cpp:3808 / 4077: GMRES and
    // pGMRES return 0 without touching u).  Mirrored as that: the solve parameters are re-read like every solve* does, u is left as it
    // was (allocated and zeroed when null), a line says so, 0 is returned.
    // The live method for operators that are not symmetric positive definite is solve_pFGMRES below.
    int solve_GMRES(value_t *&u, saena::options *opts);
    int solve_pGMRES(value_t *&u, saena::options *opts);
    // Restarted flexible GMRES, right-preconditioned by one V-cycle per inner iteration (precondition = false: plain restarted GMRES),
    // for operators solve_pCG is not defined for (sgpu_solve_FGMRES; one rank).  restart: 1..64 inner iterations per cycle;
    // opts->get_max_iter() caps the inner iterations.  residual_history() holds ||r_0|| and the residual estimate after every inner
    // iteration, last_iterations() their number; returns 1 if the recomputed residual did not reach the tolerance
    int solve_pFGMRES(value_t *&u, saena::options *opts, int restart = 30, bool precondition = true);
    // The nev smallest eigenpairs of the matrix (symmetric positive definite) by LOBPCG on a block of K = 2, 4 or 8 vectors, one
    // block V-cycle per iteration as preconditioner (precondition = false: none); sgpu_eigs_LOBPCG, one rank.  x0: column-major
    // size x K start vectors partitioned like A, or nullptr for the default start; opts->get_max_iter() caps the iterations,
    // opts->get_tol() is the tolerance of ||A x - lambda x|| relative to lambda.  lambda receives K values, ascending; x (allocated
    // size * K when null) the eigenvectors, column-major; columns nev .. K-1 are guard vectors that need not have converged.
    // eig_residuals() holds ||A x_j - lambda_j x_j||, last_iterations() the iterations; returns 1 if a wanted pair did not converge.
    // Expect slow convergence when nev cuts a cluster of equal eigenvalues in two: let nev end at a gap of the spectrum.
    int eigs(value_t *&x, std::vector<value_t> &lambda, saena::options *opts, int K, int nev, const value_t *x0 = nullptr, bool precondition = true);
    // The same for the generalised problem A x = lambda B x (sgpu_eigs_LOBPCG_gen, one rank): B is an assembled symmetric positive
    // definite matrix of the same size and partition (a mass matrix, consistent or lumped).  The eigenvectors are B-orthonormal on
    // return; a column is converged when ||A x - lambda B x|| < tol lambda ||B x||; eig_residuals() holds ||A x_j - lambda_j B x_j||.
    // The preconditioner is the V-cycle of A.  A distinct name: no call of eigs becomes ambiguous.  A LUMPED (diagonal) B must be
    // assembled after B.set_remove_boundary(false): assemble() otherwise takes every single-entry row for a boundary node and removes
    // it, and eigs_gen refuses the B that is left for its size, with a message that says so.
    int eigs_gen(value_t *&x, std::vector<value_t> &lambda, saena::matrix *B, saena::options *opts, int K, int nev, const value_t *x0 = nullptr, bool precondition = true);
    // More than K eigenpairs (sgpu_eigs_LOBPCG_many, one rank): the nev <= 64 smallest pairs of A x = lambda x, or of A x = lambda B x
    // with B given, by sweeps of the block solve on K = 2, 4 or 8 vectors; converged vectors are locked and the block iterates in
    // the B-orthogonal complement of what is locked.  A sweep asks for sweep_nev pairs (0: K / 2, half the block as guard vectors).
    // opts->get_max_iter() caps the TOTAL iterations over all sweeps (the default of 100 is small for this: 20 pairs take about 70),
    // opts->get_tol() is the tolerance as in eigs / eigs_gen.  x0: column-major size x K start vectors, or nullptr for generated ones.
    // q (allocated size * nev when null) receives the eigenvectors, column-major, B-orthonormal, in ascending order of lambda;
    // lambda and eig_residuals() are resized to the pairs found: nev, or fewer when the call returns 1 (the iterations ran out; the
    // pairs found so far are valid).  last_iterations() is the total, eig_sweeps() the number of sweeps.
    int eigs_many(value_t *&q, std::vector<value_t> &lambda, saena::options *opts, int nev, int K = 8, int sweep_nev = 0, saena::matrix *B = nullptr,
                  const value_t *x0 = nullptr, bool precondition = true);
    int eig_sweeps() const { return eig_sweeps_; }
    const std::vector<value_t> &eig_residuals() const { return eig_res_; }
    comm get_orig_comm();

    int  switch_to_dense(bool val);                 // dense row-major storage for the coarse levels past the density threshold
    int  set_dense_threshold(float thre);
    double get_dense_threshold();
    // accepted for source compatibility, no effect on this path (reference saena.cpp:696-727,901-911)
    void set_num_threads(const int &) {}
    int  set_shrink_levels(std::vector<bool>) { return 0; }
    int  set_shrink_values(std::vector<int>) { return 0; }
    int  switch_repart(bool) { return 0; }
    int  set_repart_thre(float) { return 0; }
    int  set_scale(bool sc);                        // symmetric diagonal scaling is not implemented: true is refused
    int  set_sample_sz_percent(double) { return 0; }
    int  matrix_diff(saena::matrix &A, saena::matrix &B);   // prints entry-wise differences of two assembled matrices
    int  set_verbose(bool verb);
    bool verbose = false;
    int  set_multigrid_max_level(int max);
    int  get_num_levels() const;
    // residual norms of the last solve: hist[0] = initial, hist[k] after iteration k
    const std::vector<value_t> &residual_history() const { return hist_; }
    int  last_iterations() const { return iters_; }
    void destroy();
    sgpu_amg *device_handle() { return damg_; }
private:
    saena::matrix *A_ = nullptr;
    saena_host::amg_hierarchy *H_ = nullptr;
    std::vector<sgpu_op *> dA_, dP_, dR_;
    sgpu_amg *damg_ = nullptr;
    std::vector<value_t> rhs_;
    std::vector<value_t> hist_;
    int iters_ = 0;
    std::vector<value_t> rhs_blk_;                 // set_rhs_block: column-major size x nrhs_
    int nrhs_ = 0;
    std::vector<std::vector<value_t>> hist_blk_;   // per column of the last solve_pCG_block
    std::vector<value_t> eig_res_;                 // of the last eigs / eigs_gen / eigs_many
    int eig_sweeps_ = 0;                           // of the last eigs_many
    int eigs_common(value_t *&x, std::vector<value_t> &lambda, saena::matrix *B, saena::options *opts, int K, int nev, const value_t *x0,
                    bool precondition, const char *what);
    bool dynamic_levels_ = true;
    bool switch_to_dense_ = false;
    float dense_thre_override_ = 0;
    int max_level_override_ = -1;
    bool device_eig_ = false;
    int coarse_solver_ = 1;
    int null_space_ = 0;
    void drop_device();
    int update(saena::matrix *A_new, int mode);
    // which: 0 solve, 1 solve_pCG, 2 solve_CG, 3 solve_smoother, 4 solve_pFGMRES (the only one that reads restart / precondition)
    int run(value_t *&u, saena::options *opts, int which, bool print_info, int restart = 0, bool precondition = true);
    int gmres_compiled_out(const char *name, value_t *&u, saena::options *opts);
};

void free_vector(value_t *u);

// Matrix generator functions (reference include/aux_functions2.h:12-43)
int laplacian3D(saena::matrix *A, index_t mx, index_t my, index_t mz);
// this rank's z-slabs of the full mx*my*mz grid (boundary included), as the reference returns them;
// pair with saena::vector::set(val, size, offset) using the returned first global index
index_t laplacian3D_set_rhs(value_t *&rhs, index_t mx, index_t my, index_t mz, comm c, index_t *first_index = nullptr);
int band_matrix(saena::matrix &A, index_t M, unsigned int bandwidth);

} // namespace saena
