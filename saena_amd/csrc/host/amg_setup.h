// amg_setup.h -- host-side smoothed-aggregation setup.
//
// Restates saena_object::setup / coarsen / SA / compute_coarsen of the reference
// so that a hierarchy exists on the GPU box (where the reference does not): the
// V-cycle kernels consume its output (A_l, P_l, R_l per level).  Like the
// reference, setup is host code that runs once; it is not on the timed path.
#pragma once
#include "saena_matrix.h"

#include <memory>
#include <string>
#include <vector>

namespace saena_host {

// Optional accelerator for the setup's sparse products C = A B (CSR in, CSR out, rows sorted by column, the drop rule of
// the host kernel).  libsaena_amd.so installs its GPU kernel here when a device context exists; returns 0 on success,
// non-zero to decline (the host kernel then runs).  nullptr in libsaena_host.so.
// B's entries may come in TWO pieces (the rank's own rows, then the halo rows fetched for this product): entries [0, b_split) sit
// at b_col / b_val, entries [b_split, b_ptr[b_rows]) at b_col1 / b_val1 (b_col1 == nullptr: one piece) -- the caller then stacks
// the row pointers only, not the gigabytes of columns and values.
typedef int (*spgemm_hook_fn)(int a_rows, int b_rows, int b_cols, const long *a_ptr, const int *a_col, const double *a_val,
                              const long *b_ptr, const int *b_col, const double *b_val, long b_split, const int *b_col1, const double *b_val1,
                              int row_offset, std::vector<long> &c_ptr, std::vector<int> &c_col, std::vector<double> &c_val);
extern spgemm_hook_fn g_spgemm_hook;
// PRECONDITION of the hook, of the host kernel's "bit for bit" partner: the columns of every row of B are DISTINCT and
// ASCENDING (the device kernels spread a row of B over their lanes without atomics on the sums, and bisect it by column).
// Every right operand of the setup is an assembled operator, a smoothed prolongator whose rows were sorted and merged, or
// rows fetched from one of those; see gpu_spgemm in sgpu_spgemm.hip.  A's rows may come in any order, duplicates included.

// Optional device estimate of eig_max (find_eig below) for a one-rank operator: CSR in (64-bit row pointers, columns ascending in
// every row), inv_diag[n], the number of Lanczos steps; *eig_max out.  libsaena_amd.so installs it at sgpu_init next to the product
// hook (sgpu_lanczos.hip.inc: a temporary operator from sgpu_op_create, sgpu_op_eig_max, destroy); 0 on success, non-zero to decline
// (no memory, a context of several ranks): the host find_eig then runs.  It is asked only where amg_hierarchy::device_eig or
// SAENA_DEVICE_EIG=1 says so: with the switch off nothing changes by a bit whether or not it is installed.  nullptr in libsaena_host.so.
typedef int (*eig_hook_fn)(int n, const long *ptr, const int *col, const double *val, const double *inv_diag, int steps, double *eig_max);
extern eig_hook_fn g_eig_hook;
// The two ends of find_eig that do not depend on who runs the recurrence (the host loops, or the device through the hook): the LCG
// start vector over the row index, normalised, and 1.0001 x the largest eigenvalue of the tridiagonal matrix (Sturm bisection).
void lanczos_start_vector(index_t n, double *v);
double lanczos_ritz_max(const std::vector<double> &alpha, const std::vector<double> &beta);

// sgpu_amg_params.coarse_solver by name: "direct" 1, "cg" 0, "device_cg" 2; -1 for anything else (a null pointer included).
// coarse_solver_choice: what a to_device passes to sgpu_amg_create -- SAENA_COARSE_SOLVER where the environment names a solver (a
// driver compiled unchanged), else the value its setter left.
int coarse_solver_code(const char *name);
int coarse_solver_choice(int set_value);

// Which path served the rows of a product: counted by the host kernel and by the host side of the device driver (no
// kernel takes part), for the tests that must know which accumulator they exercised.  g_spgemm_last is the last product,
// g_spgemm_total the sum over the products since spgemm_stats_reset().  The setup multiplies from one thread at a time.
enum {
    SPGEMM_HOST_DENSE = 0,    // host kernel: rows on the dense accumulator (products > columns / 8)
    SPGEMM_HOST_HASH,         //              rows on the hash accumulator
    SPGEMM_HOST_REHASH,       //              grow-and-rehash steps of the hash accumulator
    SPGEMM_LIGHT,             // device: rows on k_spgemm_light
    SPGEMM_MEDIUM,            //         rows on k_spgemm_medium<false>
    SPGEMM_TRY_KEPT,          //         rows k_spgemm_medium<true> finished in its table
    SPGEMM_TRY_ABANDONED,     //         rows it gave up (more than 3072 distinct columns, or the table full inside a step)
    SPGEMM_LDS,               //         abandoned rows served by k_spgemm_lds (dense accumulator in LDS windows)
    SPGEMM_HBM,               //         abandoned rows served by k_spgemm_heavy (dense accumulator in HBM)
    SPGEMM_CHUNKS,            //         chunks of rows the driver ran
    SPGEMM_WINDOWS,           //         column windows of k_spgemm_lds (0: that kernel did not run)
    SPGEMM_DECLINED,          // the hook was asked and declined
    SPGEMM_ON_DEVICE,         // the result is the hook's
    SPGEMM_NSTATS
};
struct spgemm_stats { long v[SPGEMM_NSTATS] = {}; };
extern spgemm_stats g_spgemm_last, g_spgemm_total;
void spgemm_stats_reset();
// saena_debug_spgemm (include/saena_c.h): C = A B from plain arrays through the setup's own product code.
// mode: 0 what the setup does, 1 the host kernel, 2 the hook (throws when there is none or when it declines)
void debug_spgemm(int mode, index_t a_rows, index_t b_rows, index_t b_cols, const nnz_t *a_ptr, const index_t *a_col, const value_t *a_val,
                  const nnz_t *b_ptr, const index_t *b_col, const value_t *b_val, nnz_t b_split, const index_t *b_col1, const value_t *b_val1,
                  index_t row_offset, std::vector<nnz_t> &c_ptr, std::vector<index_t> &c_col, std::vector<value_t> &c_val);
// saena_debug_filter (include/saena_c.h): the setup's filter on rows [row_offset, row_offset + n) of a level, from plain arrays
void debug_filter(index_t n, const nnz_t *ptr, const index_t *col, const value_t *val, double thre, index_t row_offset,
                  std::vector<nnz_t> &c_ptr, std::vector<index_t> &c_col, std::vector<value_t> &c_val);
// The exchange chain of one multi-rank apply in microseconds (pack -> RCCL send/recv -> boundary rows), as the GPU runtime
// MEASURED it on this job's communicator at sgpu_init (a ping-pong with the neighbouring rank; the maximum over the
// ranks, so every rank holds the same number); 0: not measured (host-only library, one rank).  The agglomeration model
// below starts from it instead of the constant; SAENA_SHRINK_CHAIN_US still overrides.
extern double g_measured_chain_us;

// saena::options (reference include/saena.hpp:127-193; defaults :151-155)
struct amg_options {
    int         solver_max_iter = 100;
    double      relative_tol    = 1e-8;
    std::string smoother        = "chebyshev";
    int         preSmooth       = 3;
    int         postSmooth      = 3;
    std::string PSmoother       = "jacobi";
    float       connStrength    = 0.3f;
    bool        dynamic_levels  = true;
    int         max_level       = 10;
    int         float_level     = 3;
    double      filter_thre     = 1e-14;
    double      filter_max      = 1e-8;
    int         filter_start    = 1;
    int         filter_rate     = 2;
    bool        switch_to_dense = false;
    float       dense_thre      = 0.1f;
    int         dense_sz_thre   = 5000;
    // parse the positional attributes of <SAENA><OPTIONS .../> (saena.cpp:444-546)
    void set_from_file(const std::string &name);
};

struct amg_level {
    saena_matrix *A = nullptr;                   // level 0: the caller's matrix; l > 0: owned by `Ac_store` of level l-1
    transfer_matrix P, R;                        // empty on the coarsest level
    std::unique_ptr<saena_matrix> Ac_store;      // A of level l+1
    std::vector<index_t> roots;                  // fine index of the root of every aggregate, ascending (= coarse numbering)
    std::vector<index_t> agg;                    // coarse id of every fine row (one-rank setup; the reference's `aggregate` after
                                                 // aggregate_index_update, setup1:2103-2260): kept for the setup's pins
};

// One rank's share of a hierarchy that was built at one rank and then row-partitioned.
struct dist_level {
    std::vector<index_t> split;                  // row partition of this level over the ranks
    DistLayout A, P, R;                          // P/R empty on the coarsest level
    std::vector<value_t> inv_diag;
    double eig_max = 0;
    index_t Mbig = 0;
    nnz_t nnzA = 0, nnzP = 0;
};

class amg_hierarchy {
public:
    amg_options opts;
    std::vector<amg_level> levels;               // levels.size() == max_level + 1 after setup
    int max_level = 0;
    // thresholds of saena_object.h:43-46
    unsigned int least_row_threshold = 100;
    double row_reduction_up_thrshld = 0.90;

    // saena_object::setup (saena_object.cpp:175-406)
    int setup(saena_matrix *A, const amg_options &o);
    // saena::amg::update1 / update2 (src/saena_object_lazy.cpp:7-77): a matrix of the same size with other values (its
    // pattern may differ too) through the hierarchy setup() built.  One rank.  A_new becomes level 0 and must outlive the
    // hierarchy; the matrix it replaces is no longer referenced.
    //   mode 1: nothing else changes -- every coarser A, every P, R, roots and agg stays bit for bit.
    //   mode 2: every coarse A is rebuilt over the KEPT P, R and aggregates by the tail of coarsen: (R A) P through the same
    //           spgemm (and hook), the filter on the threshold schedule replayed from opts, setup_from_csr; then find_eig where
    //           setup calls it.  The result is what setup(A_new) would build if its aggregation and transfer operators were
    //           the old hierarchy's.  The pattern of a coarse level follows the values (the products drop |v| <= 1e-14, the
    //           filter lumps by threshold), so nothing of the old coarse operators is reused.  eig_max is recomputed, where the
    //           reference carries the old value over.  The number of levels never changes.
    // Throws -- and leaves the hierarchy exactly as it was -- when there is no hierarchy yet, when it was built over more than
    // one rank, when A_new is not assembled or has another Mbig, and for any other mode.  SAENA_SETUP_TIMING=1 prints the
    // phases as "[update L<l>] ...".
    // `undo` (optional) receives what the update replaced; undo_update() puts it back -- for a caller whose own follow-up (the
    // device side of saena_amg_update) can still fail after the host side has committed.
    struct update_undo { saena_matrix *A0 = nullptr; int mode = 0; std::vector<std::unique_ptr<saena_matrix>> Ac; };
    int update(saena_matrix *A_new, int mode, update_undo *undo = nullptr);
    void undo_update(update_undo &u);

    // Multi-rank use: setup_distributed -> setup_rows_distributed, every rank builds its rows of every level (`dist`).
    // Partition per level: the fine split is A's; a coarse level inherits it through the aggregates (splitNew[r] =
    // number of roots below split[r], aggregate_index_update setup1:2115-2122); levels with <= shrink_rows rows live
    // entirely on rank 0 (the reference shrinks coarse levels onto fewer ranks, saena_matrix_shrink.cpp:167-265).
    // SAENA_SETUP=gathered selects the older form: gather the fine operator, build the whole hierarchy on every
    // rank (`levels`, `A_global`), keep the own rows (`distribute`).
    std::vector<dist_level> dist;
    std::unique_ptr<saena_matrix> A_global;      // the gathered fine operator (one-rank replica)
    std::unique_ptr<Comm> self_comm;
    // Agglomeration of coarse levels onto fewer ranks -- the reference's shrinking (saena_matrix::decide_shrinking /
    // decide_shrinking_c / shrink_set_params / shrink_cpu, src/saena_matrix_shrink.cpp:3-265, called from
    // compute_coarsen, src/saena_object_setup2.cpp:249-318) restated for one GPU per rank.  The reference times a dummy
    // matvec per level and shrinks by a factor 2..4 when communication exceeds twice the computation, and puts the
    // coarsest level on one rank.  Here the two times are a model with measured constants: one GPU applies the level in
    // T1 = 12 B x nnz / shrink_bw + shrink_launch_us, a multi-rank apply costs at least the exchange chain
    // shrink_chain_us (pack -> RCCL send/recv -> boundary rows: measured at sgpu_init on the job's communicator,
    // g_measured_chain_us; 23 us on one GPU with RCCL self send/recv, profiles/r01_halo_loopback.md and
    // profiles/r02_halo_loopback_modes.log, is the fall-back when nothing was measured).  Rules, evaluated after the coarse operator exists (its nnz is known):
    //   T1 <= chain                      -> the whole level lives on rank 0 (no exchange at all below this level);
    //   chain > 2 x T1 / active ranks    -> merge groups of f = clamp(floor(chain / compute / 5), 2, 4) consecutive active
    //                                       ranks onto the first of each group (shrink_set_params' rule: ranks k f own rows);
    //   rows <= shrink_rows              -> rank 0 (a row-count override, off by default).
    // SAENA_SHRINK_CHAIN_US / SAENA_SHRINK_ROWS override; chain 0 disables agglomeration.  The vectors need no
    // repartition step (Grid::repart_u / repart_back_u, src/grid.cpp:99-163): R's rows and P's columns are laid out on
    // the agglomerated partition, so R r lands where the coarse level lives and P e leaves from there -- the move rides
    // the transfer operators' own halo exchange.
    double  shrink_chain_us = 23.0, shrink_bw = 5e12, shrink_launch_us = 3.0;
    index_t shrink_rows = 0;
    std::vector<int> level_stride;               // per level: rank r owns rows iff r % stride == 0 (1 = all ranks, >= nranks = rank 0 only)
    int  next_stride(long nnzC, index_t rowsC, int np, int stride_prev) const;
    static std::vector<index_t> merge_split(const std::vector<index_t> &splitNew, int stride);
    int setup_distributed(saena_matrix *A_dist, const amg_options &o);
    // the distributed setup proper: every rank builds its rows of every level (fills `dist` only)
    int setup_rows_distributed(saena_matrix *A_dist, const amg_options &o);
    void distribute(Comm &c, const std::vector<index_t> &split0);

    // per-level facts, whichever way the hierarchy was built
    index_t level_rows(int l) const { return dist.empty() ? levels[(size_t)l].A->Mbig : dist[(size_t)l].Mbig; }
    nnz_t   level_nnzA(int l) const { return dist.empty() ? levels[(size_t)l].A->nnz_g : dist[(size_t)l].nnzA; }
    nnz_t   level_nnzP(int l) const { return l >= max_level ? 0 : dist.empty() ? levels[(size_t)l].P.nnz_g : dist[(size_t)l].nnzP; }
    double  level_eig(int l) const {
        const bool have = (size_t)l < levels.size() && levels[(size_t)l].A != nullptr;
        return (dist.empty() || have) ? levels[(size_t)l].A->eig_max_of_invdiagXA : dist[(size_t)l].eig_max;
    }

    // pieces, public for tests ------------------------------------------------
    // create_strength_matrix + strength_matrix::setup_matrix (setup1:520-719, strength_matrix.cpp:233-453):
    // CSR of the strong connections (local rows, global columns), diagonal included
    static void strength_graph(const saena_matrix &A, float connStrength, std::vector<nnz_t> &ptr, std::vector<index_t> &col);
    // aggregation_1_dist + aggregate_index_update (setup1:724-995, :2103-2260); returns the number of aggregates
    static index_t aggregate(const saena_matrix &A, const std::vector<nnz_t> &ptr, const std::vector<index_t> &col,
                             std::vector<index_t> &agg, std::vector<index_t> *roots = nullptr);
    // saena_object::matmat (saena_object_setup_matmat.cpp:1164-1487): C = A B for two assembled one-rank matrices;
    // products with |v| <= 1e-14 are dropped unless on the diagonal, the rule of the reference's SpGEMM output.
    // Returns the entries of C (row, col, val), row-major.
    static std::vector<cooEntry> matmat(const saena_matrix &A, const saena_matrix &B);
    // find_eig (saena_object.cpp:572-592, lamlan_saena.h): largest eigenvalue of D^-1 A by 20 Lanczos steps, x 1.0001
    static double find_eig(const saena_matrix &A);
    // Opt-in: setup() and update() take eig_max of their one-rank levels from g_eig_hook (the same recurrence on the device; equal to
    // find_eig's value within 1e-12 relative, not bit for bit: the dots are summed in another order).  Also on with SAENA_DEVICE_EIG=1,
    // read at every call.  Without a hook, or when it declines, find_eig runs.  A value the caller set on a matrix is kept either way.
    bool device_eig = false;

private:
    double filter_thre_cur = 0;
    int    filter_it = 0;
    int  coarsen(int l);                          // saena_object::coarsen (saena_object.cpp:409-452)
    void filter(std::vector<cooEntry> &v, index_t sz, index_t ofst);   // setup2:852-916
    double level_eig(const saena_matrix &A, bool *on_device) const;   // the hook where the switch is on and it accepts, else find_eig
};

} // namespace saena_host
