// sgpu_runtime.hip -- C ABI (include/saena_gpu.h) over the gfx950 kernels.
//
// One process = one rank = one MI355X.  Two HIP streams per rank: `cs` runs the
// interior rows of every operator, `hs` carries the x-vector halo (pack, RCCL
// send/recv over xGMI) and then computes the boundary rows, so the exchange
// overlaps the local SpMV exactly where the reference overlaps MPI_Isend/Irecv
// with its local loop (src/saena_matrix_matvec.cpp:32-80).  See apply().
#include "../../include/saena_gpu.h"
#include "../../include/saena_gpu_debug.h"
#include "kernels.hip.h"
#include "kernels_block.hip.h"
#include "kernels_gmres.hip.h"
#include "kernels_eig.hip.h"
#include "kernels_eig_lock.hip.h"
#include "eig_lock_plan.h"
#include "kernels_lanczos.hip.h"
#include "kernels_coarse_cg.hip.h"
#include "dispatch.h"
#include "devmem.h"
#include "forms.h"
#include "xwin_plan.h"
#include "coarse_pinv.h"
#include "host/dense_eig.h"
#include "host/comm.h"
#include "host/par.h"
#include "host/amg_setup.h"

#include <hip/hip_runtime.h>
#include <climits>
#include <rccl/rccl.h>

#include <algorithm>
#include <map>
#include <atomic>
#include <csignal>
#include <unistd.h>
#include <cmath>
#include <chrono>
#include <fcntl.h>
#include <sys/stat.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

extern "C" void sgpu_install_spgemm_hook(int on);
extern "C" void sgpu_install_eig_hook(int on);

using devmem::DevArr;
using devmem::PinArr;
using namespace forms;

namespace {

thread_local std::string g_err;
long g_launches = 0;          // host-side enqueues (kernels, graph launches, RCCL groups): sgpu_debug_launch_count
uint64_t g_plan_generation = 0;   // bumped whenever an operator's kernel plan changes: captured graphs made before are stale
#define SGPU_LAUNCH(...) do { ++g_launches; hipLaunchKernelGGL(__VA_ARGS__); } while (0)

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(SGPU_ERR_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
    } while (0)
#define NCCLCHK(expr)                                                                                  \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess) return fail(SGPU_ERR_RCCL, "%s:%d %s: %s", __FILE__, __LINE__, #expr, ncclGetErrorString(r_)); \
    } while (0)
#define CHK(expr)                                                                                      \
    do {                                                                                               \
        int s_ = (expr);                                                                               \
        if (s_ != SGPU_OK) return s_;                                                                  \
    } while (0)

struct Ctx {
    bool        live = false;
    int         device = 0, rank = 0, nranks = 1;
    int         ncu = 256;            // compute units of the device (k_csr_xlds launches one workgroup per CU)
    hipEvent_t  tk0 = nullptr, tk1 = nullptr;   // time_reps' events: every timing entry point's
    hipStream_t cs = nullptr, hs = nullptr;
    ncclComm_t  comm = nullptr;
    double     *partials = nullptr;   // dot partial sums
    double     *cblk = nullptr;       // sgpu_block_center / the block solves of a null-space hierarchy: [n_partials][8] partial sums, then 8 sums
    double     *dscalar = nullptr;    // device scalars (dot result)
    double     *hscalar = nullptr;    // pinned host mirror
    int        *dint = nullptr;       // device int scratch (coarse CG iterations, barrier)
    int        *hint = nullptr;       // pinned
    int         n_partials = 1024;
    // cross-stream dependencies cs <-> hs of the halo exchange.  hipStreamWriteValue64 / hipStreamWaitValue64 on
    // signal memory cost ~5 us per hop on the GPU, an event record + wait ~11 us (tools/hop_bench.hip,
    // profiles/r01_hop_bench.log); events remain the fallback where the stream memory operations are unavailable.
    uint64_t   *flag_x = nullptr, *flag_h = nullptr;
    uint64_t    seq = 0;
    bool        value_ops = false;
    bool        inkernel_sync = false;   // fork/join folded into the interior / pack / boundary kernels (no extra launches)
    uint64_t   *kflag_x = nullptr, *kflag_h = nullptr;   // their flags: device memory, one cache line each
    // host-routed transport (sgpu_debug_init_host_transport): no RCCL communicator, halos and reductions via callbacks
    sgpu_host_exchange_fn  xchg = nullptr;
    sgpu_host_allreduce_fn ared = nullptr;
    void                  *xuser = nullptr;
    bool multi() const { return comm != nullptr || xchg != nullptr; }
    std::vector<char> peer_seen;   // RCCL connects a peer lazily at the first send/recv with it (bit 0 send, bit 1 recv): see apply()
    double chain_us = 0.0;         // the exchange chain measured on this communicator at init (calibrate_chain), 0: not measured
};
Ctx g;

int need_ctx() { return g.live ? SGPU_OK : fail(SGPU_ERR_STATE, "sgpu_init has not been called"); }

// scalar sum over the ranks of a host-routed context
int host_allreduce(double *v, int n) {
    if (g.ared(g.xuser, v, n) != 0) return fail(SGPU_ERR_RCCL, "host transport: allreduce callback failed");
    return SGPU_OK;
}

// sum of a few host doubles over the ranks (setup-time decisions every rank must take alike); identity at one rank
int global_sum(double *v, int n);

// work vectors of n doubles: at least one element, so that an empty level still has a pointer
hipError_t alloc_vec(DevArr<double> &a, size_t n) { return a.alloc(std::max<size_t>(1, n)); }
int dev_alloc(DevArr<double> &a, size_t n) { return alloc_vec(a, n) == hipSuccess ? SGPU_OK : fail(SGPU_ERR_NOMEM, "hipMalloc failed"); }

template <class T>
int dev_upload(DevArr<T> &dst, const T *src, size_t n, size_t pad = 0) {
    const size_t bytes = (n + pad) * sizeof(T);
    if (dst.alloc(std::max<size_t>(1, n + pad)) != hipSuccess)
        return fail(SGPU_ERR_NOMEM, "hipMalloc of %zu bytes failed", bytes);
    if (pad) HIPCHK(hipMemsetAsync(dst, 0, dst.bytes(), g.cs));
    if (n) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    return SGPU_OK;
}

// One CSR part (local, or remote-over-halo) laid out for k_csr_stream.
//
// Its device arrays live in GROUPS, one per unit of lifetime: a group holds the arrays and the built / tried flags that a free
// clears with them, and `G = {}` frees it.  The scalars a launch reads (nslices, sl_pair, sl_uw, sp_w, sp_n, sp_bytes, sp2_uw,
// sp2_nslices, vi_uw8, xl_nblk ...) stay outside: a surviving form may read them after the arrays they were computed with are gone.
// Which plan keeps which group: plan_keeps() in forms.h, the one place a new form registers its storage.
struct CsrPart {
    int     nrows = 0;            // rows covered by row_ptr (M, or number of remote rows)
    int64_t nnz = 0;
    struct Csr { DevArr<int> row_ptr, col, blk_row, blk_row_big, rows; DevArr<double> val; } csr;
    int     nblk = 0, nblk_big = 0;
    int     lanes = 1;            // G
    int     variant = 0;          // 0 stream 16 KiB, 1 stream 32 KiB, 2 vector CSR, 3 cc16 16 KiB, 4 cc16 32 KiB, 5 dense rows
    struct Dense { DevArr<double> dense; } dn;   // variant 5: row-major nrows x ncols (built on demand for small, mostly full operators)
    int     ncols = 0;
    std::vector<double> h_val;    // host copy of the values, kept only while a dense form is still possible
    // 16-bit compressed columns (variants 3/4): per plan ([0] 16 KiB, [1] 32 KiB) a segment table and packed column ids
    struct Cc {
        DevArr<int> segtab, segptr;
        DevArr<unsigned short> ccol;
        bool ok = false;
        char tried = 0;           // build_cc16 ran and found no split that fits (do not try again)
    } cc[2];
    int     cc_ob[2] = {12, 12};  // offset bits of the slot/offset split (12: 16 segments of 4096 columns ... 8: 256 of 256)
    // column-major-in-block form (variants 7/8, on top of the compressed columns of the same plan)
    struct Cm {
        DevArr<double> val;
        DevArr<unsigned short> col, dst;
        DevArr<int> ptr;
        bool ok = false;
        char tried = 0;
    } cm[2];
    // sliced ELLPACK (variant 9): slices of 64 rows, position-major, 16-bit column offsets from a per-(slice, position) base.
    // The values (sl_val, sl_ptr, nslices, sl_pair) are what the row-pattern forms need ...
    struct SellValues {
        DevArr<double> sl_val;
        DevArr<int> sl_ptr;
        DevArr<int> sl_perm;      // k_sell<sorted>: slice position -> row (rows sorted by length inside windows of SL_SORT_WINDOW rows)
        bool sl_vals = false, sl_sorted = false;
        char sl_vals_tried = 0;
    } sv;
    // ... the column codes are k_sell's alone
    struct SellColumns {
        DevArr<unsigned short> sl_col, sl_len;
        DevArr<int> sl_base, sl_segptr;   // segment bases of all groups, group g owns [sl_segptr[g], sl_segptr[g+1])
    } sc;
    int             nslices = 0, sl_ob = 12;
    bool            sl_pair = false;       // two positions per lane side by side (rows of >= 16 entries), else one
    int             sl_uw = 0, sp2_uw = 0; // every slice of 64 (k_sell / k_sellp) / 128 (k_sellp2) rows has this many positions (0: widths differ)
    bool            sl_ok = false;         // values AND column codes: k_sell can run
    char            sl_tried = 0;          // (stays set when the column codes alone are dropped: variant 9 is then gone for good)
    // row patterns on top of the sliced-ELLPACK values (variant 11, k_sellp): a 16-bit pattern id per row and the table of
    // patterns (sp_n rows of sp_w + 1 ints: length, then the columns relative to the row); shares sl_val / sl_ptr
    struct Sellp {
        DevArr<unsigned short> sp_pat;
        DevArr<int> sp_tab;
        DevArr<int> sp_wgptr;     // sp_wide: table of row group g = sp_tab[sp_wgptr[g] .. sp_wgptr[g + 1])
        DevArr<int> sp_rbase;     // "k_sellp<rowbase>" (round 4): the patterns are relative to the row's FIRST COLUMN, kept here (a transfer operator
                                  // of a structured grid: its rows repeat relative to where they start, not to the row index); k_sellp only
        bool sp_ok = false, sp_wide = false;   // sp_wide: a table per group of 1024 rows (k_sellp<WIDE>; sp_w = the largest, in ints)
        char sp_tried = 0;
    } sp;
    int             sp_w = 0, sp_n = 0;
    int64_t         sp_bytes = 0;      // values + pattern ids + x + y as this form stores them
    // value-indexed row patterns (variant 17, k_vidx): 8-bit codes into per-workgroup dictionaries instead of the values; shares
    // sp_pat / sp_tab / sp_rbase
    struct Vidx {
        DevArr<unsigned char> vi_code;
        DevArr<int> vi_cptr, vi_dptr;
        DevArr<double> vi_dict;
        bool vi_ok = false;
        char vi_tried = 0;
    } vi;
    int             vi_uw8 = 0;           // every slice has this many code positions (a multiple of 8), or 0: read vi_cptr
    int64_t         vi_bytes = 0;         // codes + pattern ids + x + y as this form stores them
    int64_t         vi_code_bytes = 0;    // ... the codes alone (without the padding behind them)
    // ... launched with x in LDS windows (k_vidxw, a MODE of variant 17: sgpu_op_set_x_windows): per workgroup size R = 256 << k the
    // window list and the ONE table as 16-bit LDS byte offsets -- two small tables next to k_vidx's arrays -- and plan: what of
    // xwin_plan.h's plan every launch passes by value (the head, the common-path kernel's argument) or sizes its LDS by; vw_rows: the R in
    // use, 0 = direct gathers.  bits: the codes at one bit per entry (vw_fast.h), where the plan at this R keeps its dictionaries in scalar
    // registers -- packed from vi_code by build_xwin, read by k_vidxw_fast alone, and gone with the tables of this R.  masks: the rows
    // as lane masks (vw_masks.h), a record per slice, where the bit codes exist and the rule takes the table: same owner, same lifetime
    struct XWin { DevArr<unsigned short> tab; DevArr<int> win; DevArr<unsigned char> bits; DevArr<unsigned long long> masks; xwplan::VwScalars plan; bool ok = false; char tried = 0; };
    XWin            vw[3];
    int             vw_rows = 0;
    mutable int     vw_last = -1;         // what the last launch in the mode ran (0 k_vidxw, 1 / 2 k_vidxw_fast as fast_kind), -1: none since the mode was set
    mutable int     vw_last_width = -1;   // ... and the bits per entry of the code stream it read (8, or 1: the bit codes), -1: none
    mutable int     vw_last_rows = -1;    // ... and its row format (0: through the table, 1: lane masks), -1: none
    // x in LDS (variant 10): absolute 16-bit column ids and nnz-balanced row chunks, one per CU.  The chunk plan (k_sellx is built
    // on top of it) ...
    struct XldsPlan {
        DevArr<int> xl_blk;
        DevArr<int4> xl_info;
        DevArr<double> xl_acc;
        DevArr<int> xl_ord;       // [M] or empty: per chunk, the order its rows are taken in (longest first where a chunk holds long rows)
        bool xl_ok = false;
        char xl_tried = 0;
    } xlp;
    // ... and the columns, k_csr_xlds's alone
    struct XldsColumns { DevArr<unsigned short> xl_col; DevArr<int> xl_tab; } xlc;
    int             xl_nblk = 0, xl_maxt = 1;
    int             xl_win = 0;            // columns per window of x in LDS: XL_MAX, or less where the chunks' partial row sums live in LDS behind the window
    bool            xl_acc_lds = false;
    std::vector<int>  xl_blk_h;            // host copies of the chunk plan (k_sellx is built on top of it)
    std::vector<int4> xl_info_h;
    double          xl_piece = 0.0;
    // k_sellp with a lane per two rows (variant 14, k_sellp2): the values row-paired in slices of 128 rows; shares sp_pat / sp_tab
    struct Sellp2 { DevArr<double> sp2_val; DevArr<int> sp2_ptr; bool sp2_ok = false; char sp2_tried = 0; } sp2;
    int             sp2_nslices = 0;
    // k_sellp with x in LDS windows (variant 15, k_sellpx): the table as 16-bit LDS positions, the windows of x per workgroup;
    // shares sl_val / sl_ptr / sp_pat.  h_pstart / h_ptab: host copy of the patterns (start of each, then length + offsets), kept
    // until the plan settles
    std::vector<int> h_pstart, h_ptab;
    std::vector<unsigned short> h_pat;     // ... and of the rows' pattern ids
    struct Sellpx {
        DevArr<unsigned short> spx_tab, spx_pat;   // the workgroups' tables back to back; workgroup-local pattern ids per row
        DevArr<int> spx_win, spx_wgptr;            // windows (count, then omin / LDS base / size each); table of workgroup g: words [spx_wgptr[g], spx_wgptr[g + 1])
        bool spx_ok = false;
        char spx_tried = 0;
    } spx;
    // row templates (variant 13, k_rowt, opt-in): a template id per row; tables of (length, relative columns) and of values
    struct Rowt { DevArr<unsigned short> rt_pat; DevArr<int> rt_itab; DevArr<double> rt_vtab; bool rt_ok = false; char rt_tried = 0; } rt;
    int             rt_w = 0, rt_n = 0;
    // sliced ELLPACK inside the (chunk, window) blocks of the x-in-LDS form (variant 12, k_sellx): shares xl_blk / xl_info / xl_acc
    struct Sellx {
        DevArr<double> sx_val;
        DevArr<unsigned short> sx_col;
        DevArr<unsigned> sx_meta;
        DevArr<int> sx_bptr, sx_sptr;
        bool sx_ok = false;
        char sx_tried = 0;
    } sx;
    double          sx_pad = 0.0;          // stored / actual entries
    std::vector<int> h_rp, h_col, h_blk, h_blk_big;   // host copies kept for build_cc16 / the coarsest factorisation
};

// does the group hold memory? (sgpu_debug_op_storage)
unsigned part_storage_mask(const CsrPart &P) {
    const bool held[G_COUNT] = {
        P.csr.row_ptr || P.csr.col || P.csr.val || P.csr.blk_row || P.csr.blk_row_big || P.csr.rows,
        P.dn.dense != nullptr,
        P.cc[0].segtab || P.cc[0].segptr || P.cc[0].ccol, P.cc[1].segtab || P.cc[1].segptr || P.cc[1].ccol,
        P.cm[0].val || P.cm[0].col || P.cm[0].dst || P.cm[0].ptr, P.cm[1].val || P.cm[1].col || P.cm[1].dst || P.cm[1].ptr,
        P.sv.sl_val || P.sv.sl_ptr || P.sv.sl_perm,
        P.sc.sl_col || P.sc.sl_len || P.sc.sl_base || P.sc.sl_segptr,
        P.sp.sp_pat || P.sp.sp_tab || P.sp.sp_wgptr || P.sp.sp_rbase,
        P.vi.vi_code || P.vi.vi_cptr || P.vi.vi_dptr || P.vi.vi_dict,
        P.vw[0].tab || P.vw[0].win || P.vw[0].bits || P.vw[0].masks, P.vw[1].tab || P.vw[1].win || P.vw[1].bits || P.vw[1].masks,
        P.vw[2].tab || P.vw[2].win || P.vw[2].bits || P.vw[2].masks,
        P.sp2.sp2_val || P.sp2.sp2_ptr,
        P.spx.spx_tab || P.spx.spx_pat || P.spx.spx_win || P.spx.spx_wgptr,
        P.rt.rt_pat || P.rt.rt_itab || P.rt.rt_vtab,
        P.xlp.xl_blk || P.xlp.xl_info || P.xlp.xl_acc || P.xlp.xl_ord,
        P.xlc.xl_col || P.xlc.xl_tab,
        P.sx.sx_val || P.sx.sx_col || P.sx.sx_meta || P.sx.sx_bptr || P.sx.sx_sptr,
    };
    unsigned m = 0;
    for (int i = 0; i < G_COUNT; ++i) if (held[i]) m |= 1u << i;
    return m;
}

// How many leading slices of a sliced-ELLPACK operator beyond the 256 MiB Infinity Cache are read with plain loads (they
// allocate in the cache and the next sweep over the operator finds them there), the rest being non-temporal (they do not
// evict the resident part).  192 MiB of the 256: the level's vectors want their share.  SAENA_SELL_RESIDENT_MB overrides.
int resident_slices(int nslices, double bytes_per_slice) {
    static const double res_mb = std::getenv("SAENA_SELL_RESIDENT_MB") ? atof(std::getenv("SAENA_SELL_RESIDENT_MB")) : 192.0;
    if (res_mb <= 0 || nslices <= 0 || bytes_per_slice <= 0) return 0;
    return (int)std::min<double>((double)nslices, res_mb * 1048576.0 / bytes_per_slice);
}

int pow2floor(int x) { int p = 1; while (2 * p <= x) p *= 2; return p; }

// Row-block plan: consecutive rows while the block holds <= CAP products and
// <= MAXROWS rows; a row longer than CAP gets a block of its own.
void plan_blocks(const std::vector<int> &rp, std::vector<int> &blk, int cap, int maxrows) {
    const int M = (int)rp.size() - 1;
    blk.clear();
    blk.push_back(0);
    int r = 0;
    while (r < M) {
        const int start = r;
        const int p0 = rp[r];
        while (r < M && r - start < maxrows && rp[r + 1] - p0 <= cap) ++r;
        if (r == start) ++r;      // long row
        blk.push_back(r);
    }
}

int auto_lanes(int nrows, int nblk) {
    if (nblk <= 0 || nrows <= 0) return 1;
    const int rows_per_blk = std::max(1, (nrows + nblk - 1) / nblk);
    return std::min(64, std::max(1, pow2floor(sk::BLOCK / rows_per_blk)));
}

// (the host copies of the row pointers and columns are MOVED into the part: a level of a 16 M-row hierarchy holds 0.6 G entries)
int build_part(CsrPart &P, std::vector<int> &&rp, std::vector<int> &&col, const double *val, size_t nval, const std::vector<int> *rows) {
    P.nrows = (int)rp.size() - 1;
    P.nnz   = rp.back();
    std::vector<int> blk, blk_big;
    plan_blocks(rp, blk, sk::CAP, sk::MAXROWS);
    plan_blocks(rp, blk_big, sk::CAP_BIG, 2 * sk::MAXROWS);
    P.nblk  = (int)blk.size() - 1;
    P.nblk_big = (int)blk_big.size() - 1;
    P.lanes = auto_lanes(P.nrows, P.nblk);
    CHK(dev_upload(P.csr.blk_row_big, blk_big.data(), blk_big.size()));
    CHK(dev_upload(P.csr.row_ptr, rp.data(), rp.size()));
    CHK(dev_upload(P.csr.col, col.data(), col.size(), 8));
    CHK(dev_upload(P.csr.val, val, nval, 8));
    CHK(dev_upload(P.csr.blk_row, blk.data(), blk.size()));
    P.h_rp = std::move(rp); P.h_col = std::move(col); P.h_blk = blk; P.h_blk_big = blk_big;
    if (rows) CHK(dev_upload(P.csr.rows, rows->data(), rows->size()));
    return SGPU_OK;
}

// dense form of a small, mostly full operator (saena_matrix_dense: rows <= dense_sz_thre 5000 by default)
constexpr int DENSE_MAX_ROWS = 8192;
// Size limits only: at most 8192 rows and 64 M entries (512 MB) per rank.  WHEN the dense form is used is the caller's
// policy -- saena::amg applies the reference's density rule (density > dense_thre and rows <= dense_sz_thre,
// saena_object_setup2.cpp:328), the plan-time autotune tries it from 50 % fill on.
bool dense_candidate(int nrows, int ncols, int64_t nnz) {
    return nrows > 0 && ncols > 0 && nnz > 0 && nrows <= DENSE_MAX_ROWS && (int64_t)nrows * ncols <= (int64_t)DENSE_MAX_ROWS * DENSE_MAX_ROWS;
}
int build_dense(CsrPart &P) {
    if (P.dn.dense) return SGPU_OK;
    if (P.h_val.empty() || P.h_rp.empty()) return fail(SGPU_ERR_ARG, "this operator is too large for the dense form (more than 8192 rows or 64 M entries on this rank)");
    std::vector<double> d((size_t)P.nrows * P.ncols, 0.0);
    for (int i = 0; i < P.nrows; ++i)
        for (int k = P.h_rp[i]; k < P.h_rp[i + 1]; ++k) d[(size_t)i * P.ncols + P.h_col[k]] = P.h_val[k];
    CHK(dev_upload(P.dn.dense, d.data(), d.size()));
    return SGPU_OK;
}

// the remote part of the dense form: M x recvSize over the receive buffer (zero rows for the rows without remote entries)
int build_dense_rem(sgpu_op *op);

// 16-bit compressed columns of plan k: (slot << ob) | (col & (2^ob - 1)) with <= 2^(16-ob) segment bases per block.
// ob is the largest of 12..8 for which every block's distinct segments fit its slots (fewest table entries to read);
// blocks are independent, so the encoding runs on a few host threads.
int host_threads() {
    const char *e = std::getenv("SAENA_SETUP_THREADS");
    int n = e ? std::atoi(e) : (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(n, 16));
}
// 16-bit column codes of the local part over the row blocks `blk`: per block a table of segment bases (multiples of
// 2^ob), per entry (slot << ob) | (column & (2^ob - 1)) in CSR order.  Tries 4+12 bits down to 8+8; false: a block
// touches more than 256 segments of 256 columns.
bool encode_cc16(const CsrPart &P, const std::vector<int> &blk, std::vector<unsigned short> &ccol, std::vector<int> &segptr,
                 std::vector<int> &segtab, int &ob_out) {
    const int nblk = (int)blk.size() - 1;
    const int ncols = std::max(1, P.ncols);
    const int nt = std::min(host_threads(), std::max(1, nblk / 64));
    ccol.assign(P.h_col.size() + 8, 0);
    for (int ob = 12; ob >= 8; --ob) {
        const int maxseg = 1 << (16 - ob), nsegs_total = (ncols >> ob) + 1;
        std::vector<std::vector<int>> tabs((size_t)nt);         // per thread: the tables of its blocks, concatenated
        std::vector<int> cnt((size_t)nblk, 0);
        std::vector<char> bad((size_t)nt, 0);
        auto work = [&](int t) {
            const int b0 = (int)((long)nblk * t / nt), b1 = (int)((long)nblk * (t + 1) / nt);
            std::vector<int> slot_of((size_t)nsegs_total, -1), uniq;
            for (int b = b0; b < b1 && !bad[(size_t)t]; ++b) {
                const int p0 = P.h_rp[blk[b]], p1 = P.h_rp[blk[b + 1]];
                uniq.clear();
                int last = -1;
                for (int p = p0; p < p1; ++p) {                 // distinct segments of the block
                    const int sgm = P.h_col[p] >> ob;
                    if (sgm == last) continue;
                    last = sgm;
                    if (slot_of[(size_t)sgm] < 0) { slot_of[(size_t)sgm] = 0; uniq.push_back(sgm); }
                }
                if ((int)uniq.size() > maxseg) { bad[(size_t)t] = 1; for (int u : uniq) slot_of[(size_t)u] = -1; break; }
                std::sort(uniq.begin(), uniq.end());            // ascending bases: the table does not depend on the entry order
                for (size_t i = 0; i < uniq.size(); ++i) { slot_of[(size_t)uniq[i]] = (int)i; tabs[(size_t)t].push_back(uniq[i] << ob); }
                cnt[(size_t)b] = (int)uniq.size();
                const int om = (1 << ob) - 1;
                for (int p = p0; p < p1; ++p)
                    ccol[(size_t)p] = (unsigned short)((slot_of[(size_t)(P.h_col[p] >> ob)] << ob) | (P.h_col[p] & om));
                for (int u : uniq) slot_of[(size_t)u] = -1;
            }
        };
        if (nt == 1) work(0);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
            for (auto &x : th) x.join();
        }
        bool ok = true;
        for (char c : bad) ok = ok && !c;
        if (!ok) continue;                                       // too scattered for this split: try more, smaller segments
        segptr.assign((size_t)nblk + 1, 0);
        for (int b = 0; b < nblk; ++b) segptr[(size_t)b + 1] = segptr[(size_t)b] + cnt[(size_t)b];
        segtab.clear();
        segtab.reserve((size_t)segptr.back() + 1);
        for (auto &t : tabs) segtab.insert(segtab.end(), t.begin(), t.end());
        ob_out = ob;
        return true;
    }
    return false;
}

// The same encoding ON THE DEVICE (round 4), from the 32-bit columns already there: *ok = false when a block touches more than 256
// segments of 256 columns (the form does not apply) or the operator has more columns than the kernels' bitmap covers (the caller
// falls back to the host encoder).  d_blk: the row-block boundaries on the device; ccol gets nnz + 8 codes (CSR order).
int encode_cc16_device(const CsrPart &P, const int *d_blk, int nblk, DevArr<unsigned short> &ccol, DevArr<int> &segptr_d, DevArr<int> &segtab_d, int *ob_out, bool *ok, bool *host_fallback,
                       const int *d_perm = nullptr) {       // d_perm (k_sell<sorted>): d_blk bounds slice POSITIONS, position q holds row d_perm[q]
    *ok = false; *host_fallback = false;
    const int ncols = std::max(1, P.ncols);
    if (!P.csr.col || !P.csr.row_ptr || nblk <= 0) { *host_fallback = true; return SGPU_OK; }
    if (std::getenv("SAENA_HOST_CC16")) { *host_fallback = true; return SGPU_OK; }
    DevArr<int> d_cnt, d_bad;
    HIPCHK(d_cnt.alloc((size_t)nblk + 1));
    HIPCHK(d_bad.alloc(1));
    std::vector<int> cnt((size_t)nblk), segptr((size_t)nblk + 1, 0);
    for (int ob = 12; ob >= 8; --ob) {
        const int maxseg = 1 << (16 - ob), nsegs_total = (ncols >> ob) + 1, nwords = (nsegs_total + 31) / 32;
        if (nwords > sk::CC_BM_WORDS) { if (ob == 8) { *host_fallback = true; return SGPU_OK; } continue; }   // (a finer split needs a larger bitmap still)
        HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), g.cs));
        SGPU_LAUNCH(sk::k_cc16_count, dim3(nblk), dim3(sk::BLOCK), 0, g.cs, (const int *)P.csr.col, (const int *)P.csr.row_ptr, d_blk, ob, nwords, maxseg, d_cnt.get(), d_bad.get(), d_perm);
        HIPCHK(hipGetLastError());
        int bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        if (bad) continue;                                           // too scattered for this split: try more, smaller segments
        HIPCHK(hipMemcpy(cnt.data(), d_cnt, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < nblk; ++b) segptr[(size_t)b + 1] = segptr[(size_t)b] + cnt[(size_t)b];
        CHK(dev_upload(segptr_d, segptr.data(), segptr.size()));
        const size_t nt = (size_t)segptr.back() + 1;
        if (segtab_d.alloc(nt) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of the segment tables failed");
        HIPCHK(hipMemsetAsync(segtab_d, 0, nt * sizeof(int), g.cs));
        const size_t nc = (size_t)P.nnz + 8;
        if (ccol.alloc(nc) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of the column codes failed");
        HIPCHK(hipMemsetAsync(ccol, 0, nc * sizeof(unsigned short), g.cs));
        SGPU_LAUNCH(sk::k_cc16_encode, dim3(nblk), dim3(sk::BLOCK), 0, g.cs, (const int *)P.csr.col, (const int *)P.csr.row_ptr, d_blk, ob, nwords, (const int *)segptr_d, segtab_d.get(), ccol.get(), d_perm);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(g.cs));
        *ob_out = ob; *ok = true;
        return SGPU_OK;
    }
    return SGPU_OK;
}

int build_cc16(CsrPart &P, int k) {
    if (P.cc[k].ok || P.cc[k].tried || P.h_rp.empty()) return SGPU_OK;
    P.cc[k].tried = 1;
    const std::vector<int> &blk = k ? P.h_blk_big : P.h_blk;
    if (blk.size() < 2) return SGPU_OK;
    int ob = 12;
    {   // on the device, from the 32-bit columns already there (round 4)
        bool ok = false, fallback = false;
        CHK(encode_cc16_device(P, k ? P.csr.blk_row_big : P.csr.blk_row, (int)blk.size() - 1, P.cc[k].ccol, P.cc[k].segptr, P.cc[k].segtab, &ob, &ok, &fallback));
        if (ok) { P.cc_ob[k] = ob; P.cc[k].ok = true; return SGPU_OK; }
        if (!fallback) return SGPU_OK;                                    // a block touches more than 256 segments of 256 columns
    }
    std::vector<unsigned short> ccol;
    std::vector<int> segptr, segtab;
    if (!encode_cc16(P, blk, ccol, segptr, segtab, ob)) return SGPU_OK;   // a block touches more than 256 segments of 256 columns
    CHK(dev_upload(P.cc[k].segtab, segtab.data(), segtab.size(), 1));
    CHK(dev_upload(P.cc[k].segptr, segptr.data(), segptr.size()));
    CHK(dev_upload(P.cc[k].ccol, ccol.data(), ccol.size()));
    P.cc_ob[k] = ob;
    P.cc[k].ok = true;
    return SGPU_OK;
}

// column-major-in-block form of plan k (needs the compressed columns of the same plan and the host copy of the values)
int build_cm(CsrPart &P, int k, const std::vector<double> &h_val_all) {
    if (P.cm[k].ok || P.cm[k].tried || P.h_rp.empty()) return SGPU_OK;
    P.cm[k].tried = 1;
    CHK(build_cc16(P, k));
    const bool on_device = P.csr.val && P.csr.col && P.cc[k].ccol && P.csr.row_ptr && !std::getenv("SAENA_HOST_CM_BUILD");
    if (!P.cc[k].ok || (!on_device && h_val_all.size() != P.h_col.size())) return SGPU_OK;
    const std::vector<int> &blk = k ? P.h_blk_big : P.h_blk;
    const int cap = k ? sk::CAP_BIG : sk::CAP;
    const int nblk = (int)blk.size() - 1;
    if (nblk == 0) return SGPU_OK;
    std::vector<int> cmptr((size_t)nblk + 1, 0);
    for (int b = 0; b < nblk; ++b) {
        const int n = P.h_rp[blk[b + 1]] - P.h_rp[blk[b]];
        if (n > cap) return SGPU_OK;                               // long rows: not in this form
        if (n == 0) return SGPU_OK;                                // a block of rows without local entries (a transfer operator's
                                                                   // rows whose entries are all remote): the kernel would decode the
                                                                   // next block's first quad through an empty segment table
        cmptr[(size_t)b + 1] = cmptr[(size_t)b] + ((n + 3) & ~3);
    }
    const size_t tot = (size_t)cmptr[(size_t)nblk];
    if (P.csr.val && P.csr.col && P.cc[k].ccol && P.csr.row_ptr && !std::getenv("SAENA_HOST_CM_BUILD")) {
        // on the device (round 4): the block's entries sorted by (column, CSR position) in LDS, values and column codes taken from the
        // arrays already there
        CHK(dev_upload(P.cm[k].ptr, cmptr.data(), cmptr.size()));
        const size_t nv = tot + 8;
        if (P.cm[k].val.alloc(nv) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of the column-ordered values failed");
        if (P.cm[k].col.alloc(nv) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of the column-ordered codes failed");
        if (P.cm[k].dst.alloc(nv) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of the tile slots failed");
        HIPCHK(hipMemsetAsync(P.cm[k].val, 0, nv * sizeof(double), g.cs));
        HIPCHK(hipMemsetAsync(P.cm[k].col, 0, nv * sizeof(unsigned short), g.cs));
        HIPCHK(hipMemsetAsync(P.cm[k].dst, 0xff, nv * sizeof(unsigned short), g.cs));      // (the 8 spare entries past the end: never a valid slot)
        const int *d_blk = k ? P.csr.blk_row_big : P.csr.blk_row;
        if (k) SGPU_LAUNCH(sk::k_cm_build<sk::CAP_BIG>, dim3(nblk), dim3(sk::BLOCK), 0, g.cs, (const double *)P.csr.val, (const int *)P.csr.col, (const unsigned short *)P.cc[k].ccol,
                           (const int *)P.csr.row_ptr, d_blk, (const int *)P.cm[k].ptr, P.cm[k].val, P.cm[k].col, P.cm[k].dst);
        else SGPU_LAUNCH(sk::k_cm_build<sk::CAP>, dim3(nblk), dim3(sk::BLOCK), 0, g.cs, (const double *)P.csr.val, (const int *)P.csr.col, (const unsigned short *)P.cc[k].ccol,
                         (const int *)P.csr.row_ptr, d_blk, (const int *)P.cm[k].ptr, P.cm[k].val, P.cm[k].col, P.cm[k].dst);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(g.cs));
        P.cm[k].ok = true;
        return SGPU_OK;
    }
    // the 16-bit column codes of plan k live on the device only: re-encode on the host with the block's (sorted) table
    const int ob = P.cc_ob[k], om = (1 << ob) - 1;
    std::vector<double> val(tot + 8, 0.0);
    std::vector<unsigned short> col(tot + 8, 0), dst(tot + 8, (unsigned short)(cap + 4));
    const int nt = std::min(host_threads(), std::max(1, nblk / 64));
    auto work = [&](int t) {
        const int b0 = (int)((long)nblk * t / nt), b1 = (int)((long)nblk * (t + 1) / nt);
        std::vector<int> order, uniq;
        for (int b = b0; b < b1; ++b) {
            const int p0 = P.h_rp[blk[b]], p1 = P.h_rp[blk[b + 1]], n = p1 - p0, a0 = p0 & ~3;
            uniq.clear();
            for (int p = p0; p < p1; ++p) uniq.push_back(P.h_col[p] >> ob);
            std::sort(uniq.begin(), uniq.end());
            uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());      // the block's segment table (ascending, as build_cc16 made it)
            order.resize((size_t)n);
            for (int i = 0; i < n; ++i) order[(size_t)i] = p0 + i;
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return P.h_col[x] < P.h_col[y]; });   // (column, then row: CSR order is row-major)
            const size_t o = (size_t)cmptr[(size_t)b];
            for (int i = 0; i < n; ++i) {
                const int p = order[(size_t)i];
                const int slot = (int)(std::lower_bound(uniq.begin(), uniq.end(), P.h_col[p] >> ob) - uniq.begin());
                val[o + i] = h_val_all[(size_t)p];
                col[o + i] = (unsigned short)((slot << ob) | (P.h_col[p] & om));
                dst[o + i] = (unsigned short)(p - a0);
            }
            for (int i = n; i < ((n + 3) & ~3); ++i) col[o + i] = n ? col[o] : 0;    // padding: a valid column, value 0, the spare slot
        }
    };
    if (nt == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
        for (auto &x : th) x.join();
    }
    CHK(dev_upload(P.cm[k].val, val.data(), val.size()));
    CHK(dev_upload(P.cm[k].col, col.data(), col.size()));
    CHK(dev_upload(P.cm[k].dst, dst.data(), dst.size()));
    CHK(dev_upload(P.cm[k].ptr, cmptr.data(), cmptr.size()));
    P.cm[k].ok = true;
    return SGPU_OK;
}

// x-in-LDS form of the local part (k_csr_xlds): the rows cut into one nnz-balanced chunk per CU, the columns a chunk
// touches into windows of XL_MAX; 16-bit column ids relative to the window, per chunk a table of each row's entry offsets
// per window.  Refused when a chunk needs more than XL_MAXT windows.
int build_xlds(CsrPart &P) {
    if (P.xlp.xl_ok || P.xlp.xl_tried || P.h_rp.empty()) return SGPU_OK;
    P.xlp.xl_tried = 1;
    const int M = P.nrows;
    if (M == 0 || P.nnz == 0) return SGPU_OK;
    const int nb = std::min(std::max(1, sk::XL_PER_CU * g.ncu), M);
    std::vector<int> blk((size_t)nb + 1, 0);
    for (int b = 1; b < nb; ++b) {                                 // row whose prefix reaches b/nb of the entries
        const int64_t target = (int64_t)P.nnz * b / nb;
        int r = (int)(std::lower_bound(P.h_rp.begin(), P.h_rp.end(), (int)target) - P.h_rp.begin());
        blk[(size_t)b] = std::min(M, std::max(r, blk[(size_t)b - 1]));
    }
    blk[(size_t)nb] = M;
    std::vector<int4> info((size_t)nb);
    std::vector<int> cmins((size_t)nb), cmaxs((size_t)nb);
    int maxrows = 0;
    for (int b = 0; b < nb; ++b) {
        int cmin = INT32_MAX, cmax = -1;
        for (int r = blk[b]; r < blk[b + 1]; ++r)
            if (P.h_rp[r + 1] > P.h_rp[r]) { cmin = std::min(cmin, P.h_col[(size_t)P.h_rp[r]]); cmax = std::max(cmax, P.h_col[(size_t)P.h_rp[r + 1] - 1]); }
        if (cmax < 0) { cmin = 0; cmax = 0; }
        cmins[(size_t)b] = cmin; cmaxs[(size_t)b] = cmax;
        maxrows = std::max(maxrows, blk[b + 1] - blk[b]);
    }
    // The window: all XL_MAX doubles of the LDS array -- or, where chunks reach over several windows, XL_MAX less the chunk's rows:
    // a row's partial sum then travels from window to window in LDS behind the window of x (round 4) instead of through global
    // memory (`acc`: an 8-byte load and store per (row, window), the load at the end of a row's chain of dependent round trips).
    // Measured on the 256^3 hierarchy: R2 (k_csr_xlds, 7 windows) 160.6 -> 153.0 us, level 3 292.0 -> 287.2, R3 79.4 -> 77.9; k_sellx on
    // the 263-entry level unchanged (407 us either way).  Kept in global memory where a chunk holds more rows than a quarter of the array.
    auto windows = [&](int win) {
        int mt = 1;
        for (int b = 0; b < nb; ++b) mt = std::max(mt, (cmaxs[(size_t)b] - cmins[(size_t)b]) / win + 1);
        return mt;
    };
    int win = sk::XL_MAX, maxt = windows(sk::XL_MAX);
    if (maxt > sk::XL_MAXT) return SGPU_OK;
    bool acc_lds = false;
    if (maxt > 1 && maxrows <= sk::XL_MAX / 4 && !std::getenv("SAENA_XLDS_GLOBAL_ACC")) {
        const int win2 = sk::XL_MAX - (maxrows + 63) / 64 * 64;
        const int mt2 = windows(win2);
        if (mt2 <= sk::XL_MAXT) { win = win2; maxt = mt2; acc_lds = true; }
    }
    int64_t tabsz = 0, pieces = 0;
    for (int b = 0; b < nb; ++b) {
        const int T = (cmaxs[(size_t)b] - cmins[(size_t)b]) / win + 1, rows = blk[b + 1] - blk[b];
        info[(size_t)b] = make_int4(cmins[(size_t)b], T, (int)tabsz, 0);
        tabsz += (int64_t)rows * (T + 1);
        pieces += (int64_t)rows * T;
        if (tabsz > INT32_MAX / 2) return SGPU_OK;
    }
    P.xl_win = win; P.xl_acc_lds = acc_lds;
    // Longest rows first in the chunks that hold rows of more than 8x the chunk's mean length (BASELINE configs[4]: hub rows of 3 000
    // entries among rows of 34): a group that STARTS such a row last is the tail of its workgroup, and that workgroup the tail of the
    // launch.  A stable sort by length, descending, of the chunk's rows; other chunks keep the natural order (no array at all when no
    // chunk qualifies).  Same sums: only the order in which rows are picked up changes.
    if (!std::getenv("SAENA_XLDS_NATURAL_ORDER")) {
        std::vector<int> ord;
        for (int b = 0; b < nb; ++b) {
            const int r0 = blk[b], rows = blk[b + 1] - r0;
            if (rows < 2) continue;
            int longest = 0;
            for (int r = r0; r < r0 + rows; ++r) longest = std::max(longest, P.h_rp[r + 1] - P.h_rp[r]);
            const double mean = (double)(P.h_rp[r0 + rows] - P.h_rp[r0]) / rows;
            if ((double)longest <= 8.0 * std::max(mean, 1.0)) continue;
            if (ord.empty()) { ord.resize((size_t)M); for (int c = 0; c < nb; ++c) for (int r = blk[c]; r < blk[c + 1]; ++r) ord[(size_t)r] = r - blk[c]; }
            std::stable_sort(ord.begin() + r0, ord.begin() + r0 + rows, [&](int x, int y) {
                return P.h_rp[r0 + x + 1] - P.h_rp[r0 + x] > P.h_rp[r0 + y + 1] - P.h_rp[r0 + y]; });
        }
        if (!ord.empty()) CHK(dev_upload(P.xlp.xl_ord, ord.data(), ord.size()));
    }
    P.xl_piece = (double)P.nnz / (double)std::max<int64_t>(1, pieces);    // mean entries per (row, window): the autotune wants >= 24
    P.xl_blk_h = blk; P.xl_info_h = info;
    CHK(dev_upload(P.xlp.xl_blk, blk.data(), blk.size()));
    CHK(dev_upload(P.xlp.xl_info, info.data(), info.size()));
    if (P.csr.col && P.csr.row_ptr && !std::getenv("SAENA_HOST_XLDS_BUILD")) {
        // the window-relative columns and the (row, window) offsets on the device, from the 32-bit columns already there (round 4)
        const size_t nc = P.h_col.size() + 8, ntab = (size_t)tabsz + 1;
        if (P.xlc.xl_col.alloc(nc) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of the x-in-LDS columns failed");
        if (P.xlc.xl_tab.alloc(ntab) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of the x-in-LDS table failed");
        HIPCHK(hipMemsetAsync(P.xlc.xl_col, 0, nc * sizeof(unsigned short), g.cs));
        HIPCHK(hipMemsetAsync(P.xlc.xl_tab, 0, ntab * sizeof(int), g.cs));
        SGPU_LAUNCH(sk::k_xlds_build, dim3(nb), dim3(sk::BLOCK), 0, g.cs, (const int *)P.csr.col, (const int *)P.csr.row_ptr, (const int *)P.xlp.xl_blk, (const int4 *)P.xlp.xl_info,
                    P.xlc.xl_tab, P.xlc.xl_col, win);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(g.cs));
    } else {
    std::vector<unsigned short> col(P.h_col.size() + 8, 0);
    std::vector<int> tab((size_t)tabsz + 1, 0);
    const int nt = std::min(host_threads(), std::max(1, nb / 8));
    auto work = [&](int t) {
        for (int b = (int)((long)nb * t / nt); b < (int)((long)nb * (t + 1) / nt); ++b) {
            const int r0 = blk[b], rows = blk[b + 1] - r0, cmin = info[(size_t)b].x, T = info[(size_t)b].y;
            int *tb = tab.data() + info[(size_t)b].z;
            for (int k = 0; k < rows; ++k) {
                const int p0 = P.h_rp[r0 + k], p1 = P.h_rp[r0 + k + 1];
                int p = p0;
                for (int w = 0; w <= T; ++w) {                     // columns ascend along a row: the windows cut it into consecutive pieces
                    const int lim = w == T ? INT32_MAX : cmin + w * win;
                    while (p < p1 && P.h_col[(size_t)p] < lim) {
                        col[(size_t)p] = (unsigned short)(P.h_col[(size_t)p] - (cmin + (w - 1) * win));
                        ++p;
                    }
                    tb[(size_t)w * rows + k] = w == T ? p1 : p;
                }
            }
        }
    };
    if (nt == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
        for (auto &x : th) x.join();
    }
    CHK(dev_upload(P.xlc.xl_col, col.data(), col.size()));
    CHK(dev_upload(P.xlc.xl_tab, tab.data(), tab.size()));
    }
    if (maxt > 1 && !acc_lds) HIPCHK(P.xlp.xl_acc.alloc((size_t)M));
    P.xl_nblk = nb;
    P.xl_maxt = maxt;
    P.xlp.xl_ok = true;
    return SGPU_OK;
}

// Sliced ELLPACK of the local part (k_sell): slices of 64 rows stored position-major in pairs of positions per lane, padded to the slice's longest row;
// 16-bit column codes against a segment table per group of 4 slices (one workgroup), as in build_cc16.  Built only where
// it can win: padding <= 12 % of the entries.
// (round 4) The VALUES are re-ordered on the device from the CSR values already there (k_sell_scatter: 1.0 s -> a few ms for the 558 M
// entries of 256^3 level 1) and are all the row-pattern forms need; the 16-bit column codes -- a host pass over the entries plus
// 2 B per entry of upload -- are made only when k_sell itself is a candidate (operators whose rows follow no patterns).
// all slices of `rows` rows equally wide (a stencil level)?  -> that width, 0 otherwise.  A narrower LAST slice (its rows are
// boundary rows) is padded up: a few KiB that let the kernels compute a slice's start instead of loading it.
int uniform_width(std::vector<int> &ptr, int rows, int64_t *tot) {
    const int ns = (int)ptr.size() - 1;
    if (ns < 1 || std::getenv("SAENA_NO_UNIFORM_WIDTH")) return 0;
    const int w0 = (ptr[1] - ptr[0]) / rows;
    if (w0 == 0) return 0;
    for (int s = 1; s + 1 < ns; ++s) if ((ptr[(size_t)s + 1] - ptr[(size_t)s]) / rows != w0) return 0;
    const int wl = (ptr[(size_t)ns] - ptr[(size_t)ns - 1]) / rows;
    if (wl > w0) return 0;
    if (wl < w0) {
        if ((int64_t)ptr[(size_t)ns - 1] + (int64_t)w0 * rows > (int64_t)INT32_MAX - 1024) return 0;
        ptr[(size_t)ns] = ptr[(size_t)ns - 1] + w0 * rows;
        *tot = ptr[(size_t)ns];
    }
    return w0;
}

// k_sell<sorted>: the window the rows are sorted in (a multiple of the 256 rows of a workgroup; y, rhs, inv_diag of a wave's rows lie
// anywhere inside it: 16 KiB per vector at 2048)
static const int SL_SORT_WINDOW = [] {
    const char *e = std::getenv("SAENA_SELL_SORT_WINDOW");
    const int w = e ? std::atoi(e) : 2048;
    return std::max(256, (w / 256) * 256);
}();
int build_sell_values(CsrPart &P) {
    if (P.sv.sl_vals || P.sv.sl_vals_tried || P.h_rp.empty() || !P.csr.val || !P.csr.row_ptr) return SGPU_OK;
    P.sv.sl_vals_tried = 1;
    const int M = P.nrows;
    if (M == 0) return SGPU_OK;
    const int ns = (M + 63) / 64;
    std::vector<int> ptr((size_t)ns + 1, 0);
    int64_t tot = 0;
    for (int s = 0; s < ns; ++s) {
        int w = 0;
        for (int r = s * 64; r < std::min(M, s * 64 + 64); ++r) w = std::max(w, P.h_rp[r + 1] - P.h_rp[r]);
        if (w > 65535) return SGPU_OK;
        tot += (int64_t)w * 64;
        if (tot > (int64_t)INT32_MAX - 1024) return SGPU_OK;
        ptr[(size_t)s + 1] = (int)tot;
    }
    static const double pad_limit = std::getenv("SAENA_SELL_PAD") ? atof(std::getenv("SAENA_SELL_PAD")) : 1.12;
    std::vector<int> perm;
    if ((double)tot > pad_limit * (double)P.nnz) {
        // uneven rows (a transfer operator: P1 of 256^3 pads 20 %): the rows SORTED by length inside windows of SL_SORT_WINDOW rows
        // (a stable counting sort: rows of one length keep their order) pad 1-2 %.  The slices then hold a permutation of the
        // window's rows; k_sell's epilogue goes through sl_perm.  No pattern form on top.
        // OPT-IN (SAENA_SELL_SORTED=1): measured on the two operators it was built for it LOSES -- P1 of 256^3 400-423 us against 361-367
        // on 32 KiB tiles of 16-bit columns, P2 156-171 against 116 (k_csr_xldsr) / 137 us; windows of 512 / 2048 / 8192 rows, plain or
        // non-temporal stores alike (profiles/r04_sell_sorted_windows.log): the 64 rows of a wave are no longer neighbours, so a
        // gather instruction names ~32x the lines of x it named, and that -- not the 20 % of padding -- is what these kernels pay for.
        if (!std::getenv("SAENA_SELL_SORTED") || P.nnz < 4 * (int64_t)M) return SGPU_OK;
        perm.resize((size_t)ns * 64);
        std::vector<int> cnt;
        for (int w0 = 0; w0 < M; w0 += SL_SORT_WINDOW) {
            const int w1 = std::min(M, w0 + SL_SORT_WINDOW);
            int wmax = 0;
            for (int r = w0; r < w1; ++r) wmax = std::max(wmax, P.h_rp[r + 1] - P.h_rp[r]);
            cnt.assign((size_t)wmax + 2, 0);
            for (int r = w0; r < w1; ++r) ++cnt[(size_t)(wmax - (P.h_rp[r + 1] - P.h_rp[r])) + 1];      // longest rows first
            for (int l = 0; l <= wmax; ++l) cnt[(size_t)l + 1] += cnt[(size_t)l];
            for (int r = w0; r < w1; ++r) perm[(size_t)w0 + (size_t)cnt[(size_t)(wmax - (P.h_rp[r + 1] - P.h_rp[r]))]++] = r;
        }
        for (size_t q = (size_t)M; q < perm.size(); ++q) perm[q] = (int)q;                                 // (positions past the last row: never read)
        tot = 0;
        for (int s = 0; s < ns; ++s) {
            const int r = perm[(size_t)s * 64];                      // the longest row of the slice is its first
            tot += (int64_t)(P.h_rp[r + 1] - P.h_rp[r]) * 64;
            ptr[(size_t)s + 1] = (int)tot;
        }
        static const double sorted_limit = std::getenv("SAENA_SELL_SORTED_PAD") ? atof(std::getenv("SAENA_SELL_SORTED_PAD")) : 1.05;
        if ((double)tot > sorted_limit * (double)P.nnz) return SGPU_OK;
        CHK(dev_upload(P.sv.sl_perm, perm.data(), perm.size()));
        P.sv.sl_sorted = true;
    }
    if (!P.sv.sl_sorted) P.sl_uw = uniform_width(ptr, 64, &tot);      // (pads the last slice up to the others' width where that makes them all equal)
    // 16-byte value loads pay from a few pairs per row on, and on any operator that streams from HBM (256^3 L0, 7 entries
    // per row: 338 vs 343-350 us); the cache-resident 128^3 fine level is the one case that prefers single positions
    const bool pair = P.nnz >= 16 * (int64_t)M || 10 * P.nnz > (int64_t)256 * 1024 * 1024;
    P.sl_pair = pair;
    CHK(dev_upload(P.sv.sl_ptr, ptr.data(), ptr.size()));
    const size_t nv = (size_t)tot + 64;
    if (P.sv.sl_val.alloc(nv) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of %zu bytes failed", nv * sizeof(double));
    HIPCHK(hipMemsetAsync(P.sv.sl_val, 0, nv * sizeof(double), g.cs));
    SGPU_LAUNCH(sk::k_sell_scatter<double>, dim3((M + sk::BLOCK - 1) / sk::BLOCK), dim3(sk::BLOCK), 0, g.cs, (const double *)P.csr.val, (const int *)P.csr.row_ptr,
                (const int *)P.sv.sl_ptr, P.sv.sl_val, M, pair ? 1 : 0, (const int *)P.sv.sl_perm);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.cs));
    P.nslices = ns;
    P.sv.sl_vals = true;
    return SGPU_OK;
}

int build_sell(CsrPart &P, const std::vector<double> &) {
    if (P.sl_ok || P.sl_tried || P.h_rp.empty()) return SGPU_OK;
    P.sl_tried = 1;
    CHK(build_sell_values(P));
    if (!P.sv.sl_vals) return SGPU_OK;
    const int M = P.nrows, ns = P.nslices;
    std::vector<int> grp;                                        // row groups of one workgroup: 4 slices
    for (int r = 0; r < M; r += 256) grp.push_back(r);
    grp.push_back(M);
    std::vector<unsigned short> ccol, len((size_t)ns * 64, 0);
    std::vector<int> segptr, segtab;
    int ob = 12;
    if (P.sv.sl_sorted) {                                            // the length of the row that sits at each slice position
        std::vector<int> perm((size_t)ns * 64);
        HIPCHK(hipMemcpy(perm.data(), P.sv.sl_perm, perm.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int q = 0; q < M; ++q) len[(size_t)q] = (unsigned short)(P.h_rp[perm[(size_t)q] + 1] - P.h_rp[perm[(size_t)q]]);
    } else
    for (int r = 0; r < M; ++r) len[(size_t)r] = (unsigned short)(P.h_rp[r + 1] - P.h_rp[r]);
    // the codes in CSR order (made on the device where the bitmap covers the operator's columns, else on the host and uploaded)
    // take the values' way into the slice layout (padding keeps code 0: slot 0, offset 0 = a valid column of the group)
    DevArr<unsigned short> d_ccol;
    bool dev_tabs = false;
    {
        DevArr<int> d_grp;
        CHK(dev_upload(d_grp, grp.data(), grp.size()));
        bool ok = false, fallback = false;
        CHK(encode_cc16_device(P, d_grp, (int)grp.size() - 1, d_ccol, P.sc.sl_segptr, P.sc.sl_base, &ob, &ok, &fallback, P.sv.sl_perm));
        if (ok) dev_tabs = true;
        else if (!fallback || P.sv.sl_sorted) return SGPU_OK;             // (the host encoder knows no permutation: operators of more columns than the device's bitmap covers keep CSR)
    }
    if (!dev_tabs) {
        if (!encode_cc16(P, grp, ccol, segptr, segtab, ob)) return SGPU_OK;
        CHK(dev_upload(d_ccol, ccol.data(), ccol.size()));
    }
    int tot = 0;
    HIPCHK(hipMemcpy(&tot, P.sv.sl_ptr + ns, sizeof(int), hipMemcpyDeviceToHost));
    const size_t nc = (size_t)tot + 64;
    if (P.sc.sl_col.alloc(nc) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of %zu bytes failed", nc * 2);
    HIPCHK(hipMemsetAsync(P.sc.sl_col, 0, nc * sizeof(unsigned short), g.cs));
    SGPU_LAUNCH(sk::k_sell_scatter<unsigned short>, dim3((M + sk::BLOCK - 1) / sk::BLOCK), dim3(sk::BLOCK), 0, g.cs, (const unsigned short *)d_ccol, (const int *)P.csr.row_ptr,
                (const int *)P.sv.sl_ptr, P.sc.sl_col, M, P.sl_pair ? 1 : 0, (const int *)P.sv.sl_perm);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.cs));
    if (std::getenv("SAENA_SETUP_TIMING"))
        fprintf(stderr, "[sgpu] sliced ELLPACK%s: %d rows, %lld entries, %.1f %% padding, columns %d+%d bits\n", P.sv.sl_sorted ? " (rows sorted by length per window)" : "",
                M, (long long)P.nnz, 100.0 * ((double)tot / (double)P.nnz - 1.0), 16 - ob, ob);
    CHK(dev_upload(P.sc.sl_len, len.data(), len.size()));
    if (!dev_tabs) {
        CHK(dev_upload(P.sc.sl_base, segtab.data(), segtab.size(), 1));
        CHK(dev_upload(P.sc.sl_segptr, segptr.data(), segptr.size()));
    }
    P.sl_ob = ob;
    P.sl_ok = true;
    return SGPU_OK;
}

// Row patterns of the local part (k_sellp) on top of build_sell's values: every row is (length, columns relative to the
// row index); the operator qualifies when its rows follow at most 65 535 distinct patterns and
//   * they fit 4096 ints at a fixed width of (longest row + 1) -- stencils on structured grids (the boundary-stripped 7-point
//     Laplacian: 27 patterns), band matrices: ONE table for k_sellp / k_sellp2 with 256 threads per workgroup; or
//   * the patterns that 1024 consecutive rows follow fit SPW_MAX_TABLE ints, group of rows by group (sp_wide) -- the first
//     smoothed-aggregation level of a structured grid (Poisson level 1: 321 patterns at every size, ~400 in the local part of a
//     rank with two neighbours; a group meets a few dozen): every workgroup of k_sellp<WIDE> gets its own table (start offsets,
//     then length + offsets per pattern) and the rows' ids count within it.
// Ids are dealt in order of first appearance, so the tables do not depend on threads or hashing.
constexpr int SP_MAX_TABLE = 4096;
// rowbase = false: a pattern is (length, columns relative to the ROW INDEX) -- square operators of a structured grid.
// rowbase = true (round 4): ... relative to the row's FIRST COLUMN, which k_sellp then reads per row (4 B): the level-0 transfers of the
// Poisson hierarchy repeat 30 (R0) / 33 (P0) such patterns where they follow tens of thousands relative to the row index.
int build_sellp_mode(CsrPart &P, bool rowbase);
int build_sellp(CsrPart &P) {
    if (P.sp.sp_ok || P.sp.sp_tried || !P.sv.sl_vals || P.sv.sl_sorted || P.h_rp.empty()) return SGPU_OK;     // (sorted slices: positions are not rows)
    P.sp.sp_tried = 1;
    CHK(build_sellp_mode(P, false));
    if (!P.sp.sp_ok && !std::getenv("SAENA_NO_SELLP_ROWBASE")) CHK(build_sellp_mode(P, true));
    return SGPU_OK;
}
int build_sellp_mode(CsrPart &P, bool rowbase) {
    const int M = P.nrows;
    auto ref = [&](int r) { return !rowbase ? r : (P.h_rp[r + 1] > P.h_rp[r] ? P.h_col[(size_t)P.h_rp[r]] : 0); };
    int W = 1;
    for (int r = 0; r < M; ++r) W = std::max(W, P.h_rp[r + 1] - P.h_rp[r]);
    if (W + 3 > sk::SPW_MAX_TABLE) return SGPU_OK;
    const size_t max_ints = (size_t)P.nnz / 8 + 65536;          // an operator whose patterns hold an eighth of its entries is not this kind of operator
    std::vector<int> ctab, cstart;                             // patterns back to back: length, then that many offsets
    std::vector<unsigned short> pat(((size_t)M + 127) / 128 * 128, 0);
    int npat = 0;
    {
        // (round 4) on the host's threads: every thread finds the patterns of a contiguous range of rows with a dictionary of its own
        // (local ids in order of first appearance); the ranges are then merged IN ORDER into the global dictionary, so the global ids
        // are dealt in order of first appearance over all rows -- what the one-thread loop produced -- whatever the thread count
        const int nt = std::max(1, std::min(host_threads(), M / 65536));
        struct Part { std::vector<int> ctab, cstart; std::vector<int> ids; bool overflow = false; };     // ids: the local id of every row of the range
        std::vector<Part> parts((size_t)nt);
        auto work = [&](int t) {
            Part &Q = parts[(size_t)t];
            const int r0 = (int)((long)M * t / nt), r1 = (int)((long)M * (t + 1) / nt);
            Q.ids.resize((size_t)(r1 - r0));
            std::unordered_map<std::string, int> ids;
            std::string key;
            int prev = -1, np = 0;
            for (int r = r0; r < r1; ++r) {
                const int p0 = P.h_rp[r], n = P.h_rp[r + 1] - p0, rf = ref(r);
                if (prev >= 0 && Q.ctab[(size_t)Q.cstart[(size_t)prev]] == n) {   // most rows repeat the row before
                    const int *tt = &Q.ctab[(size_t)Q.cstart[(size_t)prev] + 1];
                    int j = 0;
                    while (j < n && P.h_col[(size_t)p0 + j] - rf == tt[j]) ++j;
                    if (j == n) { Q.ids[(size_t)(r - r0)] = prev; continue; }
                }
                key.assign(reinterpret_cast<const char *>(&n), sizeof n);
                for (int j = 0; j < n; ++j) { const int o = P.h_col[(size_t)p0 + j] - rf; key.append(reinterpret_cast<const char *>(&o), sizeof o); }
                auto it = ids.find(key);
                if (it == ids.end()) {
                    if (np == 65535 || Q.ctab.size() + (size_t)n + 1 > max_ints) { Q.overflow = true; return; }
                    it = ids.emplace(key, np++).first;
                    Q.cstart.push_back((int)Q.ctab.size());
                    Q.ctab.push_back(n);
                    for (int j = 0; j < n; ++j) Q.ctab.push_back(P.h_col[(size_t)p0 + j] - rf);
                }
                prev = it->second;
                Q.ids[(size_t)(r - r0)] = prev;
            }
        };
        if (nt == 1) work(0);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
            for (auto &x : th) x.join();
        }
        std::unordered_map<std::string, int> gids;
        std::vector<std::vector<int>> remap((size_t)nt);
        for (int t = 0; t < nt; ++t) {
            const Part &Q = parts[(size_t)t];
            if (Q.overflow) return SGPU_OK;
            remap[(size_t)t].resize(Q.cstart.size());
            for (size_t i = 0; i < Q.cstart.size(); ++i) {                      // the range's patterns in ITS order of first appearance
                const int *c = &Q.ctab[(size_t)Q.cstart[i]];
                const std::string key(reinterpret_cast<const char *>(c), ((size_t)c[0] + 1) * sizeof(int));
                auto it = gids.find(key);
                if (it == gids.end()) {
                    if (npat == 65535 || ctab.size() + (size_t)c[0] + 1 > max_ints) return SGPU_OK;
                    it = gids.emplace(key, npat++).first;
                    cstart.push_back((int)ctab.size());
                    ctab.insert(ctab.end(), c, c + c[0] + 1);
                }
                remap[(size_t)t][i] = it->second;
            }
        }
        auto fill = [&](int t) {
            const int r0 = (int)((long)M * t / nt);
            const Part &Q = parts[(size_t)t];
            for (size_t i = 0; i < Q.ids.size(); ++i) pat[(size_t)r0 + i] = (unsigned short)remap[(size_t)t][(size_t)Q.ids[i]];
        };
        if (nt == 1) fill(0);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < nt; ++t) th.emplace_back(fill, t);
            for (auto &x : th) x.join();
        }
    }
    if (npat == 0) return SGPU_OK;
    std::vector<int> tab, wgptr;
    std::vector<unsigned short> lpat;                          // wide: the rows' ids within their group's table
    const bool wide = (size_t)npat * (W + 1) > (size_t)SP_MAX_TABLE;
    size_t max_group = 0;
    if (!wide) {                                               // fixed width: W + 1 ints per pattern
        tab.assign((size_t)npat * (W + 1), 0);
        for (int i = 0; i < npat; ++i) {
            const int *c = &ctab[(size_t)cstart[(size_t)i]];
            for (int j = 0; j <= c[0]; ++j) tab[(size_t)i * (W + 1) + j] = c[j];
        }
        // (experiment, WRONG results: every gather reads the row's own column -- what the kernel costs without the spread of its gathers)
        if (std::getenv("SAENA_DEBUG_ZERO_OFFSETS")) for (int i = 0; i < npat; ++i) for (int j = 1; j <= W; ++j) tab[(size_t)i * (W + 1) + j] = 0;
    } else {                                                   // per group of SPW_BLOCK rows: [start of its k-th pattern in the group's table] [patterns] [one spare int]
        const int G = sk::SPW_BLOCK, ngrp = (M + G - 1) / G;
        wgptr.assign((size_t)ngrp + 1, 0);
        lpat.assign(pat.size(), 0);
        std::vector<int> local((size_t)npat, -1), used;
        for (int g = 0; g < ngrp; ++g) {
            used.clear();
            for (int r = g * G; r < std::min(M, (g + 1) * G); ++r) {
                const int id = pat[(size_t)r];
                if (local[(size_t)id] < 0) { local[(size_t)id] = (int)used.size(); used.push_back(id); }
                lpat[(size_t)r] = (unsigned short)local[(size_t)id];
            }
            size_t ints = used.size() + 1;
            for (int id : used) ints += 1 + (size_t)ctab[(size_t)cstart[(size_t)id]];
            if (ints > (size_t)sk::SPW_MAX_TABLE || tab.size() + ints > (size_t)INT32_MAX - 8) return SGPU_OK;
            max_group = std::max(max_group, ints);
            const size_t t0 = tab.size();
            tab.resize(t0 + ints, 0);
            size_t at = t0 + used.size();
            for (size_t k = 0; k < used.size(); ++k) {
                const int *c = &ctab[(size_t)cstart[(size_t)used[k]]];
                tab[t0 + k] = (int)(at - t0);
                for (int j = 0; j <= c[0]; ++j) tab[at++] = c[j];
                local[(size_t)used[k]] = -1;
            }
            wgptr[(size_t)g + 1] = (int)tab.size();
        }
    }
    if (std::getenv("SAENA_SETUP_TIMING")) {
        if (wide) fprintf(stderr, "[sgpu] row patterns: %d rows follow %d patterns of <= %d entries (%zu offsets in all); a table per %d rows, at most %zu ints, %.1f MB in all\n", M, npat, W,
                          ctab.size() - (size_t)npat, sk::SPW_BLOCK, max_group, (double)tab.size() * 4e-6);
        else fprintf(stderr, "[sgpu] row patterns%s: %d rows follow %d patterns of <= %d entries (%zu ints, fixed-width table)\n", rowbase ? " relative to the row's first column" : "", M, npat, W, tab.size());
    }
    if (rowbase) {
        std::vector<int> rb((size_t)((M + 127) / 128 * 128), 0);
        for (int r = 0; r < M; ++r) rb[(size_t)r] = ref(r);
        CHK(dev_upload(P.sp.sp_rbase, rb.data(), rb.size()));
    }
    CHK(dev_upload(P.sp.sp_pat, wide ? lpat.data() : pat.data(), pat.size()));
    CHK(dev_upload(P.sp.sp_tab, tab.data(), tab.size()));
    if (wide) CHK(dev_upload(P.sp.sp_wgptr, wgptr.data(), wgptr.size()));
    P.sp_w = wide ? (int)max_group : W; P.sp_n = npat; P.sp.sp_wide = wide;
    P.h_pstart = std::move(cstart); P.h_ptab = std::move(ctab); P.h_pat = std::move(pat);      // (for build_sellpx; dropped when the plan settles)
    P.sp_bytes = 8 * (int64_t)P.h_rp.back() + (rowbase ? 6 : 2) * (int64_t)M + 8 * (int64_t)P.ncols + 8 * (int64_t)M + (wide ? 4 * (int64_t)tab.size() : 0);
    P.sp.sp_ok = true;
    return SGPU_OK;
}

// k_sellpx on top of build_sellp's patterns: xwin_plan.h's plan_sellpx from the host copy of the patterns -- the windows of x per
// workgroup of SPX_ROWS rows, every workgroup's own small table of 16-bit LDS positions, its rows' ids within it.
int build_sellpx(CsrPart &P) {
    if (P.spx.spx_ok || P.spx.spx_tried || !P.sp.sp_ok || P.sp.sp_rbase || !P.sv.sl_val || P.h_ptab.empty() || P.h_pat.empty()) return SGPU_OK;
    P.spx.spx_tried = 1;
    const xwplan::SpxPlan X = xwplan::plan_sellpx(P.h_pstart, P.h_ptab, P.h_pat, P.nrows);
    if (X.refusal == xwplan::SPX_TABLE) P.h_pat.shrink_to_fit();
    if (X.refusal) return SGPU_OK;
    if (std::getenv("SAENA_SETUP_TIMING"))
        fprintf(stderr, "[sgpu] x in LDS for the row patterns: %d windows, %lld doubles of x + at most %lld table words per workgroup of %d rows (%.1f KiB); tables %.1f MB\n", X.nwin,
                (long long)X.S, (long long)X.max_words, sk::SPX_ROWS, (double)(X.S * 8 + X.max_words * 2) / 1024.0, (double)(X.tab.size() - 8) * 2e-6);
    CHK(dev_upload(P.spx.spx_tab, X.tab.data(), X.tab.size()));
    CHK(dev_upload(P.spx.spx_wgptr, X.wgptr.data(), X.wgptr.size()));
    CHK(dev_upload(P.spx.spx_pat, X.pat.data(), X.pat.size()));
    CHK(dev_upload(P.spx.spx_win, X.win.data(), X.win.size()));
    P.spx.spx_ok = true;
    return SGPU_OK;
}

// k_vidx on top of build_sellp's pattern ids (one table, not the per-workgroup tables of sp_wide): the values as 8-bit codes into a
// dictionary per workgroup of 256 rows, built on the device from the CSR values (k_vi_build).  Slices of 64 rows, each padded to its
// longest row rounded up to 8 positions.  The operator is refused where a workgroup holds more than VI_MAX distinct values.
int build_vidx(CsrPart &P) {
    if (P.vi.vi_ok || P.vi.vi_tried || !P.sp.sp_ok || P.sp.sp_wide || P.h_rp.empty() || !P.csr.val || !P.csr.row_ptr) return SGPU_OK;
    P.vi.vi_tried = 1;
    const int M = P.nrows;
    if (M == 0) return SGPU_OK;
    const int ns = (M + 63) / 64, ngrp = (ns + 3) / 4;
    const xwplan::SliceWidths sw = xwplan::slice_widths(P.h_rp.data(), M);      // (uw: the slices' common width, or 0: vi_cptr)
    if (!sw.ok) return SGPU_OK;
    const int64_t tot = sw.tot;
    const size_t nb = (size_t)tot + 512;
    if (P.vi.vi_code.alloc(nb) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of %zu bytes failed", nb);
    HIPCHK(hipMemsetAsync(P.vi.vi_code, 0, nb, g.cs));
    if (!sw.uw) CHK(dev_upload(P.vi.vi_cptr, sw.ptr.data(), sw.ptr.size()));
    DevArr<double> tmp;
    DevArr<int> d_cnt;
    CHK(dev_alloc(tmp, (size_t)ngrp * sk::VI_MAX));
    if (d_cnt.alloc((size_t)ngrp + 1) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc failed");
    int *d_flag = d_cnt + ngrp;
    HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(int), g.cs));
    SGPU_LAUNCH(sk::k_vi_build, dim3(ngrp), dim3(sk::BLOCK), 0, g.cs, (const double *)P.csr.val, (const int *)P.csr.row_ptr, (const int *)P.vi.vi_cptr,
                sw.uw, M, P.vi.vi_code.get(), tmp.get(), d_cnt.get(), d_flag);
    HIPCHK(hipGetLastError());
    std::vector<int> cnt((size_t)ngrp + 1);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    if (cnt[(size_t)ngrp]) {                                   // a workgroup holds more than VI_MAX distinct values: refused
        if (std::getenv("SAENA_SETUP_TIMING")) fprintf(stderr, "[sgpu] value-indexed form refused: a workgroup of 256 rows holds more than %d distinct values\n", sk::VI_MAX);
        P.vi.vi_code = {}; P.vi.vi_cptr = {};
        return SGPU_OK;
    }
    std::vector<int> dptr((size_t)ngrp + 1, 0);
    int dmax = 0;
    for (int b = 0; b < ngrp; ++b) { dptr[(size_t)b + 1] = dptr[(size_t)b] + cnt[(size_t)b]; dmax = std::max(dmax, cnt[(size_t)b]); }
    CHK(dev_upload(P.vi.vi_dptr, dptr.data(), dptr.size()));
    CHK(dev_upload(P.vi.vi_dict, (const double *)nullptr, 0, (size_t)dptr[(size_t)ngrp] + 1));      // (one element more: k_vidxw's lanes without a value read vdict[d0], and an empty last dictionary begins at the end)
    SGPU_LAUNCH(sk::k_vi_compact, dim3(ngrp), dim3(sk::BLOCK), 0, g.cs, (const double *)tmp, (const int *)P.vi.vi_dptr, P.vi.vi_dict.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.cs));
    P.vi_uw8 = sw.uw; P.vi_code_bytes = tot;
    P.vi_bytes = tot + (P.sp.sp_rbase ? 6 : 2) * (int64_t)M + 8 * (int64_t)P.ncols + 8 * (int64_t)M + 8 * (int64_t)dptr[(size_t)ngrp];
    P.vi.vi_ok = true;
    if (std::getenv("SAENA_SETUP_TIMING"))
        fprintf(stderr, "[sgpu] value-indexed row patterns: %d rows, %lld entries, %lld code bytes (%.2f per entry), at most %d distinct values per workgroup of 256 rows, %d in all dictionaries\n",
                M, (long long)P.nnz, (long long)tot, (double)tot / (double)std::max<int64_t>(1, P.nnz), dmax, dptr[(size_t)ngrp]);
    return SGPU_OK;
}

// The x-window launch mode of k_vidx for workgroups of R = 256 << k rows: xwin_plan.h's plan_vidxw from build_sellp's ONE pattern
// table and the dictionaries' starts (both read back from the device -- the host copies go when the plan settles).  Refused (ok stays
// false, *why says it): rowbase and per-workgroup tables, and what the plan refuses.
int build_xwin(CsrPart &P, int k, std::string *why = nullptr) {
    CsrPart::XWin &X = P.vw[k];
    const int R = 256 << k;
    auto no = [&](const char *m) { if (why) *why = m; return SGPU_OK; };
    if (X.ok) return SGPU_OK;
    if (!P.vi.vi_ok || !P.sp.sp_ok || !P.sp.sp_tab) return no("the value-indexed form was not built");
    if (P.sp.sp_rbase) return no("the patterns are relative to the rows' first columns (rowbase)");
    if (P.sp.sp_wide) return no("the patterns sit in per-workgroup tables");
    if (X.tried) return no("refused before");
    X.tried = 1;
    const int npat = P.sp_n, W = P.sp_w, M = P.nrows;
    if (npat <= 0 || W <= 0) return no("no patterns");
    std::vector<int> tab((size_t)npat * (W + 1)), dptr((size_t)((M + 63) / 64 + 3) / 4 + 1);
    HIPCHK(hipMemcpyAsync(tab.data(), P.sp.sp_tab, tab.size() * sizeof(int), hipMemcpyDeviceToHost, g.cs));
    HIPCHK(hipMemcpyAsync(dptr.data(), P.vi.vi_dptr, dptr.size() * sizeof(int), hipMemcpyDeviceToHost, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    // (the environment is read per operator, so that one process can build both paths)
    const char *fast_env = std::getenv("SAENA_VIDXW_FAST");
    const char *masks_env = std::getenv("SAENA_VIDXW_MASKS");
    const xwplan::VwPlan plan = xwplan::plan_vidxw(tab.data(), npat, W, M, P.ncols, R, P.vi_uw8, dptr.data(), fast_env && std::atoi(fast_env) == 0,
                                                   masks_env && std::atoi(masks_env) == 0);
    if (plan.refusal) return no(xwplan::refusal_text(plan.refusal));
    CHK(dev_upload(X.tab, plan.tab.data(), plan.tab.size(), 8));
    CHK(dev_upload(X.win, plan.win.data(), plan.win.size()));
    X.plan = plan.s;
    // the bit codes (vw_fast.h), where the dictionaries stay in scalar registers: packed on the device from k_vidx's codes, padding
    // included (build_vidx allocated 64 uw bytes per slice + CODE_PAD); a code above 1 -- none, by the dictionaries' lengths -- keeps the bytes
    const char *bits_env = std::getenv("SAENA_VIDXW_BITS");
    const bool bits_off = bits_env && std::atoi(bits_env) == 0;
    const int ns = (M + 63) / 64;
    const int64_t byte_codes = P.vi_code_bytes, bit_bytes = byte_codes / 8;
    const char *bits_why = plan.s.fast_kind == 0 ? "the general kernel is kept" : plan.s.fast_kind == 1 ? "the dictionaries are in LDS" : "SAENA_VIDXW_BITS=0";
    if (vwfast::bit_codes(plan.s.fast_kind, bits_off)) {
        const size_t nb = (size_t)vwfast::bit_total(ns, P.vi_uw8);
        DevArr<int> d_flag;
        if (X.bits.alloc(nb) != hipSuccess || d_flag.alloc(1) != hipSuccess) { X.bits = {}; return fail(SGPU_ERR_NOMEM, "hipMalloc of %zu bytes failed", nb); }
        HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(int), g.cs));
        SGPU_LAUNCH(sk::k_vi_pack_bits, dim3((unsigned)((nb + sk::BLOCK - 1) / sk::BLOCK)), dim3(sk::BLOCK), 0, g.cs, reinterpret_cast<const sk::sk_u2v *>(P.vi.vi_code.get()),
                    X.bits.get(), (unsigned)nb, d_flag.get());
        HIPCHK(hipGetLastError());
        int above1 = 0;
        HIPCHK(hipMemcpyAsync(&above1, d_flag, sizeof(int), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        if (above1) { X.bits = {}; bits_why = "a code above 1"; }
    }
    // the rows as lane masks (vw_masks.h), where the rule takes the table and the codes are bits: packed on the device from the pattern
    // ids, the table just uploaded, the pattern -> slot table and k_vidx's codes; a code above 1 or a position without a slot -- none,
    // by the rule -- keeps the table rows
    const char *masks_why = !X.bits && plan.s.mask_clause == vwmasks::TAKEN ? "the codes are 8 bits per entry" : vwmasks::clause_text(plan.s.mask_clause);
    const size_t mask_bytes = (size_t)vwmasks::total_words(ns) * sizeof(unsigned long long);
    if (plan.s.mask_clause == vwmasks::TAKEN && X.bits) {
        DevArr<unsigned char> d_pslot;
        DevArr<int> d_flag;
        CHK(dev_upload(d_pslot, plan.pslot.data(), plan.pslot.size()));
        if (X.masks.alloc((size_t)vwmasks::total_words(ns)) != hipSuccess || d_flag.alloc(1) != hipSuccess) { X.masks = {}; return fail(SGPU_ERR_NOMEM, "hipMalloc of %zu bytes failed", mask_bytes); }
        HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(int), g.cs));
        SGPU_LAUNCH(sk::k_vi_pack_masks, dim3((unsigned)((ns + sk::BLOCK / 64 - 1) / (sk::BLOCK / 64))), dim3(sk::BLOCK), 0, g.cs, (const unsigned short *)P.sp.sp_pat, (const unsigned short *)X.tab.get(),
                    (const unsigned char *)d_pslot.get(), reinterpret_cast<const sk::sk_u2v *>(P.vi.vi_code.get()), P.vi_uw8, M, ns, X.masks.get(), d_flag.get());
        HIPCHK(hipGetLastError());
        int flag = 0;
        HIPCHK(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        if (flag) { X.masks = {}; masks_why = flag & vwmasks::CODE_ABOVE_1 ? "a code above 1" : "a position without a slot"; }
    }
    X.ok = true;
    if (std::getenv("SAENA_SETUP_TIMING")) {
        const xwplan::VwScalars &s = X.plan;
        fprintf(stderr, "[sgpu] x windows for the value-indexed form: workgroups of %d rows, %d windows, %lld doubles of x + %d dictionaries + %lld table words = %.1f KiB of LDS (%.1f B of x per row); staged %s (%d trips)\n",
                R, s.head.nwin, (long long)s.head.S, R / sk::BLOCK, (long long)s.head.tn, (double)s.lds / 1024.0, 8.0 * (double)s.head.S / R, s.head.ntrip ? "window by window" : "flat", s.head.ntrip);
        if (s.fast_kind)
            fprintf(stderr, "[sgpu] x windows at %d rows: the common-path kernel is taken, dictionaries of %d values in %s, %d bytes of LDS\n", R, s.head.vd_u,
                    s.fast_kind == 2 ? "scalar registers" : "LDS", s.fast_lds);
        else
            fprintf(stderr, "[sgpu] x windows at %d rows: the general kernel is kept (%s)\n", R, vwfast::clause_text(s.fast_clause));
        if (X.bits)
            fprintf(stderr, "[sgpu] x windows at %d rows: codes of 1 bit per entry, %lld bytes packed from %lld bytes of 8-bit codes\n", R, (long long)bit_bytes, (long long)byte_codes);
        else
            fprintf(stderr, "[sgpu] x windows at %d rows: codes of 8 bits per entry (%s), %lld bytes, 1-bit codes would take %lld\n", R, bits_why, (long long)byte_codes, (long long)bit_bytes);
        if (X.masks)
            fprintf(stderr, "[sgpu] x windows at %d rows: rows as lane masks, %zu bytes in %d records of %d slots\n", R, mask_bytes, ns, s.head.lmax);
        else
            fprintf(stderr, "[sgpu] x windows at %d rows: rows through the table (%s)\n", R, masks_why);
    }
    return SGPU_OK;
}

// The row-paired values of k_sellp2 on top of build_sellp's pattern ids: slices of 128 rows, a slice padded to its longest
// row, position-major with the values of rows 2 l and 2 l + 1 side by side.
int build_sellp2(CsrPart &P, const std::vector<double> &h_val_all) {
    if (P.sp2.sp2_ok || P.sp2.sp2_tried || !P.sp.sp_ok || P.sp.sp_rbase || P.h_rp.empty()) return SGPU_OK;      // (rows r and r + 1 of a rowbase operator do not read adjacent columns)
    P.sp2.sp2_tried = 1;
    const int M = P.nrows;
    if (M < 2 || P.ncols < 2 || !P.csr.val || !P.csr.row_ptr) return SGPU_OK;      // (the kernel reads x 16 bytes at a time)
    const int ns = (M + 127) / 128;
    std::vector<int> ptr((size_t)ns + 1, 0);
    int64_t tot = 0;
    for (int s = 0; s < ns; ++s) {
        int w = 0;
        for (int r = s * 128; r < std::min(M, s * 128 + 128); ++r) w = std::max(w, P.h_rp[(size_t)r + 1] - P.h_rp[(size_t)r]);
        tot += (int64_t)w * 128;
        if (tot > (int64_t)INT32_MAX - 1024) return SGPU_OK;
        ptr[(size_t)s + 1] = (int)tot;
    }
    if ((double)tot > 1.12 * (double)P.nnz) return SGPU_OK;
    P.sp2_uw = uniform_width(ptr, 128, &tot);
    CHK(dev_upload(P.sp2.sp2_ptr, ptr.data(), ptr.size()));
    const size_t nv = (size_t)tot + 128;
    if (P.sp2.sp2_val.alloc(nv) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of %zu bytes failed", nv * sizeof(double));
    HIPCHK(hipMemsetAsync(P.sp2.sp2_val, 0, nv * sizeof(double), g.cs));
    SGPU_LAUNCH(sk::k_sell_scatter<double>, dim3((M + sk::BLOCK - 1) / sk::BLOCK), dim3(sk::BLOCK), 0, g.cs, (const double *)P.csr.val, (const int *)P.csr.row_ptr,
                (const int *)P.sp2.sp2_ptr, P.sp2.sp2_val, M, 2);            // (round 4: from the CSR values on the device, like build_sell_values)
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.cs));
    P.sp2_nslices = ns;
    P.sp2.sp2_ok = true;
    return SGPU_OK;
}

// Row templates (k_rowt): every row as (length, columns relative to the row, values); the operator qualifies when its rows
// follow at most 65 535 templates whose tables fit 32 KiB of LDS.  Ids in order of first appearance.
constexpr int RT_MAX_BYTES = 32768;
int build_rowt(CsrPart &P, const std::vector<double> &h_val_all) {
    if (P.rt.rt_ok || P.rt.rt_tried || P.h_rp.empty()) return SGPU_OK;
    P.rt.rt_tried = 1;
    const int M = P.nrows;
    if (M == 0 || h_val_all.size() != P.h_col.size()) return SGPU_OK;
    int W = 1;
    for (int r = 0; r < M; ++r) W = std::max(W, P.h_rp[(size_t)r + 1] - P.h_rp[(size_t)r]);
    const int per = (W + 1) * 4 + W * 8;
    if (per > RT_MAX_BYTES) return SGPU_OK;
    const int max_pat = std::min(65535, RT_MAX_BYTES / per);
    std::vector<int> itab;
    std::vector<double> vtab;
    std::vector<unsigned short> pat((size_t)M, 0);
    std::unordered_map<std::string, int> ids;
    std::string key;
    int prev = -1, npat = 0;
    for (int r = 0; r < M; ++r) {
        const int p0 = P.h_rp[(size_t)r], n = P.h_rp[(size_t)r + 1] - p0;
        if (prev >= 0 && itab[(size_t)prev * (W + 1)] == n) {          // most rows repeat the row before
            const int *t = &itab[(size_t)prev * (W + 1) + 1];
            const double *v = &vtab[(size_t)prev * W];
            int j = 0;
            while (j < n && P.h_col[(size_t)p0 + j] - r == t[j] && std::memcmp(&h_val_all[(size_t)p0 + j], &v[j], 8) == 0) ++j;
            if (j == n) { pat[(size_t)r] = (unsigned short)prev; continue; }
        }
        key.assign(reinterpret_cast<const char *>(&n), sizeof n);
        for (int j = 0; j < n; ++j) { const int o = P.h_col[(size_t)p0 + j] - r; key.append(reinterpret_cast<const char *>(&o), sizeof o); }
        key.append(reinterpret_cast<const char *>(&h_val_all[(size_t)p0]), (size_t)n * 8);
        auto f = ids.find(key);
        if (f == ids.end()) {
            if (npat == max_pat) return SGPU_OK;                       // too many distinct rows: not this kind of operator
            f = ids.emplace(key, npat++).first;
            itab.push_back(n);
            for (int j = 0; j < W; ++j) itab.push_back(j < n ? P.h_col[(size_t)p0 + j] - r : 0);
            for (int j = 0; j < W; ++j) vtab.push_back(j < n ? h_val_all[(size_t)p0 + j] : 0.0);
        }
        prev = f->second;
        pat[(size_t)r] = (unsigned short)prev;
    }
    if (npat == 0) return SGPU_OK;
    if (std::getenv("SAENA_SETUP_TIMING")) fprintf(stderr, "[sgpu] row templates: %d rows follow %d templates of <= %d entries\n", M, npat, W);
    CHK(dev_upload(P.rt.rt_pat, pat.data(), pat.size()));
    CHK(dev_upload(P.rt.rt_itab, itab.data(), itab.size()));
    CHK(dev_upload(P.rt.rt_vtab, vtab.data(), vtab.size()));
    P.rt_w = W; P.rt_n = npat;
    P.rt.rt_ok = true;
    return SGPU_OK;
}

// Sliced ELLPACK inside the (row chunk, column window) blocks of the x-in-LDS plan (k_sellx): per block the rows with a piece
// in that window (every row in the chunk's last window), sorted by piece length, 64 to a slice, position-major in pairs.
// Built where it can pay: at most 25 % padding, chunks of at most 65 534 rows.
int build_sellx(CsrPart &P, const std::vector<double> &h_val_all) {
    if (P.sx.sx_ok || P.sx.sx_tried || !P.xlp.xl_ok || P.xl_blk_h.empty()) return SGPU_OK;
    P.sx.sx_tried = 1;
    if (h_val_all.size() != P.h_col.size()) return SGPU_OK;
    const int nb = P.xl_nblk;
    const std::vector<int> &blk = P.xl_blk_h;
    for (int b = 0; b < nb; ++b) if (blk[(size_t)b + 1] - blk[(size_t)b] > 65534) return SGPU_OK;
    struct Piece { int k, p0, len; };
    // pass 1: per block the sorted piece list and its slices' widths
    std::vector<std::vector<std::vector<Piece>>> pieces((size_t)nb);       // [chunk][window] -> pieces sorted by length
    std::vector<int> bptr((size_t)nb * (sk::XL_MAXT + 1) + 1, 0);
    std::vector<int64_t> chunk_entries((size_t)nb, 0), chunk_slices((size_t)nb, 0);
    const int nt = std::min(host_threads(), std::max(1, nb / 8));
    auto pass1 = [&](int t) {
        for (int b = (int)((long)nb * t / nt); b < (int)((long)nb * (t + 1) / nt); ++b) {
            const int r0 = blk[(size_t)b], rows = blk[(size_t)b + 1] - r0, cmin = P.xl_info_h[(size_t)b].x, T = P.xl_info_h[(size_t)b].y;
            auto &pw = pieces[(size_t)b];
            pw.assign((size_t)T, {});
            for (int k = 0; k < rows; ++k) {
                const int p0 = P.h_rp[(size_t)r0 + k], p1 = P.h_rp[(size_t)r0 + k + 1];
                int p = p0;
                for (int w = 0; w < T; ++w) {
                    const int lim = w == T - 1 ? INT32_MAX : cmin + (w + 1) * P.xl_win;
                    const int q0 = p;
                    while (p < p1 && P.h_col[(size_t)p] < lim) ++p;
                    if (p > q0 || w == T - 1) pw[(size_t)w].push_back(Piece{k, q0, p - q0});
                }
            }
            int64_t ent = 0, sl = 0;
            for (int w = 0; w < T; ++w) {
                auto &v = pw[(size_t)w];
                std::stable_sort(v.begin(), v.end(), [](const Piece &x, const Piece &y) { return x.len > y.len; });
                for (size_t i = 0; i < v.size(); i += 64) { ent += (int64_t)((v[i].len + 1) & ~1) * 64; ++sl; }
            }
            chunk_entries[(size_t)b] = ent; chunk_slices[(size_t)b] = sl;
        }
    };
    {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(pass1, t);
        for (auto &x : th) x.join();
    }
    int64_t tot = 0, nsl = 0;
    std::vector<int64_t> e0((size_t)nb), s0((size_t)nb);
    for (int b = 0; b < nb; ++b) { e0[(size_t)b] = tot; s0[(size_t)b] = nsl; tot += chunk_entries[(size_t)b]; nsl += chunk_slices[(size_t)b]; }
    if (tot > (int64_t)INT32_MAX - 1024 || nsl > INT32_MAX / 64) return SGPU_OK;
    P.sx_pad = (double)tot / (double)std::max<int64_t>(1, P.nnz);
    const double pad_limit = std::getenv("SAENA_SELLX_PAD") ? atof(std::getenv("SAENA_SELLX_PAD")) : 1.25;
    if (P.sx_pad > pad_limit) return SGPU_OK;
    std::vector<double> val((size_t)tot + 128, 0.0);
    std::vector<unsigned short> col((size_t)tot + 128, 0);
    std::vector<unsigned> meta((size_t)nsl * 64, 0xffffu);
    std::vector<int> sptr((size_t)nsl + 1, 0);
    auto pass2 = [&](int t) {
        for (int b = (int)((long)nb * t / nt); b < (int)((long)nb * (t + 1) / nt); ++b) {
            const int cmin = P.xl_info_h[(size_t)b].x, T = P.xl_info_h[(size_t)b].y;
            std::vector<char> seen((size_t)(blk[(size_t)b + 1] - blk[(size_t)b]), 0);
            int64_t e = e0[(size_t)b], sl = s0[(size_t)b];
            for (int w = 0; w <= sk::XL_MAXT; ++w) {
                bptr[(size_t)b * (sk::XL_MAXT + 1) + (size_t)w] = (int)sl;
                if (w >= T) continue;
                const auto &v = pieces[(size_t)b][(size_t)w];
                const int wbase = cmin + w * P.xl_win;
                for (size_t i = 0; i < v.size(); i += 64, ++sl) {
                    const int width = (v[i].len + 1) & ~1, PP = width >> 1;
                    sptr[(size_t)sl] = (int)e;
                    for (size_t j = i; j < std::min(v.size(), i + 64); ++j) {
                        const Piece &pc = v[j];
                        const int lane = (int)(j - i);
                        const unsigned first = seen[(size_t)pc.k] ? 0u : 1u;
                        seen[(size_t)pc.k] = 1;
                        meta[(size_t)sl * 64 + (size_t)lane] = (unsigned)pc.k | ((unsigned)pc.len << 16) | (first << 31);
                        for (int q = 0; q < pc.len; ++q) {
                            const size_t o = (size_t)e + (size_t)(q >> 1) * 128 + (size_t)lane * 2 + (size_t)(q & 1);
                            val[o] = h_val_all[(size_t)pc.p0 + q];
                            col[o] = (unsigned short)(P.h_col[(size_t)pc.p0 + q] - wbase);
                        }
                    }
                    (void)PP;
                    e += (int64_t)width * 64;
                }
            }
        }
    };
    {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(pass2, t);
        for (auto &x : th) x.join();
    }
    sptr[(size_t)nsl] = (int)tot;
    bptr[(size_t)nb * (sk::XL_MAXT + 1)] = (int)nsl;
    if (std::getenv("SAENA_SETUP_TIMING"))
        fprintf(stderr, "[sgpu] sliced ELLPACK in LDS windows: %d rows, %lld entries, %.1f %% padding, %lld slices in %d chunks of <= %d windows\n", P.nrows,
                (long long)P.nnz, 100.0 * (P.sx_pad - 1.0), (long long)nsl, nb, P.xl_maxt);
    CHK(dev_upload(P.sx.sx_val, val.data(), val.size()));
    CHK(dev_upload(P.sx.sx_col, col.data(), col.size()));
    CHK(dev_upload(P.sx.sx_meta, meta.data(), meta.size(), 64));
    CHK(dev_upload(P.sx.sx_sptr, sptr.data(), sptr.size()));
    CHK(dev_upload(P.sx.sx_bptr, bptr.data(), bptr.size()));
    if (!P.xlp.xl_acc && P.xl_maxt > 1 && !P.xl_acc_lds) HIPCHK(P.xlp.xl_acc.alloc((size_t)P.nrows));
    P.sx.sx_ok = true;
    return SGPU_OK;
}

} // namespace

struct sgpu_op {
    index_t M = 0, N_local = 0;
    CsrPart loc, rem;
    bool    has_remote = false;
    DevArr<double> inv_diag;
    DevArr<double> tmp;           // smoother ping-pong buffer [M]
    DevArr<double> ones;          // [M] of 1.0 (sgpu_residual_negative: rhs - A u as 1 * 1 * (rhs - A u)), made at its first call
    DevArr<double> dvec;          // chebyshev d [M]
    // block entry points (sgpu_*_block): lanes per row of k_csr_block (0: from the mean row length at the first block apply),
    // and the block ping-pong buffer / Chebyshev d of [M * K] per K = 2, 4, 8, made at the first block smoother call with that K
    // (never re-allocated: captured block V-cycles hold the pointers)
    int     block_lanes = 0, block_lanes_auto = 0;
    DevArr<double> tmp_blk[3], dvec_blk[3];
    // the block halo of an operator with a halo plan, per K = 2, 4, 8: send / receive buffers of vIndexSize * K / recvSize * K doubles
    // (and the float pair of an fp32 wire), made at the first block apply with that K; injected_blk: sgpu_debug_inject_halo_block
    DevArr<double> send_blk[3], recv_blk[3];
    DevArr<float>  send_blk_f[3], recv_blk_f[3];
    bool    blk_halo_made[3] = {false, false, false}, injected_blk[3] = {false, false, false};
    // halo plan
    int     vIndexSize = 0, recvSize = 0;
    DevArr<int>    vIndex;
    DevArr<double> send_buf, recv_buf;
    DevArr<float>  send_f, recv_f;                    // fp32 wire buffers (halo_fp32 && nranks > 1)
    std::vector<int> sendRank, sendCount, sendDispl, recvRank, recvCount, recvDispl;
    int     halo_fp32 = 0;
    bool    injected = false;     // test hook: halo supplied by sgpu_debug_inject_halo
    bool    local_only_ok = false; // test hook: sgpu_debug_allow_local_only
    bool    single_stream = false; // exchange and rows on the compute stream, in order (short local kernels): apply() mode S
    bool    events_only = false;   // long interior kernel: the two streams are ordered by plain events (apply() mode E)
    std::string vname;            // sgpu_op_get_variant's kernel name (owns the string it returns)
    DevArr<double> dense_rem;     // variant 5 with a halo: row-major M x recvSize over the receive buffer
    std::vector<int> rem_rows_h;  // host copy of rem.csr.rows (compact boundary row -> local row)
    std::vector<double> h_val;   // host copy of the values of small local parts (coarsest-level factorisation)
    std::vector<double> h_val_all;   // host copy of all local values (kept while the column-major form may still be built)
    DevArr<unsigned> skip;        // bitmask over the M rows: set = boundary row (has remote entries), written by k_csr_boundary
    int     bnd_lanes = 1;        // lanes per boundary row
    hipEvent_t ev_x = nullptr, ev_halo = nullptr;   // cs -> hs: inputs ready; hs -> cs: exchange + boundary rows done
    ~sgpu_op() {                  // also runs when sgpu_op_create bails out half-way; the arrays free themselves
        if (ev_x) hipEventDestroy(ev_x);
        if (ev_halo) hipEventDestroy(ev_halo);
    }
};

namespace {

int build_dense_rem(sgpu_op *op) {
    if (op->dense_rem || !op->has_remote) return SGPU_OK;
    if (op->rem.h_val.empty()) return fail(SGPU_ERR_ARG, "this operator is too large for the dense form");
    const size_t nh = (size_t)op->recvSize;
    std::vector<double> d((size_t)op->M * nh, 0.0);
    // rem: CSR over the boundary rows (h_rows maps compact -> local row), columns = receive-buffer positions
    for (int i = 0; i < op->rem.nrows; ++i)
        for (int k = op->rem.h_rp[i]; k < op->rem.h_rp[i + 1]; ++k) d[(size_t)op->rem_rows_h[(size_t)i] * nh + op->rem.h_col[k]] = op->rem.h_val[k];
    CHK(dev_upload(op->dense_rem, d.data(), d.size()));
    return SGPU_OK;
}

struct EpiArgs {
    const double *rhs = nullptr, *inv_diag = nullptr, *u = nullptr;
    double       *d = nullptr, *y2 = nullptr;
    double        c0 = 0.0, c1 = 0.0;
};

// ---- kernel pickers: from the runtime's (epilogue, lanes, halo, ...) to a __global__ instantiation, through dispatch.h ----
// A family names its kernel and its parameter lists once.  An epilogue outside a family's list yields NO kernel (nullptr) and the
// launch fails with SGPU_ERR_STATE (SGPU_LAUNCH_PICKED): a missing kernel is an error, never a fall-back to another one.
using dispatch::among;
using dispatch::with_bool;
using KernelFn = void (*)(const sk::SpmvArgs);
using VecKernelFn = void (*)(const sk::SpmvArgs, int);
using VidxwKernelFn = void (*)(const sk::SpmvArgs, const sk::VwHead, int);      // k_vidxw: the head of its tables by value
using VidxwFastKernelFn = void (*)(const vwfast::VwFast);                        // k_vidxw_fast: its one argument
using SellKernelFn = void (*)(const sk::SpmvArgs, int);     // seq != 0: the launch carries the fork (block 0 stores flag_x = seq when it starts)
using XldsKernelFn = void (*)(const sk::SpmvArgs, const sk::XldsArgs);
using SellxKernelFn = void (*)(const sk::SpmvArgs, const sk::SellxArgs);
using DenseKernelFn = void (*)(const sk::SpmvArgs, const double *, int, int);
using DenseHaloKernelFn = void (*)(const sk::SpmvArgs, const double *, const double *, int, int, int, const double *, const float *, int);
using BndKernelFn = void (*)(const sk::BoundaryArgs);

template <class F>
auto per_epi(int epi, F &&f) { return among<sk::EPI_SPMV, sk::EPI_RESIDUAL, sk::EPI_JACOBI, sk::EPI_CHEBY0, sk::EPI_CHEBYK, sk::EPI_SUB, sk::EPI_RSWEEP>(epi, f); }
// k_dense_rows_halo, k_csr_boundary, k_csr_block: no EPI_RSWEEP (vcycle_level fuses the restriction's sweep on one rank only, on a scalar operator without a remote part)
template <class F>
auto per_epi_no_rsweep(int epi, F &&f) { return among<sk::EPI_SPMV, sk::EPI_RESIDUAL, sk::EPI_JACOBI, sk::EPI_CHEBY0, sk::EPI_CHEBYK, sk::EPI_SUB>(epi, f); }

// lanes per row -> an instantiated group size.  The tile, vector and boundary kernels: the powers of two up to a wave, anything else 64
int lanes_or_64(int lanes) { return lanes == 1 || lanes == 2 || lanes == 4 || lanes == 8 || lanes == 16 || lanes == 32 ? lanes : 64; }
template <class F>
auto per_lanes(int lanes, F &&f) { return among<1, 2, 4, 8, 16, 32, 64>(lanes_or_64(lanes), f); }
// the x-in-LDS kernels: the smallest power of two in lo .. hi that holds the lanes, else hi
int lanes_up(int lanes, int lo, int hi) { int G = lo; while (G < lanes && G < hi) G *= 2; return G; }

// tile family F: 0 k_csr_stream, 1 k_csr_cc16, 2 k_csr_cm; tiles of CAP / CAP_BIG products; H: interior half of a multi-rank apply (kernels.hip.h)
template <int F>
KernelFn pick_tile(int epi, int lanes, bool big, bool halo) {
    return per_epi(epi, [&](auto E) { return among<sk::CAP, sk::CAP_BIG>(big ? sk::CAP_BIG : sk::CAP, [&](auto C) { return per_lanes(lanes, [&](auto G) { return with_bool(halo, [&](auto H) -> KernelFn {
        if constexpr (F == 0) return sk::k_csr_stream<E(), G(), C(), H()>;
        else if constexpr (F == 2) return sk::k_csr_cm<E(), G(), C(), H()>;
        else return sk::k_csr_cc16<E(), G(), C(), H()>; }); }); }); });
}
VecKernelFn pick_vec(int epi, int lanes, bool halo) {
    return per_epi(epi, [&](auto E) { return per_lanes(lanes, [&](auto G) { return with_bool(halo, [&](auto H) -> VecKernelFn { return sk::k_csr_vector<E(), G(), H()>; }); }); });
}
VecKernelFn pick_wave(int epi, int lanes, bool halo) {                       // groups of 8 lanes at least
    return per_epi(epi, [&](auto E) { return among<8, 16, 32, 64>(std::max(8, lanes_or_64(lanes)), [&](auto G) { return with_bool(halo, [&](auto H) -> VecKernelFn { return sk::k_csr_wave<E(), G(), H()>; }); }); });
}
SellKernelFn pick_sell(int epi, bool halo, bool pair, bool nt) {
    return per_epi(epi, [&](auto E) { return with_bool(halo, [&](auto H) { return with_bool(pair, [&](auto P) { return with_bool(nt, [&](auto N) -> SellKernelFn { return sk::k_sell<E(), H(), P(), N()>; }); }); }); });
}
SellKernelFn pick_sellp(int epi, bool halo, bool pair, bool nt, bool wide) {
    return per_epi(epi, [&](auto E) { return with_bool(halo, [&](auto H) { return with_bool(pair, [&](auto P) { return with_bool(nt, [&](auto N) { return with_bool(wide, [&](auto W) -> SellKernelFn {
        return sk::k_sellp<E(), H(), P(), N(), W()>; }); }); }); }); });
}
// PRE exists for the residual and the Jacobi sweep only, and only without a halo
template <bool WIDE>
SellKernelFn pick_sellp2(int epi, bool halo, bool nt, bool pre = false) {
    return per_epi(epi, [&](auto E) { return with_bool(halo, [&](auto H) { return with_bool(nt, [&](auto N) { return with_bool(pre, [&](auto R) -> SellKernelFn {
        return sk::k_sellp2<E(), H(), N(), WIDE, R() && !H() && (E() == sk::EPI_RESIDUAL || E() == sk::EPI_JACOBI)>; }); }); }); });
}
SellKernelFn pick_sellpx(int epi, bool halo, bool pair, bool nt) {
    return per_epi(epi, [&](auto E) { return with_bool(halo, [&](auto H) { return with_bool(pair, [&](auto P) { return with_bool(nt, [&](auto N) -> SellKernelFn { return sk::k_sellpx<E(), H(), P(), N()>; }); }); }); });
}
SellKernelFn pick_vidx(int epi, bool halo, bool nt) {
    return per_epi(epi, [&](auto E) { return with_bool(halo, [&](auto H) { return with_bool(nt, [&](auto N) -> SellKernelFn { return sk::k_vidx<E(), H(), N()>; }); }); });
}
VidxwKernelFn pick_vidxw(int epi, bool halo, bool nt) {
    return per_epi(epi, [&](auto E) { return with_bool(halo, [&](auto H) { return with_bool(nt, [&](auto N) -> VidxwKernelFn { return sk::k_vidxw<E(), H(), N()>; }); }); });
}
// the common path (vw_fast.h): 256 / 512 rows, the three epilogues with operands fetched up front, dictionaries in LDS / in scalar registers
// bits (with sd alone): the codes at one bit per entry; masks (with bits alone): the rows as lane masks (vw_masks.h)
VidxwFastKernelFn pick_vidxw_fast(int rows, int epi, bool nt, bool sd, bool bits, bool masks) {
    if ((bits && !sd) || (masks && !bits)) return nullptr;
    return among<256, 512>(rows, [&](auto R) { return among<sk::EPI_SPMV, sk::EPI_RESIDUAL, sk::EPI_JACOBI>(epi, [&](auto E) { return with_bool(nt, [&](auto N) { return with_bool(sd, [&](auto S) {
        return with_bool(bits, [&](auto B) { return with_bool(masks, [&](auto K) -> VidxwFastKernelFn { return sk::k_vidxw_fast<R(), E(), N(), S(), S() && B(), S() && B() && K()>; }); }); }); }); }); });
}
SellKernelFn pick_rowt(int epi, bool halo, bool nt) {
    return per_epi(epi, [&](auto E) { return with_bool(halo, [&](auto H) { return with_bool(nt, [&](auto N) -> SellKernelFn { return sk::k_rowt<E(), H(), N()>; }); }); });
}
SellxKernelFn pick_sellx(int epi, bool halo) {
    return per_epi(epi, [&](auto E) { return with_bool(halo, [&](auto H) -> SellxKernelFn { return sk::k_sellx<E(), H()>; }); });
}
XldsKernelFn pick_xlds(int epi, int lanes, bool halo) {
    return per_epi(epi, [&](auto E) { return among<4, 8, 16, 32, 64>(lanes_up(lanes, 4, 64), [&](auto G) { return with_bool(halo, [&](auto H) -> XldsKernelFn { return sk::k_csr_xlds<E(), G(), H()>; }); }); });
}
// k_csr_xldsr: four rows per group step (short rows), 4 / 8 / 16 / 32 lanes per group
// (eight rows per step were tried: 128 registers per lane do not hold them -- 136 bytes of scratch per lane, 110 against 94.5 us)
XldsKernelFn pick_xldsr(int epi, int lanes, bool halo) {
    return per_epi(epi, [&](auto E) { return among<4, 8, 16, 32>(lanes_up(lanes, 4, 32), [&](auto G) { return with_bool(halo, [&](auto H) -> XldsKernelFn { return sk::k_csr_xlds<E(), G(), H(), 4>; }); }); });
}
DenseKernelFn pick_dense(int epi) {
    return per_epi(epi, [&](auto E) -> DenseKernelFn { return sk::k_dense_rows<E()>; });
}
DenseHaloKernelFn pick_dense_halo(int epi) {
    return per_epi_no_rsweep(epi, [&](auto E) -> DenseHaloKernelFn { return sk::k_dense_rows_halo<E()>; });
}
BndKernelFn pick_bnd(int epi, int lanes) {
    return per_epi_no_rsweep(epi, [&](auto E) { return per_lanes(lanes, [&](auto G) -> BndKernelFn { return sk::k_csr_boundary<E(), G()>; }); });
}
// launch what a picker returned for the caller's `epi`, or fail
#define SGPU_LAUNCH_PICKED(family, k, ...)                                                                            \
    do {                                                                                                             \
        const auto k_ = (k);                                                                                         \
        if (!k_) return fail(SGPU_ERR_STATE, "no %s kernel for epilogue %d", family, epi);                           \
        SGPU_LAUNCH(k_, __VA_ARGS__);                                                                                \
    } while (0)
// the same for the kernels templated on a column count (the block, eig, lock and Gram-Schmidt layers): `k` is what among<...>(cols, ...)
// returned
#define SGPU_LAUNCH_COLS(family, cols, k, ...)                                                                        \
    do {                                                                                                             \
        const auto k_ = (k);                                                                                         \
        if (!k_) return fail(SGPU_ERR_STATE, "no %s kernel for %d columns", family, (int)(cols));                    \
        SGPU_LAUNCH(k_, __VA_ARGS__);                                                                                \
    } while (0)
// K of a block vector into an instantiation: per_K(K, [](auto k) { return sk::kernel<k()>; }); null for a K that is not 2, 4 or 8
template <class F>
auto per_K(int K, F &&f) { return among<2, 4, 8>(K, f); }

// measurement: `reps` back-to-back runs of once() between the context's two events, *ms = the time of one run.  The events are made
// at the first use and destroyed with the context: not part of what a caller's wall clock around the call sees.  A warm-up run,
// where a caller wants one, is the caller's
template <class Once>
int time_reps(int reps, float *ms, Once &&once) {
    if (!g.tk0) { HIPCHK(hipEventCreate(&g.tk0)); HIPCHK(hipEventCreate(&g.tk1)); }
    HIPCHK(hipEventRecord(g.tk0, g.cs));
    for (int i = 0; i < reps; ++i) CHK(once());
    HIPCHK(hipEventRecord(g.tk1, g.cs));
    HIPCHK(hipEventSynchronize(g.tk1));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, g.tk0, g.tk1));
    *ms = t / reps;
    return SGPU_OK;
}

// what every SpMV launch shares: the vectors and the epilogue's operands; a form then sets its own fields, all others stay zero
sk::SpmvArgs spmv_args(const double *x, double *y, const EpiArgs &e) {
    sk::SpmvArgs a{};
    a.x = x; a.y = y; a.rhs = e.rhs; a.inv_diag = e.inv_diag; a.u = e.u; a.d = e.d; a.y2 = e.y2; a.c0 = e.c0; a.c1 = e.c1; a.cc_ob = 12;
    return a;
}

// The row-pattern forms (variants 11, 14, 15, 17): non-temporal streams once the stored operator (values, pattern ids, x, y) is beyond
// the 256 MiB Infinity Cache, or as SAENA_SELLP_NT says; the first resident_slices slices keep their plain loads (SpmvArgs::nt_from)
bool row_pattern_nt(sk::SpmvArgs &a, int64_t stored_bytes, int nslices, double bytes_per_slice) {
    static const int nt_env = std::getenv("SAENA_SELLP_NT") ? std::atoi(std::getenv("SAENA_SELLP_NT")) : -1;
    const bool nt = nt_env >= 0 ? nt_env != 0 : stored_bytes > (int64_t)256 * 1024 * 1024;
    a.nt_from = nt ? resident_slices(nslices, bytes_per_slice) : 0;
    return nt;
}

int launch_part(const CsrPart &P, int epi, const double *x, double *y, const EpiArgs &e, const unsigned *skip = nullptr, uint64_t seq = 0) {
    if (P.nblk == 0) return SGPU_OK;
    sk::SpmvArgs a = spmv_args(x, y, e);
    a.flag_x = seq ? g.kflag_x : nullptr; a.seq = seq;
    a.row_ptr = P.csr.row_ptr; a.col = P.csr.col; a.val = P.csr.val;
    a.skip = skip; a.ncols = P.ncols;
    static const int st_plain_env = std::getenv("SAENA_STORE_PLAIN") ? std::atoi(std::getenv("SAENA_STORE_PLAIN")) : 0;
    a.st_plain = st_plain_env;
    static const int nt_rt = std::getenv("SAENA_STREAM_NT") ? std::atoi(std::getenv("SAENA_STREAM_NT")) : 0;
    a.nt = nt_rt == 1 || (nt_rt == 2 && 12 * P.nnz > (int64_t)256 * 1024 * 1024) ? 1 : 0;
    const bool halo = skip != nullptr || seq != 0;
    switch (P.variant) {
    default: {                                                    // F_STREAM16, F_STREAM32: 32-bit columns, 16 / 32 KiB tiles
        const bool big = P.variant == F_STREAM32;
        a.blk_row = big ? P.csr.blk_row_big : P.csr.blk_row;
        a.nblk = big ? P.nblk_big : P.nblk;
        SGPU_LAUNCH_PICKED("k_csr_stream", pick_tile<0>(epi, P.lanes, big, halo), dim3(a.nblk), dim3(sk::BLOCK), 0, g.cs, a);
    } break;
    case F_VECTOR: {                                              // vector CSR
        const int rpb = sk::BLOCK / P.lanes;
        a.blk_row = nullptr; a.nblk = 0;
        SGPU_LAUNCH_PICKED("k_csr_vector", pick_vec(epi, P.lanes, halo), dim3((P.nrows + rpb - 1) / rpb), dim3(sk::BLOCK), 0, g.cs, a, P.nrows);
    } break;
    case F_CC16_16: case F_CC16_32: {                             // 16-bit compressed columns
        const int k = tile_plan(P.variant);
        if (!P.cc[k].ok) return fail(SGPU_ERR_STATE, "compressed columns of plan %d were not built", k);
        a.blk_row = k ? P.csr.blk_row_big : P.csr.blk_row;
        a.nblk = k ? P.nblk_big : P.nblk;
        a.segtab = P.cc[k].segtab; a.segptr = P.cc[k].segptr; a.ccol = P.cc[k].ccol; a.cc_ob = P.cc_ob[k];
        SGPU_LAUNCH_PICKED("k_csr_cc16", pick_tile<1>(epi, P.lanes, k == 1, halo), dim3(a.nblk), dim3(sk::BLOCK), 0, g.cs, a);
    } break;
    case F_DENSE: {                                               // dense rows, one wave per row
        if (!P.dn.dense) return fail(SGPU_ERR_STATE, "the dense form was not built");
        if (halo) return fail(SGPU_ERR_STATE, "the dense form serves operators without a halo");
        a.blk_row = nullptr; a.nblk = 0;
        SGPU_LAUNCH_PICKED("k_dense_rows", pick_dense(epi), dim3((P.nrows + 3) / 4), dim3(sk::BLOCK), 0, g.cs, a, (const double *)P.dn.dense, P.nrows, P.ncols);
    } break;
    case F_WAVE: {                                                // wave-streamed long rows, 16-byte loads
        const int gl = std::max(8, P.lanes), rpb = sk::BLOCK / gl;
        a.blk_row = nullptr; a.nblk = 0;
        SGPU_LAUNCH_PICKED("k_csr_wave", pick_wave(epi, gl, halo), dim3((P.nrows + rpb - 1) / rpb), dim3(sk::BLOCK), 0, g.cs, a, P.nrows);
    } break;
    case F_CM16: case F_CM32: {                                   // compressed columns, entries in column order inside a block
        const int k = tile_plan(P.variant);
        if (!P.cm[k].ok) return fail(SGPU_ERR_STATE, "the column-major form of plan %d was not built", k);
        a.blk_row = k ? P.csr.blk_row_big : P.csr.blk_row;
        a.nblk = k ? P.nblk_big : P.nblk;
        a.segtab = P.cc[k].segtab; a.segptr = P.cc[k].segptr; a.cc_ob = P.cc_ob[k];
        a.val = P.cm[k].val; a.ccol = P.cm[k].col; a.dst = P.cm[k].dst; a.cmptr = P.cm[k].ptr;
        SGPU_LAUNCH_PICKED("k_csr_cm", pick_tile<2>(epi, P.lanes, k == 1, halo), dim3(a.nblk), dim3(sk::BLOCK), 0, g.cs, a);
    } break;
    case F_SELL: {                                                // sliced ELLPACK, a lane per row
        if (!P.sl_ok) return fail(SGPU_ERR_STATE, "the sliced-ELLPACK form was not built");
        a.blk_row = P.sv.sl_sorted ? P.sv.sl_perm : nullptr; a.nblk = P.nslices;
        a.val = P.sv.sl_val; a.ccol = P.sc.sl_col; a.segtab = P.sc.sl_base; a.segptr = P.sc.sl_segptr; a.cc_ob = P.sl_ob; a.cmptr = P.sv.sl_ptr; a.dst = P.sc.sl_len;
        // non-temporal streams once the stored operator is beyond the 256 MiB Infinity Cache (k_sellp in kernels.hip.h; 128^3 L1,
        // 843 MB: 127 -> 121 us, profiles/r03_sell_nt.log)
        static const int nt_env = std::getenv("SAENA_SELL_NT") ? std::atoi(std::getenv("SAENA_SELL_NT")) : -1;
        const bool nt = nt_env >= 0 ? nt_env != 0 : 10 * P.nnz + 18 * (int64_t)P.nrows > (int64_t)256 * 1024 * 1024;
        // sorted slices: a wave's 64 stores of y name up to 64 lines of its window -- plain stores, which the L2 merges into whole lines
        static const int sorted_plain = std::getenv("SAENA_SELL_SORTED_PLAIN_STORES") ? std::atoi(std::getenv("SAENA_SELL_SORTED_PLAIN_STORES")) : 1;
        if (P.sv.sl_sorted && sorted_plain) a.st_plain = 1;
        a.nt_from = nt ? resident_slices(P.nslices, 10.0 * (double)P.nnz / (double)std::max(1, P.nslices)) : 0;
        SGPU_LAUNCH_PICKED("k_sell", pick_sell(epi, halo, P.sl_pair, nt), dim3((P.nslices + 3) / 4), dim3(sk::BLOCK), 0, g.cs, a, P.nrows);
    } break;
    case F_XLDS: case F_XLDSR: {                                  // x in LDS, a workgroup per CU (F_XLDSR: four rows per group step -- short rows)
        if (!P.xlp.xl_ok || !P.xlc.xl_col) return fail(SGPU_ERR_STATE, "the x-in-LDS form was not built");
        a.blk_row = P.xlp.xl_blk; a.nblk = P.xl_nblk; a.ccol = P.xlc.xl_col;
        sk::XldsArgs w;
        w.info = P.xlp.xl_info; w.tab = P.xlc.xl_tab; w.acc = P.xlp.xl_acc; w.ncols = P.ncols;
        w.win = P.xl_win; w.acc_lds = P.xl_acc_lds ? 1 : 0; w.ord = P.xlp.xl_ord;
        SGPU_LAUNCH_PICKED("k_csr_xlds", P.variant == F_XLDSR ? pick_xldsr(epi, P.lanes, halo) : pick_xlds(epi, P.lanes, halo), dim3(P.xl_nblk), dim3(sk::XL_BLOCK), 0, g.cs, a, w);
    } break;
    case F_SELLP: {                                               // sliced ELLPACK values + row patterns, a lane per row
        if (!P.sp.sp_ok || !P.sv.sl_val) return fail(SGPU_ERR_STATE, "the row-pattern form was not built");
        a.blk_row = nullptr; a.nblk = P.nslices;
        a.val = P.sv.sl_val; a.cmptr = P.sv.sl_ptr; a.dst = P.sp.sp_pat; a.ptab = P.sp.sp_tab; a.pt_w = P.sp_w; a.pt_n = P.sp_n;
        a.rbase = P.sp.sp_rbase;
        const bool nt = row_pattern_nt(a, P.sp_bytes, P.nslices, 8.0 * (double)P.nnz / (double)std::max(1, P.nslices));
        a.uw = P.sl_uw;
        if (P.sp.sp_wide) {                                          // a table per workgroup: 1024 threads, 16 slices of 64 rows
            a.segptr = P.sp.sp_wgptr;
            SGPU_LAUNCH_PICKED("k_sellp", pick_sellp(epi, halo, P.sl_pair, nt, true), dim3((P.nslices + 15) / 16), dim3(sk::SPW_BLOCK), (size_t)P.sp_w * sizeof(int), g.cs, a, P.nrows);
        } else
        SGPU_LAUNCH_PICKED("k_sellp", pick_sellp(epi, halo, P.sl_pair, nt, false), dim3((P.nslices + 3) / 4), dim3(sk::BLOCK), (size_t)P.sp_n * (P.sp_w + 1) * sizeof(int), g.cs, a, P.nrows);
    } break;
    case F_SELLX: {                                               // sliced ELLPACK in the LDS windows, a workgroup per CU
        if (!P.sx.sx_ok || !P.xlp.xl_ok) return fail(SGPU_ERR_STATE, "the sliced-ELLPACK-in-LDS form was not built");
        a.blk_row = P.xlp.xl_blk; a.nblk = P.xl_nblk;
        sk::SellxArgs w;
        w.info = P.xlp.xl_info; w.bptr = P.sx.sx_bptr; w.sptr = P.sx.sx_sptr; w.meta = P.sx.sx_meta; w.val = P.sx.sx_val; w.col = P.sx.sx_col; w.acc = P.xlp.xl_acc; w.ncols = P.ncols;
        w.win = P.xl_win; w.acc_lds = P.xl_acc_lds ? 1 : 0;
        if (nt_rt == 0 && !std::getenv("SAENA_STREAM_NT")) a.nt = 10 * P.nnz > (int64_t)256 * 1024 * 1024 ? 1 : 0;      // non-temporal streams beyond the Infinity Cache (438 -> 426 us)
        SGPU_LAUNCH_PICKED("k_sellx", pick_sellx(epi, halo), dim3(P.xl_nblk), dim3(sk::XL_BLOCK), 0, g.cs, a, w);
    } break;
    case F_ROWT: {                                                // row templates: a thread per row, no operator stream at all
        if (!P.rt.rt_ok) return fail(SGPU_ERR_STATE, "the row-template form was not built");
        a.blk_row = nullptr; a.nblk = 0;
        a.val = P.rt.rt_vtab; a.dst = P.rt.rt_pat; a.ptab = P.rt.rt_itab; a.pt_w = P.rt_w; a.pt_n = P.rt_n;
        const bool nt = 26 * (int64_t)P.nrows > (int64_t)256 * 1024 * 1024;       // ids + x + y (+ rhs) beyond the Infinity Cache
        const size_t lds = (size_t)P.rt_n * ((size_t)P.rt_w * 8 + (size_t)(P.rt_w + 1) * 4);
        SGPU_LAUNCH_PICKED("k_rowt", pick_rowt(epi, halo, nt), dim3((P.nrows + sk::BLOCK - 1) / sk::BLOCK), dim3(sk::BLOCK), lds, g.cs, a, P.nrows);
    } break;
    case F_SELLP2: {                                              // k_sellp with a lane per two rows
        if (!P.sp2.sp2_ok || !P.sp.sp_ok) return fail(SGPU_ERR_STATE, "the row-paired row-pattern form was not built");
        a.blk_row = nullptr; a.nblk = P.sp2_nslices;
        a.val = P.sp2.sp2_val; a.cmptr = P.sp2.sp2_ptr; a.dst = P.sp.sp_pat; a.ptab = P.sp.sp_tab; a.pt_w = P.sp_w; a.pt_n = P.sp_n;
        const bool nt = row_pattern_nt(a, P.sp_bytes, P.sp2_nslices, 8.0 * (double)P.nnz / (double)std::max(1, P.sp2_nslices));
        a.ncols = P.ncols;
        a.uw = P.sp2_uw;
        static const int pre_env = std::getenv("SAENA_SELLP2_PRE") ? std::atoi(std::getenv("SAENA_SELLP2_PRE")) : 1;
        const bool pre = pre_env != 0 && !halo;
        if (P.sp.sp_wide) {                                          // a table per workgroup: 512 threads, 8 slices of 128 rows
            a.segptr = P.sp.sp_wgptr;
            SGPU_LAUNCH_PICKED("k_sellp2", pick_sellp2<true>(epi, halo, nt, pre), dim3((P.sp2_nslices + 7) / 8), dim3(sk::SPW2_BLOCK), (size_t)P.sp_w * sizeof(int), g.cs, a, P.nrows);
        } else
        SGPU_LAUNCH_PICKED("k_sellp2", pick_sellp2<false>(epi, halo, nt, pre), dim3((P.sp2_nslices + 3) / 4), dim3(sk::BLOCK), (size_t)P.sp_n * (P.sp_w + 1) * sizeof(int), g.cs, a, P.nrows);
    } break;
    case F_SELLPX: {                                              // k_sellp with x in LDS windows
        if (!P.spx.spx_ok || !P.sp.sp_ok || !P.sv.sl_val) return fail(SGPU_ERR_STATE, "the row-pattern form with x in LDS was not built");
        a.blk_row = nullptr; a.nblk = P.nslices;
        a.val = P.sv.sl_val; a.cmptr = P.sv.sl_ptr; a.dst = P.spx.spx_pat; a.ptab = reinterpret_cast<const int *>(P.spx.spx_tab.get()); a.pt_w = 0; a.pt_n = P.sp_n;
        a.segtab = P.spx.spx_win; a.segptr = P.spx.spx_wgptr; a.ncols = P.ncols;
        const bool nt = row_pattern_nt(a, P.sp_bytes, P.nslices, 8.0 * (double)P.nnz / (double)std::max(1, P.nslices));
        SGPU_LAUNCH_PICKED("k_sellpx", pick_sellpx(epi, halo, P.sl_pair, nt), dim3((P.nslices + sk::SPX_ROWS / 64 - 1) / (sk::SPX_ROWS / 64)), dim3(sk::SPX_BLOCK), 0, g.cs, a, P.nrows);
    } break;
    case F_VIDX: {                                                // row patterns + 8-bit value codes, a lane per row
        if (!P.vi.vi_ok || !P.sp.sp_ok) return fail(SGPU_ERR_STATE, "the value-indexed row-pattern form was not built");
        a.blk_row = nullptr; a.nblk = P.nslices ? P.nslices : (P.nrows + 63) / 64;
        a.dst = P.sp.sp_pat; a.ptab = P.sp.sp_tab; a.pt_w = P.sp_w; a.pt_n = P.sp_n; a.rbase = P.sp.sp_rbase;
        a.vcode = P.vi.vi_code; a.vcptr = P.vi.vi_cptr; a.vdict = P.vi.vi_dict; a.vdptr = P.vi.vi_dptr; a.uw = P.vi_uw8;
        const bool nt = row_pattern_nt(a, P.vi_bytes, a.nblk, (double)P.nnz / (double)std::max(1, a.nblk));     // (about a byte of codes per entry)
        const size_t lds = ((size_t)((P.sp_n * (P.sp_w + 1) + 1) & ~1)) * sizeof(int) + sk::VI_MAX * sizeof(double);
        if (P.vw_rows) {                                          // x in LDS windows: workgroups of vw_rows rows, the table as 16-bit LDS byte offsets
            const int k = xwin_slot(P.vw_rows), spb = P.vw_rows / 64;
            const CsrPart::XWin &X = P.vw[k];
            if (!X.ok) return fail(SGPU_ERR_STATE, "the x windows of the value-indexed form were not built");
            a.ptab = reinterpret_cast<const int *>(X.tab.get()); a.pt_w = X.plan.wp; a.segtab = X.win; a.ncols = P.ncols;
            if (vwfast::launch_takes(X.plan.fast_kind, halo, epi)) {   // the common path: the plan's argument, the launch's vectors and the arrays the plan points at
                vwfast::VwFast f = X.plan.fast;
                if (f.nblk != a.nblk) return fail(SGPU_ERR_STATE, "the x windows were planned for %d slices, the launch has %d", f.nblk, a.nblk);
                f.vcode = a.vcode; f.dst = a.dst; f.ptab = X.tab.get(); f.vdict = a.vdict;
                // the bit codes where build_xwin packed them: an eighth of the code stream, and the non-temporal rule is given what this launch reads
                const bool bits = X.plan.fast_kind == 2 && X.bits;
                // the rows as lane masks where build_xwin packed them: such a launch reads neither pattern ids (2 B a row: the mode has no
                // rowbase) nor codes but a record per slice, and the non-temporal rule is given that; it reports the bit codes' width
                const bool masks = bits && X.masks;
                bool ntf = nt;
                if (masks)
                    ntf = row_pattern_nt(a, P.vi_bytes - P.vi_code_bytes - 2 * (int64_t)P.nrows + (int64_t)vwmasks::REC_BYTES * a.nblk, a.nblk, (double)vwmasks::REC_BYTES);
                else if (bits)
                    ntf = row_pattern_nt(a, P.vi_bytes - P.vi_code_bytes + P.vi_code_bytes / 8, a.nblk, (double)P.nnz / 8.0 / (double)std::max(1, a.nblk));
                if (bits) { f.vcode = X.bits.get(); f.cbytes = vwfast::bit_slice_bytes(f.w8); }
                f.x = a.x; f.y = a.y; f.rhs = a.rhs; f.inv_diag = a.inv_diag; f.u = a.u; f.c0 = a.c0;
                f.nt_from = a.nt_from; f.st_plain = a.st_plain; f.nrows = P.nrows;
                f.masks = masks ? X.masks.get() : nullptr;
                P.vw_last = X.plan.fast_kind; P.vw_last_width = vwfast::code_width(bits); P.vw_last_rows = masks ? 1 : 0;
                SGPU_LAUNCH_PICKED("k_vidxw_fast", pick_vidxw_fast(P.vw_rows, epi, ntf, X.plan.fast_kind == 2, bits, masks), dim3((a.nblk + spb - 1) / spb), dim3(P.vw_rows), (size_t)X.plan.fast_lds, g.cs, f);
                break;
            }
            P.vw_last = 0; P.vw_last_width = 8; P.vw_last_rows = 0;
            SGPU_LAUNCH_PICKED("k_vidxw", pick_vidxw(epi, halo, nt), dim3((a.nblk + spb - 1) / spb), dim3(P.vw_rows), (size_t)X.plan.lds, g.cs, a, X.plan.head, P.nrows);
        } else
        SGPU_LAUNCH_PICKED("k_vidx", pick_vidx(epi, halo, nt), dim3((a.nblk + 3) / 4), dim3(sk::BLOCK), lds, g.cs, a, P.nrows);
    } break;
    }
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// dense storage with a halo: all rows in one launch after the exchange (k_dense_rows_halo)
int launch_dense_halo(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e, bool halo_is_f32, hipStream_t stream) {
    if (op->M == 0) return SGPU_OK;
    if (!op->loc.dn.dense || (!op->dense_rem && op->has_remote)) return fail(SGPU_ERR_STATE, "the dense form was not built");
    const sk::SpmvArgs a = spmv_args(x, y, e);
    SGPU_LAUNCH_PICKED("k_dense_rows_halo", pick_dense_halo(epi), dim3((op->M + 3) / 4), dim3(sk::BLOCK), 0, stream, a, (const double *)op->loc.dn.dense, (const double *)op->dense_rem,
                (int)op->M, op->loc.ncols, op->has_remote ? op->recvSize : 0, (const double *)op->recv_buf, halo_is_f32 ? (const float *)op->recv_f : (const float *)nullptr,
                op->halo_fp32 ? 1 : 0);       // (an injected halo arrives as float-rounded doubles: halo_f null, x still rounded)
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}
// the rows of an operator whose halo has arrived: interior rows + boundary rows, or the dense form's single launch
int launch_rows_after_exchange(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e, bool f32, hipStream_t stream);

// The rows that own remote entries, computed whole (local + halo products, one epilogue) on `stream`.
int launch_boundary(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e, bool halo_is_f32, hipStream_t stream) {
    if (op->rem.nrows == 0) return SGPU_OK;
    sk::BoundaryArgs b;
    b.s = spmv_args(x, y, e);
    b.s.row_ptr = op->loc.csr.row_ptr; b.s.col = op->loc.csr.col; b.s.val = op->loc.csr.val;
    b.rows = op->rem.csr.rows; b.nrows = op->rem.nrows;
    b.h_ptr = op->rem.csr.row_ptr; b.h_col = op->rem.csr.col; b.h_val = op->rem.csr.val;
    b.halo = op->recv_buf; b.halo_f = halo_is_f32 ? op->recv_f : nullptr;
    const int rpb = sk::BLOCK / op->bnd_lanes;
    SGPU_LAUNCH_PICKED("k_csr_boundary", pick_bnd(epi, op->bnd_lanes), dim3((b.nrows + rpb - 1) / rpb), dim3(sk::BLOCK), 0, stream, b);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// the halo exchange proper: one grouped send/recv per neighbour (src/saena_matrix_matvec.cpp:32-41 MPI_Irecv/Isend)
int exchange_group(sgpu_op *op, bool f32, hipStream_t st) {
    NCCLCHK(ncclGroupStart());
    for (size_t i = 0; i < op->sendRank.size(); ++i) {
        if (f32) NCCLCHK(ncclSend(op->send_f + op->sendDispl[i], (size_t)op->sendCount[i], ncclFloat, op->sendRank[i], g.comm, st));
        else NCCLCHK(ncclSend(op->send_buf + op->sendDispl[i], (size_t)op->sendCount[i], ncclDouble, op->sendRank[i], g.comm, st));
    }
    for (size_t i = 0; i < op->recvRank.size(); ++i) {
        if (f32) NCCLCHK(ncclRecv(op->recv_f + op->recvDispl[i], (size_t)op->recvCount[i], ncclFloat, op->recvRank[i], g.comm, st));
        else NCCLCHK(ncclRecv(op->recv_buf + op->recvDispl[i], (size_t)op->recvCount[i], ncclDouble, op->recvRank[i], g.comm, st));
    }
    NCCLCHK(ncclGroupEnd());
    ++g_launches;
    return SGPU_OK;
}

int launch_rows_after_exchange(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e, bool f32, hipStream_t stream) {
    if (is_dense(op->loc.variant) && op->has_remote) return launch_dense_halo(op, epi, x, y, e, f32, stream);
    CHK(launch_part(op->loc, epi, x, y, e, op->has_remote ? op->skip : nullptr));     // (always on cs: callers pass cs)
    if (op->has_remote) CHK(launch_boundary(op, epi, x, y, e, f32, stream));
    return SGPU_OK;
}

// Host-routed exchange: pack -> host -> callback -> device, then the same interior / boundary kernels, all on cs.
int apply_host_transport(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e) {
    const bool f32 = op->halo_fp32 != 0;
    const size_t eb = f32 ? sizeof(float) : sizeof(double);
    std::vector<char> hs((size_t)op->vIndexSize * eb), hr((size_t)op->recvSize * eb);
    if (op->vIndexSize) {
        const dim3 grid(std::min(sk::PACK_MAX_BLOCKS, (op->vIndexSize + sk::BLOCK - 1) / sk::BLOCK));
        if (f32) SGPU_LAUNCH(sk::k_pack_f32, grid, dim3(sk::BLOCK), 0, g.cs, x, op->vIndex, op->send_f, op->vIndexSize, (const uint64_t *)nullptr, (uint64_t)0);
        else SGPU_LAUNCH(sk::k_pack, grid, dim3(sk::BLOCK), 0, g.cs, x, op->vIndex, op->send_buf, op->vIndexSize, 0, (const uint64_t *)nullptr, (uint64_t)0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs.data(), f32 ? (const void *)op->send_f : (const void *)op->send_buf, hs.size(), hipMemcpyDeviceToHost, g.cs));
    }
    HIPCHK(hipStreamSynchronize(g.cs));
    if (g.xchg(g.xuser, hs.data(), op->sendRank.data(), op->sendCount.data(), (int)op->sendRank.size(),
               hr.data(), op->recvRank.data(), op->recvCount.data(), (int)op->recvRank.size(), (int)eb) != 0)
        return fail(SGPU_ERR_RCCL, "host transport: exchange callback failed");
    if (op->recvSize) HIPCHK(hipMemcpyAsync(f32 ? (void *)op->recv_f : (void *)op->recv_buf, hr.data(), hr.size(), hipMemcpyHostToDevice, g.cs));
    CHK(launch_rows_after_exchange(op, epi, x, y, e, f32, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));                  // the staging vectors die with this frame
    return SGPU_OK;
}

// How apply() orders the exchange of `op` against its rows (the values of sgpu_debug_exchange_mode).  fresh_peer: this exchange is
// the first with one of its peers in one direction, which runs in the plainest two-stream mode (see apply()).
enum { XM_NONE = 0, XM_HOST = 1, XM_ONE_STREAM = 2, XM_KERNEL_FLAGS = 3, XM_VALUE_OPS = 4, XM_EVENTS = 5 };
int exchange_mode(const sgpu_op *op, bool fresh_peer) {
    if (op->injected || !(op->vIndexSize || op->recvSize)) return XM_NONE;
    if (g.xchg) return XM_HOST;
    if (!g.comm) return XM_NONE;
    if (op->single_stream || (is_dense(op->loc.variant) && op->has_remote)) return XM_ONE_STREAM;      // (the dense form has no interior/boundary split)
    const bool plain = fresh_peer || op->events_only;
    if (g.inkernel_sync && op->loc.nblk > 0 && !plain) return XM_KERNEL_FLAGS;
    if (g.value_ops && !plain) return XM_VALUE_OPS;
    return XM_EVENTS;
}

// y = epi(A x).  With a communicator the two streams split the ROWS, not the phases:
//   cs (compute): interior rows -- every row without remote entries -- straight away;
//   hs (halo):    wait for the inputs (ev_x) -> pack -> ncclSend/ncclRecv group -> boundary rows whole;
//   cs joins hs (ev_halo) before anything later on cs can see y or reuse x.
// The exchange chain has no event hop in its middle (each hop costs ~10 us on this stack, see
// profiles/r01_halo_loopback_trace.md) and the interior launch never waits for it: this is where the
// reference overlaps MPI_Isend/Irecv with its local loop (src/saena_matrix_matvec.cpp:32-80).
int apply(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e) {
    int mode = exchange_mode(op, false);
    if (mode == XM_HOST) return apply_host_transport(op, epi, x, y, e);
    if (mode == XM_NONE) {
        if (op->has_remote && op->injected)             // halo supplied by the caller (tests): same kernels, one stream
            return launch_rows_after_exchange(op, epi, x, y, e, false, g.cs);
        // an operator with remote entries but no way to fetch them (no communicator, no host transport, no injected
        // halo): the local part alone would be a silently wrong product (a binding that forgot the unique id, or a
        // 1-rank context fed N-rank layouts).  sgpu_debug_allow_local_only lifts this for plan/launch tests.
        if ((op->has_remote || op->recvSize) && !g.multi() && !op->local_only_ok)
            return fail(SGPU_ERR_STATE, "operator has %d halo entries but this context has no communicator (sgpu_init was given nranks=%d, no unique id)",
                        op->recvSize, g.nranks);
        if (is_dense(op->loc.variant) && op->halo_fp32)    // matvec_dense_float rounds the rank's own block of x as well
            return launch_dense_halo(op, epi, x, y, e, false, g.cs);
        return launch_part(op->loc, epi, x, y, e);      // no halo: the local part is the whole operator
    }
    const bool f32 = op->halo_fp32 != 0;                 // both ends of a link must agree: the flag alone decides the wire type
    const unsigned *skip = op->has_remote ? op->skip : nullptr;
    if (mode == XM_ONE_STREAM) {
        // S  one stream.  A SHORT local kernel has nothing to hide the exchange behind, and the fork/join between the
        //    two streams then costs more than it overlaps: pack -> send/recv group -> interior rows -> boundary rows,
        //    all on cs, in stream order (4 enqueues instead of 6, no flag, no event; capturable in a hipGraph).
        if (op->vIndexSize) {
            const dim3 grid(std::min(sk::PACK_MAX_BLOCKS, (op->vIndexSize + sk::BLOCK - 1) / sk::BLOCK));
            if (f32) SGPU_LAUNCH(sk::k_pack_f32, grid, dim3(sk::BLOCK), 0, g.cs, x, op->vIndex, op->send_f, op->vIndexSize, (const uint64_t *)nullptr, (uint64_t)0);
            else SGPU_LAUNCH(sk::k_pack, grid, dim3(sk::BLOCK), 0, g.cs, x, op->vIndex, op->send_buf, op->vIndexSize, 0, (const uint64_t *)nullptr, (uint64_t)0);
            HIPCHK(hipGetLastError());
        }
        CHK(exchange_group(op, f32, g.cs));
        return launch_rows_after_exchange(op, epi, x, y, e, f32, g.cs);
    }
    const uint64_t n = ++g.seq;
    // Three ways to express the two dependencies (fork: hs after cs's earlier work; join: cs after hs), fastest first:
    //  K  flags polled by kernels: block 0 of the interior launch stores flag_x = n when it starts, the pack launch
    //     polls it; a one-wave k_flag_set behind the boundary kernel stores flag_h = n, a one-wave k_flag_wait on cs
    //     polls it.  No runtime helper launches, no event hops.
    //  V  hipStreamWriteValue64 / hipStreamWaitValue64 (each is a ~4 us helper launch, ~5 us per hop)
    //  E  events (~11 us per hop)
    // Invariant of all three: whatever polls or waits was enqueued AFTER the thing it waits for -- nothing on the GPU
    // ever depends on a launch the host has yet to make.  (So a device-wide synchronisation inside an RCCL host call,
    // e.g. while it connects a new peer, always completes; and an error return leaves no stream waiting.)
    // The first exchange with a peer makes RCCL set up the connection inside ncclGroupEnd (allocations, IPC handles,
    // possibly device-wide synchronisation): that one runs in the plainest mode, events, with no polling kernel around.
    // (tracked per DIRECTION: RCCL sets the send side and the receive side of a peer up separately, so an operator
    // that only sends to r followed by one that only receives from r is two fresh connections)
    bool fresh_peer = false;
    if (g.peer_seen.size() != (size_t)g.nranks) g.peer_seen.assign((size_t)g.nranks, 0);
    for (int r : op->sendRank) if (!(g.peer_seen[(size_t)r] & 1)) { fresh_peer = true; g.peer_seen[(size_t)r] |= 1; }
    for (int r : op->recvRank) if (!(g.peer_seen[(size_t)r] & 2)) { fresh_peer = true; g.peer_seen[(size_t)r] |= 2; }
    // A LONG interior kernel hides the whole exchange chain whichever way the streams are ordered (16.6 M rows per GPU,
    // configs[3]: ~290 us of interior work against a 48 us chain in the plainest mode), so such operators take plain
    // events: nothing polls, nothing depends on co-residency.  The polling forms earn their keep in between.
    if (fresh_peer) mode = exchange_mode(op, true);
    const bool K = mode == XM_KERNEL_FLAGS, V = mode == XM_VALUE_OPS;
    if (K) {
        CHK(launch_part(op->loc, epi, x, y, e, skip, n));
    } else {
        if (V) HIPCHK(hipStreamWriteValue64(g.cs, g.flag_x, n, 0));
        else HIPCHK(hipEventRecord(op->ev_x, g.cs));
        CHK(launch_part(op->loc, epi, x, y, e, skip));
    }
    auto hs_chain = [&]() -> int {
        const bool pack_waits = K && op->vIndexSize > 0;
        if (K && !pack_waits) {
            SGPU_LAUNCH(sk::k_flag_wait, dim3(1), dim3(64), 0, g.hs, (const uint64_t *)g.kflag_x, n);
            HIPCHK(hipGetLastError());
        } else if (!K) {
            if (V) HIPCHK(hipStreamWaitValue64(g.hs, g.flag_x, n, hipStreamWaitValueGte, ~0ull));
            else HIPCHK(hipStreamWaitEvent(g.hs, op->ev_x, 0));
        }
        if (op->vIndexSize) {
            const dim3 grid(std::min(sk::PACK_MAX_BLOCKS, (op->vIndexSize + sk::BLOCK - 1) / sk::BLOCK));
            const uint64_t *flag = pack_waits ? g.kflag_x : nullptr;
            if (f32) SGPU_LAUNCH(sk::k_pack_f32, grid, dim3(sk::BLOCK), 0, g.hs, x, op->vIndex, op->send_f, op->vIndexSize, flag, n);
            else SGPU_LAUNCH(sk::k_pack, grid, dim3(sk::BLOCK), 0, g.hs, x, op->vIndex, op->send_buf, op->vIndexSize, 0, flag, n);
            HIPCHK(hipGetLastError());
        }
        CHK(exchange_group(op, f32, g.hs));
        if (op->has_remote) CHK(launch_boundary(op, epi, x, y, e, f32, g.hs));
        return SGPU_OK;
    };
    const int st = hs_chain();
    CHK(st);
    // join: nothing later on cs may see y (or overwrite x and the send buffers) before hs is through
    if (K) {
        SGPU_LAUNCH(sk::k_flag_set, dim3(1), dim3(64), 0, g.hs, g.kflag_h, n);
        HIPCHK(hipGetLastError());
        SGPU_LAUNCH(sk::k_flag_wait, dim3(1), dim3(64), 0, g.cs, (const uint64_t *)g.kflag_h, n);
        HIPCHK(hipGetLastError());
        return SGPU_OK;
    }
    if (V) {
        HIPCHK(hipStreamWriteValue64(g.hs, g.flag_h, n, 0));
        HIPCHK(hipStreamWaitValue64(g.cs, g.flag_h, n, hipStreamWaitValueGte, ~0ull));
    } else {
        HIPCHK(hipEventRecord(op->ev_halo, g.hs));
        HIPCHK(hipStreamWaitEvent(g.cs, op->ev_halo, 0));
    }
    return SGPU_OK;
}

int ensure_tmp(sgpu_op *op) {
    if (!op->tmp) HIPCHK(alloc_vec(op->tmp, op->M));
    return SGPU_OK;
}
int ensure_d(sgpu_op *op) {
    if (!op->dvec) HIPCHK(alloc_vec(op->dvec, op->M));
    return SGPU_OK;
}

int grid_for(size_t n) { return (int)std::min<size_t>(2048, std::max<size_t>(1, (n / 2 + sk::BLOCK - 1) / sk::BLOCK)); }

// iter Jacobi sweeps ping-ponging u <-> alt; *out = buffer holding the result.
int zero_sweep(sgpu_op *op, int cheby, double c0, const double *rhs, double *y, double *d) {
    if (op->M == 0) return SGPU_OK;
    SGPU_LAUNCH(sk::k_zero_sweep, dim3(grid_for(2 * (size_t)op->M)), dim3(sk::BLOCK), 0, g.cs, cheby, c0, rhs, (const double *)op->inv_diag,
                       y, d, (size_t)op->M);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// zero_first: the iterate in `u` is known to be zero (its CONTENT is not read): the first sweep skips the matrix
// zero_done: that first sweep has already been written to `alt` by the restriction's epilogue (EPI_RSWEEP)
int jacobi_pp(sgpu_op *op, int iter, double omega, double *u, double *alt, const double *rhs, double **out, bool zero_first = false, bool zero_done = false) {
    if (!op->inv_diag && op->M > 0) return fail(SGPU_ERR_ARG, "jacobi: operator has no inv_diag");   // (a rank may own no rows of a level)
    double *cur = u, *nxt = alt;
    for (int j = 0; j < iter; ++j) {
        if (j == 0 && zero_first) {
            if (!zero_done) CHK(zero_sweep(op, 0, omega, rhs, nxt, nullptr));
        } else {
            EpiArgs e; e.rhs = rhs; e.inv_diag = op->inv_diag; e.u = cur; e.c0 = omega;
            CHK(apply(op, sk::EPI_JACOBI, cur, nxt, e));
        }
        std::swap(cur, nxt);
    }
    *out = cur;
    return SGPU_OK;
}

// saena_matrix::chebyshev scalars, src/saena_matrix.cpp:1084-1091,1113-1117
int cheby_pp(sgpu_op *op, int iter, double eig_max, double *u, double *alt, const double *rhs, double **out, bool zero_first = false, bool zero_done = false) {
    if (!op->inv_diag && op->M > 0) return fail(SGPU_ERR_ARG, "chebyshev: operator has no inv_diag");
    CHK(ensure_d(op));
    const double alpha = 0.13 * eig_max, beta = eig_max;
    const double delta = (beta - alpha) / 2.0, theta = (beta + alpha) / 2.0;
    const double s1 = theta / delta, twos1 = 2.0 * s1;
    double rhok = 1.0 / s1;
    double *cur = u, *nxt = alt;
    if (iter <= 0) { *out = cur; return SGPU_OK; }
    if (zero_first) {
        if (!zero_done) CHK(zero_sweep(op, 1, 1.0 / theta, rhs, nxt, op->dvec));
        std::swap(cur, nxt);
    } else {
        EpiArgs e; e.rhs = rhs; e.inv_diag = op->inv_diag; e.u = cur; e.d = op->dvec; e.c0 = 1.0 / theta;
        CHK(apply(op, sk::EPI_CHEBY0, cur, nxt, e));
        std::swap(cur, nxt);
    }
    for (int i = 1; i < iter; ++i) {
        const double rhokp1 = 1.0 / (twos1 - rhok);
        const double two_rhokp1 = 2.0 * rhokp1;
        const double d1 = rhokp1 * rhok;
        const double d2 = two_rhokp1 / delta;
        rhok = rhokp1;
        EpiArgs e; e.rhs = rhs; e.inv_diag = op->inv_diag; e.u = cur; e.d = op->dvec; e.c0 = d2; e.c1 = d1;
        CHK(apply(op, sk::EPI_CHEBYK, cur, nxt, e));
        std::swap(cur, nxt);
    }
    *out = cur;
    return SGPU_OK;
}

int dot_local_async(const double *x, const double *y, size_t n, double *dout) {
    const int nb = (int)std::min<size_t>(g.n_partials, std::max<size_t>(1, (n + sk::BLOCK - 1) / sk::BLOCK));
    SGPU_LAUNCH(sk::k_dot_partial, dim3(nb), dim3(sk::BLOCK), 0, g.cs, x, y, n, g.partials);
    SGPU_LAUNCH(sk::k_reduce_partials, dim3(1), dim3(sk::BLOCK), 0, g.cs, g.partials, nb, dout);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// global dot whose result stays on the device (S[slot]); with a communicator the rank sums are combined in place
int dot_dev(const double *x, const double *y, size_t n, int slot) {
    CHK(dot_local_async(x, y, n, g.dscalar + slot));
    if (g.comm) NCCLCHK(ncclAllReduce(g.dscalar + slot, g.dscalar + slot, 1, ncclDouble, ncclSum, g.comm, g.cs));
    if (g.xchg) {                                        // host-routed: down, sum over ranks, back up (later kernels read S[slot])
        double v = 0;
        HIPCHK(hipMemcpyAsync(&v, g.dscalar + slot, sizeof v, hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        CHK(host_allreduce(&v, 1));
        HIPCHK(hipMemcpyAsync(g.dscalar + slot, &v, sizeof v, hipMemcpyHostToDevice, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
    }
    return SGPU_OK;
}
int dot_nblocks(size_t n) { return (int)std::min<size_t>(g.n_partials, std::max<size_t>(1, (n + sk::BLOCK - 1) / sk::BLOCK)); }
// u -= (S[ia]/S[ib]) p; r -= (S[ia]/S[ib]) h; S[iout] = global r.r of the new r; *host_out = the same (ONE host sync)
int pcg_update_dev(int ia, int ib, const double *p, const double *h, double *u, double *r, size_t n, int iout, double *host_out) {
    const int nb = dot_nblocks(n);
    SGPU_LAUNCH(sk::k_pcg_update_dev, dim3(nb), dim3(sk::BLOCK), 0, g.cs, (const double *)g.dscalar, ia, ib, p, h, u, r, n, g.partials);
    SGPU_LAUNCH(sk::k_reduce_partials, dim3(1), dim3(sk::BLOCK), 0, g.cs, g.partials, nb, g.dscalar + iout);
    HIPCHK(hipGetLastError());
    if (g.comm) NCCLCHK(ncclAllReduce(g.dscalar + iout, g.dscalar + iout, 1, ncclDouble, ncclSum, g.comm, g.cs));
    HIPCHK(hipMemcpyAsync(g.hscalar + iout, g.dscalar + iout, sizeof(double), hipMemcpyDeviceToHost, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    if (g.xchg) {
        CHK(host_allreduce(g.hscalar + iout, 1));
        HIPCHK(hipMemcpyAsync(g.dscalar + iout, g.hscalar + iout, sizeof(double), hipMemcpyHostToDevice, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
    }
    *host_out = g.hscalar[iout];
    return SGPU_OK;
}
int pcg_direction_dev(int ia, int ib, const double *z, double *p, size_t n) {
    SGPU_LAUNCH(sk::k_pcg_direction_dev, dim3(grid_for(2 * n)), dim3(sk::BLOCK), 0, g.cs, (const double *)g.dscalar, ia, ib, z, p, n);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// y = x - mean(x) over this rank's n rows (y may be x): the sum on the dot's grid into the dots' partial sums, S[CENTER_SLOT], then
// the subtraction.  Three launches, nothing comes down.  Slot 3 is no solver's: sgpu_dot has 0, the Krylov loops 4..7, global_sum 8..
constexpr int CENTER_SLOT = 3;
int center_async(const double *x, double *y, size_t n) {
    if (n == 0) return SGPU_OK;
    const int nb = dot_nblocks(n);
    SGPU_LAUNCH(sk::k_sum_partial, dim3(nb), dim3(sk::BLOCK), 0, g.cs, x, n, g.partials);
    SGPU_LAUNCH(sk::k_reduce_partials, dim3(1), dim3(sk::BLOCK), 0, g.cs, g.partials, nb, g.dscalar + CENTER_SLOT);
    SGPU_LAUNCH(sk::k_center, dim3(grid_for(2 * n)), dim3(sk::BLOCK), 0, g.cs, (const double *)(g.dscalar + CENTER_SLOT), x, y, n);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

const double JACOBI_OMEGA_REF = (double)(float)(2.0 / 3);   // saena_matrix.h:182

int global_sum(double *v, int n) {
    if (n > 8) return fail(SGPU_ERR_ARG, "global_sum: at most 8 values");
    if (g.xchg) return host_allreduce(v, n);
    if (g.comm) {
        HIPCHK(hipMemcpyAsync(g.dscalar + 8, v, n * sizeof(double), hipMemcpyHostToDevice, g.cs));
        NCCLCHK(ncclAllReduce(g.dscalar + 8, g.dscalar + 8, (size_t)n, ncclDouble, ncclSum, g.comm, g.cs));
        HIPCHK(hipMemcpyAsync(g.hscalar + 8, g.dscalar + 8, n * sizeof(double), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        for (int i = 0; i < n; ++i) v[i] = g.hscalar[8 + i];
    }
    return SGPU_OK;
}

} // namespace

// ===========================================================================
extern "C" {

const char *sgpu_last_error(void) { return g_err.c_str(); }

int sgpu_get_unique_id(void *out128) {
    if (!out128) return fail(SGPU_ERR_ARG, "null unique-id buffer");
    static_assert(sizeof(ncclUniqueId) == SGPU_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    memcpy(out128, &id, sizeof id);
    return SGPU_OK;
}

// The exchange chain of a multi-rank apply, measured on THIS communicator: pack kernel -> one grouped ncclSend/ncclRecv of a
// halo-sized message (32 KiB) with the neighbouring rank (rank ^ 1; the last rank of an odd job and a one-rank
// communicator exchange with themselves) -> a small kernel on the received data, on the compute stream, 20 times after 5
// warm-up rounds (the first connects the peers), timed with events.  Every rank takes the maximum over the ranks, so the
// agglomeration decisions that start from it (host/amg_setup.h: next_stride) are the same everywhere.  The reference
// times a dummy matvec per level for the same decision (saena_matrix::decide_shrinking, src/saena_matrix_shrink.cpp:3-118).
static int calibrate_chain() {
    const int n = 4096;                                  // doubles: about one face of a 64^3 block
    DevArr<double> a_, b_;
    HIPCHK(a_.alloc(n)); HIPCHK(b_.alloc(n));
    double *a = a_, *b = b_;
    struct Free { hipEvent_t e0 = nullptr, e1 = nullptr; ~Free() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); } } fr;
    HIPCHK(hipMemsetAsync(a, 0, n * sizeof(double), g.cs));
    HIPCHK(hipEventCreate(&fr.e0)); HIPCHK(hipEventCreate(&fr.e1));
    int peer = g.rank ^ 1;
    if (peer >= g.nranks) peer = g.rank;
    auto round = [&]() -> int {
        SGPU_LAUNCH(sk::k_axpby, dim3((n + sk::BLOCK - 1) / sk::BLOCK), dim3(sk::BLOCK), 0, g.cs, 1.0, (const double *)a, 0.0, b, (size_t)n);      // "pack"
        NCCLCHK(ncclGroupStart());
        NCCLCHK(ncclSend(b, n, ncclDouble, peer, g.comm, g.cs));
        NCCLCHK(ncclRecv(a, n, ncclDouble, peer, g.comm, g.cs));
        NCCLCHK(ncclGroupEnd());
        SGPU_LAUNCH(sk::k_axpby, dim3((n + sk::BLOCK - 1) / sk::BLOCK), dim3(sk::BLOCK), 0, g.cs, 1.0, (const double *)a, 0.0, b, (size_t)n);      // "boundary rows"
        return SGPU_OK;
    };
    for (int i = 0; i < 5; ++i) CHK(round());
    HIPCHK(hipStreamSynchronize(g.cs));
    const int reps = 20;
    HIPCHK(hipEventRecord(fr.e0, g.cs));
    for (int i = 0; i < reps; ++i) CHK(round());
    HIPCHK(hipEventRecord(fr.e1, g.cs));
    HIPCHK(hipEventSynchronize(fr.e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, fr.e0, fr.e1));
    // what a real apply adds to this ping-pong: the fork and the join of its two streams (~9 us with the in-kernel flags:
    // 35.5 us per SpMV with a halo against 26.4-27 us of local kernel, profiles/r01_halo_loopback.md).  With RCCL self
    // send/recv on one GPU the sum is the 23 us the model's constant was taken from.
    double us = (double)ms * 1e3 / reps + 9.0;
    // the same number on every rank: the maximum
    HIPCHK(hipMemcpyAsync(g.dscalar, &us, sizeof(double), hipMemcpyHostToDevice, g.cs));
    NCCLCHK(ncclAllReduce(g.dscalar, g.dscalar, 1, ncclDouble, ncclMax, g.comm, g.cs));
    HIPCHK(hipMemcpyAsync(&us, g.dscalar, sizeof(double), hipMemcpyDeviceToHost, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    // The agglomeration rules compare this number with thresholds (T1 <= chain, chain > 2 T1 / active): a 20-rep event timing
    // moves by a microsecond or two from run to run, and near a threshold that would move a coarse level between ranks -- and with
    // it the order of its reductions (round-3 advisor finding).  The model therefore sees the measurement on a coarse grid, steps
    // of sqrt(2) around the 23 us constant (16.3, 23, 32.5, 46, ...): a run-to-run wobble stays inside a step except at its edges,
    // and SAENA_SHRINK_CHAIN_US pins it for tests and benches that depend on where a level lives.
    const double raw = us;
    us = 23.0 * std::exp2(std::round(2.0 * std::log2(std::max(us, 1.0) / 23.0)) / 2.0);
    g.chain_us = us;
    saena_host::g_measured_chain_us = us;
    if (std::getenv("SAENA_SETUP_TIMING") && g.rank == 0) fprintf(stderr, "[sgpu] exchange chain on this communicator: %.1f us measured (pack -> send/recv of %d doubles with rank %d -> rows, + 9 us of fork / join), %.1f us in the agglomeration model\n", raw, n, peer, us);
    return SGPU_OK;
}

int sgpu_init(int device_id, int rank, int nranks, const void *uid) {
    if (g.live) return fail(SGPU_ERR_STATE, "sgpu_init called twice");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(SGPU_ERR_ARG, "bad rank %d of %d", rank, nranks);
    if (nranks > 1 && !uid) return fail(SGPU_ERR_ARG, "nranks > 1 needs an RCCL unique id");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev == 0) return fail(SGPU_ERR_HIP, "no HIP device visible: libsaena_amd needs an MI355X (there is no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(SGPU_ERR_ARG, "device %d not in [0,%d)", device_id, ndev);
    // host waits spin instead of sleeping on an interrupt: the Krylov loop synchronises once per iteration (the
    // convergence test) and a V-cycle at 128^3 is 2 ms -- a 30-50 us wake-up is 2 % of it.  Refused when the process has
    // already fixed the policy: not an error.
    HIPCHK(hipSetDevice(device_id));                    // first: the flags below apply to the CURRENT device
    if (!std::getenv("SAENA_NO_SPIN_WAIT") && hipSetDeviceFlags(hipDeviceScheduleSpin) != hipSuccess) (void)hipGetLastError();
    { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && n > 0) g.ncu = n; }
    g.device = device_id; g.rank = rank; g.nranks = nranks;
    HIPCHK(hipStreamCreateWithFlags(&g.cs, hipStreamNonBlocking));
    {   // the halo stream's small kernels (pack, RCCL, boundary rows) must not queue behind the interior launch
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        const int prio = std::getenv("SAENA_HALO_STREAM_PRIORITY") ? std::atoi(std::getenv("SAENA_HALO_STREAM_PRIORITY")) : greatest;
        HIPCHK(hipStreamCreateWithPriority(&g.hs, hipStreamNonBlocking, prio));
    }
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&g.partials), g.n_partials * sizeof(double)));
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&g.cblk), ((size_t)g.n_partials + 1) * 8 * sizeof(double)));
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&g.dscalar), 16 * sizeof(double)));
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&g.hscalar), 16 * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&g.dint), 16 * sizeof(int)));
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&g.hint), 16 * sizeof(int), hipHostMallocDefault));
    if (!std::getenv("SAENA_NO_STREAM_VALUE_OPS") &&
        hipExtMallocWithFlags(reinterpret_cast<void **>(&g.flag_x), 8, hipMallocSignalMemory) == hipSuccess &&
        hipExtMallocWithFlags(reinterpret_cast<void **>(&g.flag_h), 8, hipMallocSignalMemory) == hipSuccess &&
        hipStreamWriteValue64(g.cs, g.flag_x, 0, 0) == hipSuccess && hipStreamWriteValue64(g.hs, g.flag_h, 0, 0) == hipSuccess &&
        hipStreamWaitValue64(g.hs, g.flag_x, 0, hipStreamWaitValueGte, ~0ull) == hipSuccess &&
        hipStreamSynchronize(g.cs) == hipSuccess && hipStreamSynchronize(g.hs) == hipSuccess) {
        g.value_ops = true;
    } else {
        (void)hipGetLastError();
        if (g.flag_x) { hipFree(g.flag_x); g.flag_x = nullptr; }
        if (g.flag_h) { hipFree(g.flag_h); g.flag_h = nullptr; }
    }
    if (!std::getenv("SAENA_NO_INKERNEL_SYNC")) {
        char *fl = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&fl), 512));
        HIPCHK(hipMemsetAsync(fl, 0, 512, g.cs));        // (on cs and waited for: neither cs nor hs waits for a memset on the null stream)
        HIPCHK(hipStreamSynchronize(g.cs));
        g.kflag_x = reinterpret_cast<uint64_t *>(fl); g.kflag_h = reinterpret_cast<uint64_t *>(fl + 128);
        g.inkernel_sync = true;
    }
    if (uid) {      // also with one rank when an id is given: the RCCL paths (self send/recv included) then run for real
        ncclUniqueId id;
        memcpy(&id, uid, sizeof id);
        NCCLCHK(ncclCommInitRank(&g.comm, nranks, id, rank));
    }
    g.live = true;
    sgpu_install_spgemm_hook(1);         // the AMG setup's Galerkin products run on this device from now on (sgpu_spgemm.hip)
    sgpu_install_eig_hook(1);            // and, where the caller opts in, its eig_max estimates (sgpu_lanczos.hip.inc)
    if (g.comm && !std::getenv("SAENA_NO_CHAIN_CALIBRATION")) {
        const int s = calibrate_chain();
        if (s != SGPU_OK) { sgpu_finalize(); return s; }      // streams, buffers and the communicator go with the failed context (the error text stays)
    }
    return SGPU_OK;
}

int sgpu_debug_init_host_transport(int device_id, int rank, int nranks, sgpu_host_exchange_fn exchange,
                                   sgpu_host_allreduce_fn allreduce_sum, void *user) {
    if (!exchange || !allreduce_sum) return fail(SGPU_ERR_ARG, "null transport callback");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(SGPU_ERR_ARG, "bad rank %d of %d", rank, nranks);
    CHK(sgpu_init(device_id, 0, 1, nullptr));
    g.rank = rank; g.nranks = nranks;
    g.xchg = exchange; g.ared = allreduce_sum; g.xuser = user;
    return SGPU_OK;
}

int sgpu_finalize(void) {
    if (!g.live) return SGPU_OK;
    sgpu_install_spgemm_hook(0);
    sgpu_install_eig_hook(0);
    hipDeviceSynchronize();
    if (g.comm) { ncclCommDestroy(g.comm); g.comm = nullptr; }
    if (g.tk0) { hipEventDestroy(g.tk0); hipEventDestroy(g.tk1); g.tk0 = g.tk1 = nullptr; }
    hipFree(g.partials); hipFree(g.cblk); hipFree(g.dscalar); hipHostFree(g.hscalar); hipFree(g.dint); hipHostFree(g.hint);
    if (g.flag_x) hipFree(g.flag_x);
    if (g.flag_h) hipFree(g.flag_h);
    if (g.kflag_x) hipFree(g.kflag_x);
    hipStreamDestroy(g.cs); hipStreamDestroy(g.hs);
    g = Ctx();
    saena_host::g_measured_chain_us = 0.0;
    return SGPU_OK;
}

int sgpu_rank(void) { return g.rank; }
int sgpu_nranks(void) { return g.nranks; }

int sgpu_device_sync(void) {
    CHK(need_ctx());
    HIPCHK(hipStreamSynchronize(g.hs));
    HIPCHK(hipStreamSynchronize(g.cs));
    return SGPU_OK;
}

int sgpu_barrier(void) {
    CHK(sgpu_device_sync());
    if (g.xchg) { double z = 0; CHK(host_allreduce(&z, 1)); }
    if (g.comm) {
        HIPCHK(hipMemsetAsync(g.dint, 0, sizeof(int), g.cs));
        NCCLCHK(ncclAllReduce(g.dint, g.dint, 1, ncclInt, ncclSum, g.comm, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
    }
    return SGPU_OK;
}

// ---- vectors ----
int sgpu_vec_alloc(value_t **dev, size_t n) {
    CHK(need_ctx());
    if (!dev) return fail(SGPU_ERR_ARG, "null out pointer");
    if (hipMalloc(reinterpret_cast<void **>(dev), std::max<size_t>(1, n) * sizeof(value_t)) != hipSuccess)
        return fail(SGPU_ERR_NOMEM, "hipMalloc of %zu doubles failed", n);
    return SGPU_OK;
}
int sgpu_vec_free(value_t *dev) { CHK(need_ctx()); HIPCHK(hipFree(dev)); return SGPU_OK; }
int sgpu_vec_upload(value_t *dev, const value_t *host, size_t n) {
    CHK(need_ctx());
    HIPCHK(hipMemcpyAsync(dev, host, n * sizeof(value_t), hipMemcpyHostToDevice, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    return SGPU_OK;
}
int sgpu_vec_download(value_t *host, const value_t *dev, size_t n) {
    CHK(need_ctx());
    HIPCHK(hipStreamSynchronize(g.hs));
    HIPCHK(hipMemcpyAsync(host, dev, n * sizeof(value_t), hipMemcpyDeviceToHost, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    return SGPU_OK;
}
int sgpu_vec_fill(value_t *dev, value_t a, size_t n) {
    CHK(need_ctx());
    if (n == 0) return SGPU_OK;
    SGPU_LAUNCH(sk::k_fill, dim3(grid_for(n)), dim3(sk::BLOCK), 0, g.cs, dev, a, n);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}
int sgpu_vec_copy(value_t *dst, const value_t *src, size_t n) {
    CHK(need_ctx());
    HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(value_t), hipMemcpyDeviceToDevice, g.cs));
    return SGPU_OK;
}
int sgpu_vec_axpby(value_t a, const value_t *x, value_t b, value_t *y, size_t n) {
    CHK(need_ctx());
    if (n == 0) return SGPU_OK;
    SGPU_LAUNCH(sk::k_axpby, dim3(grid_for(n)), dim3(sk::BLOCK), 0, g.cs, a, x, b, y, n);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}
int sgpu_dot(const value_t *x, const value_t *y, size_t n, value_t *out) {
    CHK(need_ctx());
    CHK(dot_local_async(x, y, n, g.dscalar));
    if (g.comm) NCCLCHK(ncclAllReduce(g.dscalar, g.dscalar, 1, ncclDouble, ncclSum, g.comm, g.cs));
    HIPCHK(hipMemcpyAsync(g.hscalar, g.dscalar, sizeof(double), hipMemcpyDeviceToHost, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    if (g.xchg) CHK(host_allreduce(g.hscalar, 1));
    *out = g.hscalar[0];
    return SGPU_OK;
}
int sgpu_vec_center(const value_t *x, value_t *y, size_t n, value_t *mean_host) {
    CHK(need_ctx());
    if (!x || !y) return fail(SGPU_ERR_ARG, "sgpu_vec_center: null argument");
    if (g.nranks > 1) return fail(SGPU_ERR_ARG, "sgpu_vec_center: the mean is taken over this rank's rows; one rank only (this context has %d)", g.nranks);
    if (n == 0) { if (mean_host) *mean_host = 0.0; return SGPU_OK; }
    CHK(center_async(x, y, n));
    if (mean_host) {
        HIPCHK(hipMemcpyAsync(g.hscalar + CENTER_SLOT, g.dscalar + CENTER_SLOT, sizeof(double), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        *mean_host = g.hscalar[CENTER_SLOT] / (double)n;       // k_center's division
    }
    return SGPU_OK;
}

// ---- operators ----
int sgpu_op_create(const sgpu_op_desc *d, sgpu_op **out) {
    CHK(need_ctx());
    if (!d || !out) return fail(SGPU_ERR_ARG, "null descriptor");
    if (d->M < 0 || d->N_local < 0 || d->nnz_l_local < 0 || d->nnz_l_remote < 0) return fail(SGPU_ERR_ARG, "negative size");
    if (d->nnz_l_local >= INT32_MAX || d->nnz_l_remote >= INT32_MAX) return fail(SGPU_ERR_ARG, "local nnz must fit int32");
    if (d->M && !d->nnzPerRow_local) return fail(SGPU_ERR_ARG, "nnzPerRow_local is null");
    if (d->nnz_l_local && (!d->col_local || !d->val_local)) return fail(SGPU_ERR_ARG, "col_local/val_local is null");
    std::unique_ptr<sgpu_op> op(new sgpu_op());
    op->M = d->M; op->N_local = d->N_local; op->halo_fp32 = d->halo_fp32;

    // local part: prefix-sum row pointers, rebase columns (v_p = v - split[rank], saena_matrix_matvec.cpp:56)
    {
        std::vector<int> rp((size_t)d->M + 1, 0);
        for (index_t i = 0; i < d->M; ++i) {
            if (d->nnzPerRow_local[i] < 0) return fail(SGPU_ERR_ARG, "negative row length at row %d", i);
            rp[i + 1] = rp[i] + d->nnzPerRow_local[i];
        }
        if (rp[d->M] != d->nnz_l_local) return fail(SGPU_ERR_ARG, "sum(nnzPerRow_local)=%d != nnz_l_local=%ld", rp[d->M], (long)d->nnz_l_local);
        std::vector<int> col((size_t)d->nnz_l_local);
        // within a row the columns are distinct and ascend: build_xlds / k_xlds_build take a chunk's column range from each row's first
        // and last entry and cut a row at the windows' edges as it goes, build_dense stores one value per (row, column).  Checked in
        // the rebasing pass: a thread finds the row its first entry belongs to and walks the row ends from there; the lowest
        // offending row is named
        std::atomic<long> bad{-1}, bad_row{-1};
        saena_host::parallel_chunks<long>((long)d->nnz_l_local, 1L << 20, [&](int, long k0, long k1) {      // rebased on threads: 0.6 G entries per level at 16 M rows
            if (k0 >= k1) return;
            long r = (long)(std::upper_bound(rp.begin(), rp.end(), (int)k0) - rp.begin()) - 1;              // rp[r] <= k0 < rp[r + 1]
            long end = rp[(size_t)r + 1];
            long prev = k0 > rp[(size_t)r] ? (long)d->col_local[k0 - 1] - d->col_offset : -1;
            bool noted = false;
            for (long k = k0; k < k1; ++k) {
                if (k == end) { do ++r; while (rp[(size_t)r + 1] <= k); end = rp[(size_t)r + 1]; prev = -1; }
                const long c = (long)d->col_local[k] - d->col_offset;
                if (c < 0 || c >= d->N_local) { bad.store(k); return; }
                if (c <= prev && !noted) {
                    noted = true;
                    long seen = bad_row.load();
                    while ((seen < 0 || r < seen) && !bad_row.compare_exchange_weak(seen, r)) {}
                }
                prev = c;
                col[(size_t)k] = (int)c;
            }
        });
        if (bad.load() >= 0) return fail(SGPU_ERR_ARG, "col_local[%ld]=%d outside this rank's column block", bad.load(), d->col_local[bad.load()]);
        if (bad_row.load() >= 0) {
            const long r = bad_row.load();
            int k = rp[(size_t)r] + 1;
            while (col[(size_t)k] > col[(size_t)k - 1]) ++k;
            return fail(SGPU_ERR_ARG, "row %ld of col_local %s column %d at position %d of the row (col_local[%d]): within a row the columns must be distinct and ascending",
                        r, col[(size_t)k] == col[(size_t)k - 1] ? "repeats" : "steps back to", d->col_local[k], k - rp[(size_t)r], k);
        }
        const size_t nval = (size_t)d->nnz_l_local;
        auto host_copy = [&](std::vector<double> &dst) { dst.resize(nval); saena_host::parallel_copy(dst.data(), d->val_local, nval); };
        CHK(build_part(op->loc, std::move(rp), std::move(col), d->val_local, nval, nullptr));
        op->loc.ncols = d->N_local;
        // (whole operator: local + remote entries against the columns this rank reads, owned + halo)
        if (dense_candidate(d->M, d->N_local + d->col_remote_size, d->nnz_l_local + d->nnz_l_remote)) host_copy(op->loc.h_val);
        if (d->M <= sk::CG_MAXN) host_copy(op->h_val);
        // k_sellx (rows of 96-1024 entries) and the opt-in k_rowt are built from a host copy of the values at the plan-time autotune,
        // which drops the copy afterwards; every other form is made on the device from the CSR values there (round 4: the copy of the
        // 558 M-entry level alone was 4.5 GB to write and to unmap).  SAENA_KEEP_HOST_VALUES=1: keep it for good (development sweeps)
        const double avg_row = d->M > 0 ? (double)d->nnz_l_local / d->M : 0.0;
        if (std::getenv("SAENA_KEEP_HOST_VALUES") ||
            (!std::getenv("SAENA_NO_AUTOTUNE") && ((avg_row >= 96.0 && avg_row <= 1024.0) || (avg_row <= 768.0 && std::getenv("SAENA_ROW_TEMPLATES")))))
            host_copy(op->h_val_all);
    }
    // remote part: CSC over the receive buffer -> CSR over the halo buffer on the rows that own remote entries
    if (d->nnz_l_remote > 0) {
        if (!d->nnzPerCol_remote || !d->row_remote || !d->val_remote) return fail(SGPU_ERR_ARG, "remote arrays are null");
        std::vector<int> cnt((size_t)d->M, 0);
        nnz_t tot = 0;
        for (index_t j = 0; j < d->col_remote_size; ++j) tot += d->nnzPerCol_remote[j];
        if (tot != d->nnz_l_remote) return fail(SGPU_ERR_ARG, "sum(nnzPerCol_remote) != nnz_l_remote");
        for (nnz_t k = 0; k < d->nnz_l_remote; ++k) {
            if (d->row_remote[k] < 0 || d->row_remote[k] >= d->M) return fail(SGPU_ERR_ARG, "row_remote out of range");
            cnt[d->row_remote[k]]++;
        }
        std::vector<int> rows, slot((size_t)d->M, -1), rp(1, 0);
        for (index_t i = 0; i < d->M; ++i)
            if (cnt[i]) { slot[i] = (int)rows.size(); rows.push_back(i); rp.push_back(rp.back() + cnt[i]); }
        std::vector<int> fillp(rp.begin(), rp.end() - 1), col((size_t)d->nnz_l_remote);
        std::vector<double> val((size_t)d->nnz_l_remote);
        nnz_t k = 0;
        for (index_t j = 0; j < d->col_remote_size; ++j)
            for (index_t t = 0; t < d->nnzPerCol_remote[j]; ++t, ++k) {
                const int s = slot[d->row_remote[k]];
                // (a row twice inside one receive column: the remote CSR would add both, the dense form's remote part keep the last)
                if (fillp[s] > rp[(size_t)s] && col[fillp[s] - 1] == j)
                    return fail(SGPU_ERR_ARG, "row_remote[%ld]: row %d appears twice in receive column %d", (long)k, d->row_remote[k], j);
                col[fillp[s]] = j; val[fillp[s]] = d->val_remote[k]; fillp[s]++;
            }
        if (!op->loc.h_val.empty()) { op->rem.h_val = val; op->rem_rows_h = rows; }      // a dense form is still possible
        CHK(build_part(op->rem, std::move(rp), std::move(col), val.data(), val.size(), &rows));
        op->has_remote = true;
        // boundary rows: masked out of the interior launch, computed whole by k_csr_boundary
        std::vector<unsigned> mask(((size_t)d->M + 31) / 32, 0u);
        long len = d->nnz_l_remote;
        for (int r : rows) { mask[(size_t)r >> 5] |= 1u << (r & 31); len += d->nnzPerRow_local[r]; }
        CHK(dev_upload(op->skip, mask.data(), mask.size()));
        // lanes per boundary row: about one lane per entry (a G-lane group then reads its row as one coalesced
        // segment; one lane per 7-entry row made the launch 2.5x slower).  SAENA_BOUNDARY_LANES=1 restores the
        // reference's sequential per-row sum on these rows.
        const long avg = len / (long)rows.size();
        int gl = 1;
        while (gl < avg && gl < 64) gl *= 2;
        if (const char *bl = std::getenv("SAENA_BOUNDARY_LANES")) gl = std::max(1, std::min(64, pow2floor(std::atoi(bl))));
        op->bnd_lanes = gl;
    }
    if (d->inv_diag) CHK(dev_upload(op->inv_diag, d->inv_diag, (size_t)d->M));

    // halo plan
    op->vIndexSize = d->vIndexSize;
    op->recvSize   = d->col_remote_size;
    int sd = 0, rd = 0;
    if ((d->numSendProc > 0 && (!d->sendProcRank || !d->sendProcCount)) || (d->numRecvProc > 0 && (!d->recvProcRank || !d->recvProcCount)))
        return fail(SGPU_ERR_ARG, "send/recv plan arrays are null");
    for (int i = 0; i < d->numSendProc; ++i) {
        op->sendRank.push_back(d->sendProcRank[i]); op->sendCount.push_back(d->sendProcCount[i]); op->sendDispl.push_back(sd);
        sd += d->sendProcCount[i];
    }
    for (int i = 0; i < d->numRecvProc; ++i) {
        op->recvRank.push_back(d->recvProcRank[i]); op->recvCount.push_back(d->recvProcCount[i]); op->recvDispl.push_back(rd);
        rd += d->recvProcCount[i];
    }
    if (d->vIndexSize && !d->vIndex) return fail(SGPU_ERR_ARG, "vIndex is null");
    if (sd != d->vIndexSize) return fail(SGPU_ERR_ARG, "sum(sendProcCount)=%d != vIndexSize=%d", sd, d->vIndexSize);
    if (rd != d->col_remote_size) return fail(SGPU_ERR_ARG, "sum(recvProcCount)=%d != col_remote_size=%d", rd, d->col_remote_size);
    if (g.multi()) {   // (a context without a communicator may hold plans of a larger world for the single-GPU halo tests)
        const bool loopback = g.nranks == 1;        // one rank with a communicator: self send/recv, for RCCL path tests
        for (int r : op->sendRank) if (r < 0 || r >= g.nranks || (r == g.rank && !loopback)) return fail(SGPU_ERR_ARG, "bad send rank %d", r);
        for (int r : op->recvRank) if (r < 0 || r >= g.nranks || (r == g.rank && !loopback)) return fail(SGPU_ERR_ARG, "bad recv rank %d", r);
    }
    if (d->vIndexSize) {
        for (index_t i = 0; i < d->vIndexSize; ++i)
            if (d->vIndex[i] < 0 || d->vIndex[i] >= d->N_local) return fail(SGPU_ERR_ARG, "vIndex out of range");
        CHK(dev_upload(op->vIndex, d->vIndex, (size_t)d->vIndexSize));
        HIPCHK(op->send_buf.alloc((size_t)d->vIndexSize));
    }
    if (op->recvSize) {
        HIPCHK(op->recv_buf.alloc((size_t)op->recvSize));
        HIPCHK(hipMemsetAsync(op->recv_buf, 0, (size_t)op->recvSize * sizeof(double), g.cs));
    }
    if (op->halo_fp32 && g.multi()) {
        if (op->vIndexSize) HIPCHK(op->send_f.alloc((size_t)op->vIndexSize));
        if (op->recvSize) HIPCHK(op->recv_f.alloc((size_t)op->recvSize));
    }
    {   // Two streams pay when the interior kernel is long enough to hide part of the exchange chain behind.
        // SAENA_SINGLE_STREAM_NNZ overrides the nnz threshold (0: never).
        // Measured with RCCL self send/recv (profiles/r02_halo_loopback_modes.log): the GPU-side chain is ~23 us either
        // way, but the two-stream form takes 23-25 us of HOST time to enqueue against 15 us for the one-stream form, so
        // applies whose local kernel runs under ~5 us (< 1 M nnz) are host-bound on two streams (28 vs 25 us drained);
        // from ~10 us of local work on, the overlap wins (32 planes: 27 vs 31 us).
        // both thresholds were measured with a 23 us chain (RCCL self send/recv on one GPU); they scale with the chain this
        // job's communicator showed at init (calibrate_chain): a slower exchange moves both crossovers up
        const double scale = g.chain_us > 0.0 ? std::min(8.0, std::max(0.5, g.chain_us / 23.0)) : 1.0;
        long thr = (long)(1000.0 * 1000.0 * scale);
        if (const char *e = std::getenv("SAENA_SINGLE_STREAM_NNZ")) thr = std::atol(e);
        op->single_stream = (long)d->nnz_l_local < thr;
        long ev = (long)(30.0 * 1000 * 1000 * scale);   // 12 B x 30 M nnz / 5 TB/s = 72 us of interior work: the event-ordered chain (~48 us) hides behind it
        if (const char *e2 = std::getenv("SAENA_EVENT_SYNC_NNZ")) ev = std::atol(e2);
        op->events_only = (long)d->nnz_l_local >= ev;
    }
    // same-device dependencies only: no system-scope fence needed (saves ~2 us per hop, tools/hop_bench.hip)
    HIPCHK(hipEventCreateWithFlags(&op->ev_x, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK(hipEventCreateWithFlags(&op->ev_halo, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK(hipStreamSynchronize(g.cs));
    *out = op.release();
    return SGPU_OK;
}

int sgpu_op_destroy(sgpu_op *op) {
    if (!op) return SGPU_OK;
    if (g.live) hipDeviceSynchronize();
    delete op;
    return SGPU_OK;
}

int sgpu_op_info(const sgpu_op *op, index_t *M, index_t *N_local, nnz_t *nnz_local, nnz_t *nnz_remote, int *nblk, int *lanes) {
    if (!op) return fail(SGPU_ERR_ARG, "null op");
    if (M) *M = op->M;
    if (N_local) *N_local = op->N_local;
    if (nnz_local) *nnz_local = op->loc.nnz;
    if (nnz_remote) *nnz_remote = op->rem.nnz;
    if (nblk) *nblk = op->loc.nblk;
    if (lanes) *lanes = op->loc.lanes;
    return SGPU_OK;
}

int sgpu_op_set_lanes_per_row(sgpu_op *op, int lanes) {
    if (!op) return fail(SGPU_ERR_ARG, "null op");
    ++g_plan_generation;                                 // captured V-cycle graphs that launch this operator are stale now
    if (lanes == 0) { op->loc.lanes = auto_lanes(op->loc.nrows, op->loc.nblk); return SGPU_OK; }
    if (lanes < 1 || lanes > 64 || (lanes & (lanes - 1))) return fail(SGPU_ERR_ARG, "lanes_per_row must be a power of two in [1,64]");
    op->loc.lanes = lanes;
    return SGPU_OK;
}

// the workgroup sizes (256 << k rows) at which the autotune times the x-window mode of F_VIDX: 256 rows win on the cache-resident
// 128^3 fine level, 512 on the HBM-resident 256^3 one; 1024 won on neither and stays a setting of sgpu_op_set_x_windows
static const int XWIN_CANDIDATES[] = {0, 1};

extern "C++" {
namespace {
// the form's base name, decorated from the part's flags: the slot/offset split of the compressed columns ("k_csr_cc16<32KiB,5+11>"),
// <wide> (a pattern table per workgroup), <rowbase> (patterns relative to the row's first column), <sorted> (slices sorted by length)
std::string form_name(const CsrPart &P) {
    const int f = P.variant;
    std::string n = FORM_NAMES[f];
    if (is_cc16(f) || is_column_major(f)) {
        const int ob = P.cc_ob[tile_plan(f)];
        n.pop_back();
        n += "," + std::to_string(16 - ob) + "+" + std::to_string(ob) + ">";
    }
    const bool wide = (f == F_SELLP || f == F_SELLP2) && P.sp.sp_wide, rbase = (f == F_SELLP || f == F_VIDX) && P.sp.sp_rbase;
    if (wide || rbase) n += std::string("<") + (wide ? "wide" : "") + (wide && rbase ? "," : "") + (rbase ? "rowbase" : "") + ">";
    if (f == F_SELL && P.sv.sl_sorted) n += "<sorted>";
    return n;
}

// Build what `form` launches from: its prerequisite builders in order.  Every builder opens with its own tried / ok guard, so a
// second call builds nothing.  *ok: the form can run on this operator (the dense form reports through the builder's own error).
int build_form(sgpu_op *op, int form, bool *ok) {
    CsrPart &L = op->loc;
    *ok = true;
    switch (form) {
    case F_CC16_16: case F_CC16_32: CHK(build_cc16(L, tile_plan(form))); *ok = L.cc[tile_plan(form)].ok; break;
    case F_DENSE:   CHK(build_dense(L)); CHK(build_dense_rem(op)); break;
    case F_CM16: case F_CM32: CHK(build_cm(L, tile_plan(form), op->h_val_all)); *ok = L.cm[tile_plan(form)].ok; break;
    case F_SELL:    CHK(build_sell(L, op->h_val_all)); *ok = L.sl_ok; break;
    case F_XLDS: case F_XLDSR: CHK(build_xlds(L)); *ok = L.xlp.xl_ok; break;
    case F_SELLP:   CHK(build_sell_values(L)); CHK(build_sellp(L)); *ok = L.sp.sp_ok; break;
    case F_SELLX:   CHK(build_xlds(L)); CHK(build_sellx(L, op->h_val_all)); *ok = L.sx.sx_ok; break;
    case F_ROWT:    CHK(build_rowt(L, op->h_val_all)); *ok = L.rt.rt_ok; break;
    case F_SELLP2:  CHK(build_sell_values(L)); CHK(build_sellp(L)); CHK(build_sellp2(L, op->h_val_all)); *ok = L.sp2.sp2_ok; break;
    case F_SELLPX:  CHK(build_sell_values(L)); CHK(build_sellp(L)); CHK(build_sellpx(L)); *ok = L.spx.spx_ok; break;
    case F_VIDX:    CHK(build_sell_values(L)); CHK(build_sellp(L)); CHK(build_vidx(L)); *ok = L.vi.vi_ok; break;
    default: break;                                      // F_STREAM16, F_STREAM32, F_VECTOR, F_WAVE: the CSR arrays as they are
    }
    return SGPU_OK;
}

// why build_form left `form` without its ok
int refuse_form(int form) {
    switch (form) {
    case F_CC16_16: case F_CC16_32:
        return fail(SGPU_ERR_ARG, "a row block of this operator touches more than 256 column segments of 256 columns");
    case F_CM16: case F_CM32:
        return fail(SGPU_ERR_ARG, "the column-major form needs compressed columns, no row longer than the tile and the host copy of the values "
                                  "(kept until the plan-time autotune, or with SAENA_KEEP_HOST_VALUES=1)");
    case F_SELL:
        return fail(SGPU_ERR_ARG, "the sliced-ELLPACK form needs even rows (padding <= 12 %%), 16-bit column codes (<= 256 segments per 256 rows) and "
                                  "the host copy of the values (kept until the plan-time autotune, or with SAENA_KEEP_HOST_VALUES=1)");
    case F_XLDS: case F_XLDSR:
        return fail(SGPU_ERR_ARG, "the x-in-LDS form needs row chunks (one per CU) that reach over at most %d columns", sk::XL_MAXT * sk::XL_MAX);
    case F_SELLP:
        return fail(SGPU_ERR_ARG, "the row-pattern form needs what the sliced-ELLPACK form needs and rows that follow at most %d-int's worth of "
                                  "(length, relative columns) patterns per group of %d rows", sk::SPW_MAX_TABLE, sk::SPW_BLOCK);
    case F_SELLX:
        return fail(SGPU_ERR_ARG, "the sliced-ELLPACK-in-LDS form needs the x-in-LDS plan (row chunks over at most %d column windows), at most 25 %% padding "
                                  "and the host copy of the values (kept until the plan-time autotune, or with SAENA_KEEP_HOST_VALUES=1)", sk::XL_MAXT);
    case F_ROWT:
        return fail(SGPU_ERR_ARG, "the row-template form needs rows that repeat at most %d bytes' worth of (length, relative columns, values) templates "
                                  "and the host copy of the values (kept until the plan-time autotune, or with SAENA_KEEP_HOST_VALUES=1)", RT_MAX_BYTES);
    case F_SELLP2:
        return fail(SGPU_ERR_ARG, "the row-paired row-pattern form needs what the row-pattern form needs (k_sellp) and the host copy of the values");
    case F_SELLPX:
        return fail(SGPU_ERR_ARG, "the row-pattern form with x in LDS needs what the row-pattern form needs (k_sellp) and pattern offsets that fall into at most %d "
                                  "windows of x which fit %d KiB of LDS together with the table", sk::SPX_MAXWIN, sk::SPX_LDS_BYTES / 1024);
    case F_VIDX:
        return fail(SGPU_ERR_ARG, "the value-indexed row-pattern form needs what the row-pattern form needs (k_sellp) with ONE pattern table, and at most %d "
                                  "distinct values (as bit patterns) in every group of %d rows", sk::VI_MAX, sk::BLOCK);
    }
    return fail(SGPU_ERR_STATE, "form %d was not built", form);
}
} // namespace
} // extern "C++"

int sgpu_op_get_variant(const sgpu_op *op, int *variant, const char **kernel_name) {
    if (!op) return fail(SGPU_ERR_ARG, "null op");
    if (variant) *variant = op->loc.variant;
    if (kernel_name) {
        const_cast<sgpu_op *>(op)->vname = form_name(op->loc);
        *kernel_name = op->vname.c_str();
    }
    return SGPU_OK;
}

int sgpu_op_set_variant(sgpu_op *op, int variant) {
    if (!op) return fail(SGPU_ERR_ARG, "null op");
    if (variant < 0 || variant >= F_COUNT) return fail(SGPU_ERR_ARG, "variant must be 0..%d", F_COUNT - 1);
    bool ok = false;
    CHK(build_form(op, variant, &ok));
    if (!ok) return refuse_form(variant);
    op->loc.variant = variant;
    op->loc.vw_rows = 0;                                 // F_VIDX alone gathers directly; sgpu_op_set_x_windows turns the windows on
    op->loc.vw_last = -1; op->loc.vw_last_width = -1; op->loc.vw_last_rows = -1;
    ++g_plan_generation;
    if (variant == F_VIDX)
        if (const char *e = std::getenv("SAENA_X_WINDOWS")) {     // development: pin the mode where only the variant can be pinned (counter passes); refused -> direct
            const int rows = std::atoi(e), k = xwin_slot(rows);
            if (k >= 0) {
                CHK(build_xwin(op->loc, k));
                if (op->loc.vw[k].ok) op->loc.vw_rows = rows;
            }
        }
    return SGPU_OK;
}

int sgpu_op_set_x_windows(sgpu_op *op, int rows_per_workgroup) {
    CHK(need_ctx());
    if (!op) return fail(SGPU_ERR_ARG, "null op");
    const int R = rows_per_workgroup;
    op->loc.vw_last = -1; op->loc.vw_last_width = -1; op->loc.vw_last_rows = -1;
    if (R == 0) { op->loc.vw_rows = 0; ++g_plan_generation; return SGPU_OK; }
    const int k = xwin_slot(R);
    if (k < 0) return fail(SGPU_ERR_ARG, "x windows: rows per workgroup must be 0 (off), 256, 512 or 1024");
    if (op->loc.variant != F_VIDX) return fail(SGPU_ERR_ARG, "x windows are a launch mode of the value-indexed form: set variant 17 first");
    std::string why;
    CHK(build_xwin(op->loc, k, &why));
    if (!op->loc.vw[k].ok)
        return fail(SGPU_ERR_ARG, "x windows refused for workgroups of %d rows (%s): the mode needs ONE pattern table relative to the row index, at most %d windows, "
                                  "16-bit LDS positions and %d KiB of LDS for windows, dictionaries and table; the operator keeps its direct gathers",
                    R, why.c_str(), sk::SPX_MAXWIN, sk::VW_MAX_LDS / 1024);
    op->loc.vw_rows = R;
    ++g_plan_generation;
    return SGPU_OK;
}

int sgpu_op_get_x_windows(const sgpu_op *op, int *rows_per_workgroup) {
    if (!op || !rows_per_workgroup) return fail(SGPU_ERR_ARG, "null argument");
    *rows_per_workgroup = op->loc.variant == F_VIDX ? op->loc.vw_rows : 0;
    return SGPU_OK;
}

int sgpu_op_get_x_window_kernel(const sgpu_op *op, int *kernel) {
    if (!op || !kernel) return fail(SGPU_ERR_ARG, "null argument");
    const CsrPart &P = op->loc;
    const int k = P.variant == F_VIDX ? xwin_slot(P.vw_rows) : -1;
    *kernel = k < 0 ? 0 : P.vw_last >= 0 ? P.vw_last : P.vw[k].plan.fast_kind;
    return SGPU_OK;
}

// bits per entry of the code stream the last launch of variant 17 read: 1 where k_vidxw_fast ran on the bit codes (vw_fast.h), 8
// for k_vidx, k_vidxw and k_vidxw_fast on the byte codes; before a launch: what a launch without a halo would read; 0: not variant 17
int sgpu_op_get_x_window_code_width(const sgpu_op *op, int *bits_per_entry) {
    if (!op || !bits_per_entry) return fail(SGPU_ERR_ARG, "null argument");
    const CsrPart &P = op->loc;
    const int k = P.variant == F_VIDX ? xwin_slot(P.vw_rows) : -1;
    *bits_per_entry = P.variant != F_VIDX ? 0 : k < 0 ? 8 : P.vw_last_width >= 0 ? P.vw_last_width : vwfast::code_width(P.vw[k].plan.fast_kind == 2 && P.vw[k].bits);
    return SGPU_OK;
}

// the row format of the last launch of variant 17 in the x-window mode: 1 where k_vidxw_fast read its rows as lane masks
// (vw_masks.h), 0 where the rows went through the pattern table; before a launch: what a launch without a halo would read
int sgpu_op_get_x_window_row_format(const sgpu_op *op, int *format) {
    if (!op || !format) return fail(SGPU_ERR_ARG, "null argument");
    const CsrPart &P = op->loc;
    const int k = P.variant == F_VIDX ? xwin_slot(P.vw_rows) : -1;
    *format = k < 0 ? 0 : P.vw_last_rows >= 0 ? P.vw_last_rows : (P.vw[k].plan.fast_kind == 2 && P.vw[k].bits && P.vw[k].masks) ? 1 : 0;
    return SGPU_OK;
}

// ---- plan cache: what the autotune chose for an operator of this shape on this device, so that a second process picks the
// same kernel (same summation order: bit-identical solves across processes) and skips the sweep.  One line per operator in
// $SAENA_PLAN_CACHE, default $XDG_CACHE_HOME or ~/.cache + /saena_amd/plans-v5.tsv (v3: round 4 added candidate forms, v4: the value-indexed form, v5: its x-window mode, a field of its own -- plans an older library cached must not shadow them); SAENA_PLAN_CACHE=off disables it.
extern "C++" {                                              // (helpers with C++ types inside the extern "C" block)
namespace {
uint64_t fnv1a(uint64_t h, const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ULL; }
    return h;
}
std::string plan_cache_path() {
    if (const char *e = std::getenv("SAENA_PLAN_CACHE")) {
        const std::string v(e);
        return (v.empty() || v == "off" || v == "0") ? std::string() : v;
    }
    std::string dir;
    if (const char *x = std::getenv("XDG_CACHE_HOME")) dir = x;
    else if (const char *h = std::getenv("HOME")) dir = std::string(h) + "/.cache";
    if (dir.empty()) return std::string();
    ::mkdir(dir.c_str(), 0755);
    dir += "/saena_amd";
    ::mkdir(dir.c_str(), 0755);
    return dir + "/plans-v5.tsv";
}
// key: device, sizes, what the kernel does (smoother epilogue or plain product, halo mask), the row-length histogram in
// powers of two and the column ids at 256 evenly spaced entries
uint64_t plan_key(const sgpu_op *op) {
    uint64_t h = 1469598103934665603ULL;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, g.device) == hipSuccess) {
        h = fnv1a(h, pr.gcnArchName, strnlen(pr.gcnArchName, sizeof pr.gcnArchName));
        h = fnv1a(h, &pr.multiProcessorCount, sizeof(int));
    }
    const CsrPart &P = op->loc;
    const int64_t dims[6] = {op->M, op->N_local, P.nnz, op->inv_diag ? 1 : 0, op->has_remote ? 1 : 0, (int64_t)op->rem.nnz};
    h = fnv1a(h, dims, sizeof dims);
    int64_t hist[34] = {0};
    for (int r = 0; r < P.nrows; ++r) {
        const int n = P.h_rp[(size_t)r + 1] - P.h_rp[(size_t)r];
        int b = 0;
        while ((1 << b) <= n && b < 32) ++b;
        hist[b]++;
    }
    h = fnv1a(h, hist, sizeof hist);
    const size_t nn = P.h_col.size();
    for (int i = 0; i < 256 && nn; ++i) { const int c = P.h_col[(size_t)((double)i / 256.0 * (double)nn)]; h = fnv1a(h, &c, sizeof c); }
    return h;
}
bool plan_cache_lookup(uint64_t key, int *v, int *lanes, int *xw) {
    const std::string path = plan_cache_path();
    if (path.empty()) return false;
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return false;
    char line[256];
    bool hit = false;
    while (fgets(line, sizeof line, f)) {               // the last line of a key wins
        unsigned long long k; int vv, ll, xx;
        if (sscanf(line, "%llx %d %d %d", &k, &vv, &ll, &xx) == 4 && k == key && plan_line_valid(vv, ll, xx)) { *v = vv; *lanes = ll; *xw = xx; hit = true; }
    }
    fclose(f);
    return hit;
}
// the runner-up as the log and the cache line's comment show it: "lanes" of an x-window candidate are its rows per workgroup
int shown_lanes(const Candidate &c) { return c.xwin_rows ? c.xwin_rows : c.lanes; }
void plan_cache_store(uint64_t key, const sgpu_op *op, const Candidate &c, float ms, const Candidate &ru, float rms) {     // (ru.form < 0: no runner-up)
    const std::string path = plan_cache_path();
    if (path.empty()) return;
    char line[256];
    int n = snprintf(line, sizeof line, "%016llx\t%d\t%d\t%d\t%.4f\t# %d rows %lld nnz", (unsigned long long)key, c.form, c.lanes, c.xwin_rows, ms, op->M, (long long)op->loc.nnz);
    if (ru.form >= 0) n += snprintf(line + n, sizeof line - (size_t)n, "; %s %.4f ms; runner-up %s with %d lanes %.4f ms", FORM_NAMES[c.form], ms, FORM_NAMES[ru.form], shown_lanes(ru), rms);   // (the lookup reads the first four fields: variant, lanes, x-window rows)
    n += snprintf(line + n, sizeof line - (size_t)n, "\n");
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_APPEND, 0644);    // one write() of one short line: appends of concurrent ranks do not interleave
    if (fd < 0) return;
    if (::write(fd, line, (size_t)n) != n) { /* a cache: best effort */ }
    ::close(fd);
}
// drop what the chosen plan does not need: alternative forms on the device (every group plan_keeps() does not name), the host copy
// of the values
void finish_plan(sgpu_op *op, int bv) {
    CsrPart &L = op->loc;
    if (!plan_keeps(G_DENSE, bv, 0)) L.dn = {};
    if (std::getenv("SAENA_KEEP_HOST_VALUES")) return;             // development sweeps switch variants after the autotune
    auto drop = [&](int grp) { return !plan_keeps(grp, bv, L.vw_rows); };
    for (int k = 0; k < 2; ++k) {                                  // (a plan whose build was refused keeps its `tried` mark)
        if (L.cm[k].ok && drop(G_CM0 + k)) L.cm[k] = {};
        if (L.cc[k].ok && drop(G_CC0 + k)) L.cc[k] = {};
    }
    if (drop(G_SELL_VALUES)) L.sv = {};                            // (a later set_variant(11) re-orders the values again, from the device's CSR copy)
    if (drop(G_SELL_COLUMNS)) {
        L.sc = {};
        L.sl_ok = false;                                           // variant 9 is gone for good (sl_tried stays set) while a row-pattern form
        if (drop(G_SELLP)) L.sl_tried = 0;                         // lives on; with the whole family gone it may be built again
    }
    if (drop(G_SELLP)) L.sp = {};
    for (int k = 0; k < 3; ++k) if (drop(G_XWIN0 + k)) L.vw[k] = {};      // (variant 17 keeps the tables of the workgroup size in use only)
    if (drop(G_VIDX)) { L.vi = {}; L.vw_rows = 0; }
    if (drop(G_SELLP2)) L.sp2 = {};
    if (drop(G_SELLPX)) L.spx = {};
    if (drop(G_ROWT)) L.rt = {};
    if (drop(G_SELLX)) L.sx = {};
    if (drop(G_XLDS_PLAN)) L.xlp = {};
    if (drop(G_XLDS_COLUMNS)) L.xlc = {};                          // (k_sellx keeps the chunk plan only: xl_ok stays, launch_part refuses 10 / 16 on the missing columns)
    std::vector<int>().swap(L.h_pstart); std::vector<int>().swap(L.h_ptab); std::vector<unsigned short>().swap(L.h_pat);
    // the host copy of the values goes (the forms that still need it -- k_sellx, k_rowt -- are refused from here on).  Unmapping 4.5 GB
    // of resident host memory takes 0.25 s (the 558 M-entry level: most of what the autotune's log called "freeing"): a detached
    // thread does it, like the host setup's own large temporaries
    if (!op->h_val_all.empty()) {
        if (op->h_val_all.size() >= ((size_t)1 << 22) && !std::getenv("SAENA_NO_ASYNC_FREE")) {
            auto *junk = new std::vector<double>(std::move(op->h_val_all));
            try { std::thread([junk] { delete junk; }).detach(); } catch (...) { delete junk; }       // (no thread to be had: free it here)
        }
        std::vector<double>().swap(op->h_val_all);
    }
}
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
} // namespace
} // extern "C++"

// Plan-time autotune of the local kernel: time the (variant, lanes) candidates that the operator's row lengths leave in
// play on the operator itself and keep the fastest.  Summation order inside a row depends on the choice, so results may
// differ at rounding level between choices (never between runs of one choice); therefore
//   * candidates within 3 % of the fastest are ranked by a fixed order -- forms with the reference's sequential row sum
//     first, then by (variant, lanes) -- so that noise between near-equal kernels does not move the choice;
//   * the choice is written to the plan cache and a later process (same device, same operator shape) takes it from there.
// Cost: forms that the row lengths rule out are not built (each build is a pass over the entries on the host plus an
// upload), and after a first short round only candidates within 30 % of the best are timed again.
int sgpu_op_autotune(sgpu_op *op) {
    CHK(need_ctx());
    if (!op) return fail(SGPU_ERR_ARG, "null op");
    if (op->loc.nnz < 200000) { finish_plan(op, op->loc.variant); return SGPU_OK; }          // launch-latency territory: keep the heuristic
    const bool verbose = std::getenv("SAENA_SETUP_TIMING") != nullptr;
    const double t_begin = now_s();
    const uint64_t key = plan_key(op);
    {
        int cv = 0, cl = 1, cx = 0;
        if (plan_cache_lookup(key, &cv, &cl, &cx) && sgpu_op_set_variant(op, cv) == SGPU_OK && (cx == 0 || sgpu_op_set_x_windows(op, cx) == SGPU_OK)) {
            op->loc.lanes = cl;
            ++g_plan_generation;
            finish_plan(op, cv);
            if (verbose) fprintf(stderr, "[sgpu] plan of %d rows x %lld nnz from the cache: variant %d, %d lanes, x windows %d (%.3f s)\n", op->M, (long long)op->loc.nnz, cv, cl, op->loc.vw_rows, now_s() - t_begin);
            return SGPU_OK;
        }
    }
    const int g0 = auto_lanes(op->loc.nrows, op->loc.nblk);
    std::vector<int> lanes;
    for (int g : {g0 / 2, g0, g0 * 2}) if (g >= 1 && g <= 64) lanes.push_back(g);
    DevArr<double> x, y, r;
    CHK(dev_alloc(x, op->N_local)); CHK(dev_alloc(y, op->M)); CHK(dev_alloc(r, op->M));
    CHK(sgpu_vec_fill(x, 1.0, op->N_local)); CHK(sgpu_vec_fill(r, 1.0, op->M));
    const int kind = op->inv_diag ? 1 : 0;
    const double avg_row = (double)op->loc.nnz / std::max(1, op->loc.nrows);
    const bool all = std::getenv("SAENA_AUTOTUNE_ALL") != nullptr;     // every form that applies, as before round 3 (development)
    // which forms are worth building, by row length (profiles/r02_perf_levels_256_*.log: what won where):
    //   rows of up to ~128 entries with even lengths -- sliced ELLPACK (with or without a column stream) or 16-bit columns on
    //   16 KiB tiles; a few hundred entries -- column order inside 32 KiB tiles, 16-bit columns on either tile; a thousand and
    //   more -- x in LDS, the wave-streamed kernel, 16-bit or 32-bit columns on tiles
    std::vector<int> variants, xwin_rows;
    bool sell_like = false, ok = false;
    if (!std::getenv("SAENA_NO_SELL") && (all || avg_row <= 160.0)) {                                 // even rows: a lane per row
        CHK(build_sell_values(op->loc));                                                             // (on the device, from the CSR values: round 4)
        if (op->loc.sv.sl_vals) {
            if (!std::getenv("SAENA_NO_SELLP")) {                                                    // rows that repeat a few patterns: no column stream
                CHK(build_form(op, F_SELLP, &ok));
                if (ok) variants.push_back(F_SELLP);
                // ... and the values as 8-bit codes into a dictionary per workgroup (operators of at most VI_MAX distinct values per
                // 256 rows: the constant-coefficient stencil levels and their transfers): 1 B per entry instead of 8.  Offered where the
                // values are more than the eight XCDs' L2 (32 MiB) hold from one launch to the next -- the bytes it saves come from the
                // Infinity Cache or HBM; below that it was not measured and the plan stays as it was (128^3 fine level: 111 MB)
                if (op->loc.sp.sp_ok && !op->loc.sp.sp_wide && 8 * op->loc.nnz > ((int64_t)32 << 20) && !std::getenv("SAENA_NO_VALUE_INDEX")) {
                    CHK(build_form(op, F_VIDX, &ok));
                    if (ok) variants.push_back(F_VIDX);
                    // ... and the same form with x in LDS windows (k_vidxw), a candidate of its own per workgroup size kept
                    if (ok && !std::getenv("SAENA_NO_X_WINDOWS"))
                        for (int k : XWIN_CANDIDATES) { CHK(build_xwin(op->loc, k)); if (op->loc.vw[k].ok) xwin_rows.push_back(256 << k); }
                }
                // ... and a lane per two rows: half the gathers.  With a table per workgroup (sp_wide: the 68-entry level) it wins on the
                // operator of 128^3 (110 against 116 us, k_sellpx 114) and ties on that of 256^3 (940 / 945, k_sellpx 890), whose row-paired
                // copy is 4.5 GB: tried up to 1 GB (profiles/r03_sellp_pergroup_tables.log).  (Round 4: the device makes the copy in
                // milliseconds, but allocating and FREEING 4.5 GB costs 0.2 s of the plan and the form lost again on 256^3 -- 942 against
                // k_sellpx's 888 us: the limit stays)
                if (op->loc.sp.sp_ok && (!op->loc.sp.sp_wide || op->loc.sp_bytes <= ((int64_t)1 << 30)) && !std::getenv("SAENA_NO_SELLP2")) {
                    CHK(build_form(op, F_SELLP2, &ok));
                    if (ok) variants.push_back(F_SELLP2);
                }
                if (op->loc.sp.sp_ok && avg_row >= 16.0 && !std::getenv("SAENA_NO_SELLPX")) {                 // ... with x in LDS windows: where a row gathers dozens of entries
                    CHK(build_form(op, F_SELLPX, &ok));
                    if (ok) variants.push_back(F_SELLPX);
                }
                if (op->loc.sp.sp_ok && std::getenv("SAENA_ROW_TEMPLATES") && !op->h_val_all.empty()) {     // OPT-IN: rows that also repeat their values
                    CHK(build_form(op, F_ROWT, &ok));
                    if (ok) variants.push_back(F_ROWT);
                }
            }
            // k_sell itself (10 B per entry: the same values + 16-bit column codes, which cost a host pass over the entries and 2 B per
            // entry of upload) only where the rows follow no patterns -- it never beat k_sellp on an operator that has them (8 B per
            // entry, the same structure: 128^3 level 1 137.8 against 119.3 us, profiles/r03_sellp_wide_l1_128.log)
            if (!op->loc.sp.sp_ok || op->loc.sp.sp_rbase || all) {             // (... and next to a rowbase table: the 4 B per row it adds are a fifth of what the codes cost on 6-entry rows)
                CHK(build_form(op, F_SELL, &ok));
                if (ok) variants.push_back(F_SELL);
            }
            sell_like = op->loc.sp.sp_ok || (op->loc.sl_ok && !op->loc.sv.sl_sorted);         // (sorted slices: one more candidate next to the tile kernels)
        }
    }
    const double t_sell = now_s();
    const bool short_rows = sell_like && avg_row <= 128.0 && !all;
    for (int f : {F_CC16_16, F_CC16_32}) {
        // (round 4) an operator whose rows follow patterns runs at 8 B per entry; the tile kernels' 10 B per entry never came within 15 % of
        // it (256^3 L0 343 against 277 us, L1 1 190-1 270 against 890): not built, not timed, not freed
        if (op->loc.sp.sp_ok && !all) continue;
        if (f == F_CC16_32 && (short_rows || avg_row < 16.0) && !all) continue;                              // 32 KiB tiles never won on the shortest rows (at 18 entries per
                                                                                                     // row -- P1 of 256^3 -- they do: 361 against 385 us, profiles/r03_transfers_sell_padding.log)
        CHK(build_form(op, f, &ok));
        if (ok) variants.push_back(f);
    }
    const double t_cc = now_s();
    if (!short_rows) {
        if (!op->loc.cc[0].ok || avg_row >= 256.0 || all) variants.push_back(F_STREAM16);                   // 32-bit columns: where 16-bit ones do not apply, and on long rows
        if (!op->loc.cc[1].ok || avg_row >= 256.0 || all) variants.push_back(F_STREAM32);
    }
    variants.push_back(F_VECTOR);                                                                // vector CSR: no build
    if (op->loc.nnz >= 256 * (int64_t)std::max(1, op->loc.nrows)) variants.push_back(F_WAVE);        // long rows: the wave-streamed kernel
    // x in LDS: long rows over few columns; and (round 4) IRREGULAR operators of a few dozen entries per row -- no sliced-ELLPACK form
    // (uneven rows), random columns inside a window: the tile kernels' gathers are what bounds them (configs[4] at 1 M rows: 134 us
    // against 111 us with x in LDS, 4 rows per group step below that)
    const bool irregular_short = !sell_like && avg_row >= 12.0;
    if ((op->loc.nnz >= 48 * (int64_t)std::max(1, op->loc.nrows) || irregular_short) && !std::getenv("SAENA_NO_XLDS") && (!short_rows)) {
        CHK(build_form(op, F_XLDS, &ok));
        if (ok && op->loc.xl_piece >= 24.0) variants.push_back(F_XLDS);
        if (ok && op->loc.xl_piece >= 8.0 && op->loc.xl_piece < 160.0 && !std::getenv("SAENA_NO_XLDSR")) variants.push_back(F_XLDSR);   // short pieces: four rows per group step
    }
    // (on the transfers it does not pay: P1 of 256^3, 18 entries per row, 504 us against 350; P2 ties; R2 165 against 156 us,
    //  profiles/r03_sellx_steps.log)
    if (op->loc.xlp.xl_ok && !op->h_val_all.empty() && avg_row >= 96.0 && avg_row <= 1024.0 && !std::getenv("SAENA_NO_SELLX")) {
        CHK(build_form(op, F_SELLX, &ok));                                                           // a few hundred entries per row: a lane per row piece, x in LDS
        if (ok) variants.push_back(F_SELLX);
    }
    const double t_xl = now_s();
    // (k_csr_cm, 12 B per entry, is built further down -- only where the candidates timed so far leave it a chance)
    const double t_cm = now_s();      // (the builds end here; k_csr_cm's is timed separately below)
    if (!op->has_remote && !op->loc.h_val.empty() && (double)op->loc.nnz >= 0.5 * (double)op->loc.nrows * op->loc.ncols && build_form(op, F_DENSE, &ok) == SGPU_OK)
        variants.push_back(F_DENSE);                        // at least half full: the dense form moves fewer bytes
    // Only the LOCAL part is timed, without the halo exchange: ranks may end up with different candidate
    // lists (a rank's blocks may be too scattered for 16-bit columns), so no collective may run in here.
    EpiArgs e; e.rhs = r; e.inv_diag = op->inv_diag; e.u = x; e.c0 = JACOBI_OMEGA_REF;
    const int epi = kind == 1 ? sk::EPI_JACOBI : sk::EPI_SPMV;
    ++g_plan_generation;                                 // frees/replaces buffers captured graphs may reference
    struct Guard {                                       // an error return inside the sweep leaves the operator as it was
        sgpu_op *op; int v, l, xw; hipEvent_t e0 = nullptr, e1 = nullptr; bool armed = true;
        ~Guard() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); if (armed) { op->loc.variant = v; op->loc.lanes = l; op->loc.vw_rows = xw; } }
    } guard{op, op->loc.variant, op->loc.lanes, op->loc.vw_rows};
    HIPCHK(hipEventCreate(&guard.e0)); HIPCHK(hipEventCreate(&guard.e1));
    const hipEvent_t e0 = guard.e0, e1 = guard.e1;
    std::vector<int> lanes_x;                            // k_csr_xlds: lanes per (row, window) piece, about a 64th of its length
    {
        const int gx = std::min(64, std::max(4, pow2floor((int)std::max(1.0, op->loc.xl_piece / 64.0))));
        for (int g : {gx / 2, gx, gx * 2}) if (g >= 4 && g <= 64) lanes_x.push_back(g);
    }
    const std::vector<int> lanes_r = {8, 16, 32};         // k_csr_xldsr: lanes per group of four rows
    std::vector<Candidate> cands;
    for (int v : variants)
        for (int gl : (v == F_XLDS ? lanes_x : v == F_XLDSR ? lanes_r : lanes)) {
            if (one_candidate(v) && gl != lanes.front()) continue;         // a lane per row (piece), a wave per dense row: whatever the setting
            cands.push_back({v, gl, 0});
        }
    for (int rows : xwin_rows) cands.push_back({F_VIDX, lanes.front(), rows});
    {                                                    // a few milliseconds of the current plan first: a process's first kernels run at ramping clocks
        float ms = 0;
        for (int burst = 0; burst < 8 && ms < 2.0f; ++burst) {
            HIPCHK(hipEventRecord(e0, g.cs));
            for (int i = 0; i < 8; ++i) CHK(launch_part(op->loc, epi, x, y, e));
            HIPCHK(hipEventRecord(e1, g.cs));
            HIPCHK(hipEventSynchronize(e1));
            float t = 0;
            HIPCHK(hipEventElapsedTime(&t, e0, e1));
            ms += t;
        }
    }
    auto sample = [&](const Candidate &c, int reps, float *ms) -> int {
        op->loc.variant = c.form; op->loc.lanes = c.lanes; op->loc.vw_rows = c.xwin_rows;
        HIPCHK(hipEventRecord(e0, g.cs));
        for (int i = 0; i < reps; ++i) CHK(launch_part(op->loc, epi, x, y, e));
        HIPCHK(hipEventRecord(e1, g.cs));
        HIPCHK(hipEventSynchronize(e1));
        HIPCHK(hipEventElapsedTime(ms, e0, e1));
        *ms /= reps;
        return SGPU_OK;
    };
    // round 0 warms up (clocks, caches, code objects) and estimates; round 1 measures the candidates within 30 % of the best
    // estimate (>= 1 ms each); the deciding rounds then time the ones within 8 % of the fastest three more times, interleaved, >= 2 ms
    // each, every candidate keeping its best time: single 1 ms samples picked losers now and then
    std::map<Candidate, float> est, seen;
    float best_est = 1e30f;
    for (const auto &c : cands) { float ms = 0; CHK(sample(c, 2, &ms)); est[c] = ms; best_est = std::min(best_est, ms); }
    // rows of a few hundred entries: column order inside the block (k_csr_cm) -- a host pass over the entries and a 12 B per entry upload
    // (0.6-0.9 s on the 150-200 M entry operators of 256^3).  Its best rate anywhere was 5.0 TB/s of stored bytes (256^3 L2), so it is
    // built only where the forms timed so far are slower than its bytes at 5.2 TB/s (R1 of 256^3: 438 us against a bound of 351 -> built,
    // wins with 384; L2: k_sellx 440 against 459 -> skipped, it measured 493)
    const double t_cm0 = now_s();
    if (avg_row >= 96.0 && avg_row <= 768.0 && !std::getenv("SAENA_NO_CM") &&
        (all || (double)best_est > 12.0 * (double)op->loc.nnz / 5.2e9)) {
        CHK(build_form(op, F_CM32, &ok));
        if (ok)
            for (int gl : lanes) {
                const Candidate c{F_CM32, gl, 0};
                float ms = 0;
                CHK(sample(c, 3, &ms));
                cands.push_back(c); est[c] = ms; best_est = std::min(best_est, ms);
            }
    }
    const double t_cm1 = now_s();
    for (int round = 1; round < 2; ++round)               // (ONE measuring round since round 4: the deciding rounds below re-time whatever is close)
        for (const auto &c : cands) {
            if (est[c] > 1.3f * best_est && !all) continue;
            const int reps = std::min(48, std::max(3, (int)(1.0f / std::max(est[c], 1e-3f)) + 1));   // a measuring sample lasts >= 1 ms
            float ms = 0;
            CHK(sample(c, reps, &ms));
            auto it = seen.find(c);
            if (it == seen.end()) seen[c] = ms; else it->second = std::min(it->second, ms);
        }
    // The deciding rounds (round 4): the candidates within 8 % of the fastest are timed again in three INTERLEAVED trials of >= 2 ms each,
    // every one keeping its best time -- two 1 ms samples (six launches of a 0.2 ms kernel) let the fine level of 256^3 come out as
    // k_sellp on one box and k_sellp2 on the next while their times differ by more than the spread of either (204-222 against 218-239 us).
    {
        float lead = 1e30f;
        for (const auto &kv : seen) lead = std::min(lead, kv.second);
        std::vector<Candidate> close;
        for (const auto &kv : seen) if (kv.second <= 1.08f * lead) close.push_back(kv.first);
        if (close.size() > 1)
            for (int trial = 0; trial < 3; ++trial)
                for (const auto &c : close) {
                    const int reps = std::min(64, std::max(3, (int)(2.0f / std::max(seen[c], 1e-3f)) + 1));
                    float ms = 0;
                    CHK(sample(c, reps, &ms));
                    seen[c] = std::min(seen[c], ms);
                }
    }
    const PlanChoice c = choose_plan(seen, Candidate{guard.v, guard.l, guard.xw}, lanes.front());
    guard.armed = false;
    op->loc.variant = c.best.form; op->loc.lanes = c.best.lanes; op->loc.vw_rows = c.best.xwin_rows;
    const double t_fin0 = now_s();
    finish_plan(op, c.best.form);
    const double t_fin1 = now_s();
    plan_cache_store(key, op, c.best, c.ms, c.runner_up, c.runner_up_ms);
    if (verbose)
        fprintf(stderr, "[sgpu] autotune of %d rows x %lld nnz (%.1f per row): %zu candidates, variant %d with %d lanes (x windows: %d rows per workgroup) at %.1f us (fastest %.1f us; runner-up variant %d with %d lanes at %.1f us); sliced ELLPACK %.2f s, "
                        "16-bit columns %.2f s, x in LDS %.2f s, column order %.2f s, timing %.2f s (of which freeing the forms that lost %.2f s)\n", op->M, (long long)op->loc.nnz, avg_row, cands.size(), c.best.form, c.best.lanes, c.best.xwin_rows, c.ms * 1e3,
                c.fastest * 1e3, c.runner_up.form, shown_lanes(c.runner_up), c.runner_up_ms * 1e3, t_sell - t_begin, t_cc - t_sell, t_xl - t_cc, t_cm1 - t_cm0, now_s() - t_cm - (t_cm1 - t_cm0), t_fin1 - t_fin0);
    return SGPU_OK;
}

int sgpu_spmv(sgpu_op *op, const value_t *v, value_t *w) {
    CHK(need_ctx());
    if (!op || !v || !w) return fail(SGPU_ERR_ARG, "null argument");
    return apply(op, sk::EPI_SPMV, v, w, EpiArgs());
}

int sgpu_residual(sgpu_op *op, const value_t *u, const value_t *rhs, value_t *res) {
    CHK(need_ctx());
    if (!op || !u || !rhs || !res) return fail(SGPU_ERR_ARG, "null argument");
    EpiArgs e; e.rhs = rhs;
    return apply(op, sk::EPI_RESIDUAL, u, res, e);
}

// res = c * w o (rhs - A u): the epilogue of the first Chebyshev step with w in inv_diag's place -- (c w_i) (rhs_i - (A u)_i), the
// reference's left-to-right product; that epilogue also writes u + res, here into the operator's ping-pong buffer, which nobody reads
int sgpu_residual_multiply(sgpu_op *op, const value_t *u, const value_t *rhs, value_t *res, const value_t *w, value_t c) {
    CHK(need_ctx());
    if (!op || !u || !rhs || !res || !w) return fail(SGPU_ERR_ARG, "null argument");
    if (res == u || res == rhs || res == w) return fail(SGPU_ERR_ARG, "residual_multiply: res must not alias u, rhs or w");
    CHK(ensure_tmp(op));
    EpiArgs e; e.rhs = rhs; e.inv_diag = w; e.u = u; e.d = res; e.c0 = c;
    return apply(op, sk::EPI_CHEBY0, u, op->tmp, e);
}

int sgpu_residual_negative(sgpu_op *op, const value_t *u, const value_t *rhs, value_t *res) {
    CHK(need_ctx());
    if (!op || !u || !rhs || !res) return fail(SGPU_ERR_ARG, "null argument");
    if (!op->ones && op->M > 0) {
        HIPCHK(op->ones.alloc((size_t)op->M));
        CHK(sgpu_vec_fill(op->ones, 1.0, (size_t)op->M));
    }
    return sgpu_residual_multiply(op, u, rhs, res, op->ones, 1.0);      // 1 * 1 * (rhs - A u): exact, signs of zeros included
}

int sgpu_jacobi(sgpu_op *op, int iter, value_t omega, value_t *u, const value_t *rhs) {
    CHK(need_ctx());
    if (!op || !u || !rhs || iter < 0) return fail(SGPU_ERR_ARG, "bad argument");
    if (omega == 0.0) omega = JACOBI_OMEGA_REF;
    CHK(ensure_tmp(op));
    double *res = nullptr;
    CHK(jacobi_pp(op, iter, omega, u, op->tmp, rhs, &res));
    if (res != u) HIPCHK(hipMemcpyAsync(u, res, (size_t)op->M * sizeof(double), hipMemcpyDeviceToDevice, g.cs));
    return SGPU_OK;
}

int sgpu_chebyshev(sgpu_op *op, int iter, value_t eig_max, value_t *u, const value_t *rhs) {
    CHK(need_ctx());
    if (!op || !u || !rhs || iter < 0) return fail(SGPU_ERR_ARG, "bad argument");
    if (!(eig_max > 0.0)) return fail(SGPU_ERR_ARG, "chebyshev needs eig_max > 0");
    CHK(ensure_tmp(op));
    double *res = nullptr;
    CHK(cheby_pp(op, iter, eig_max, u, op->tmp, rhs, &res));
    if (res != u) HIPCHK(hipMemcpyAsync(u, res, (size_t)op->M * sizeof(double), hipMemcpyDeviceToDevice, g.cs));
    return SGPU_OK;
}

int sgpu_prolong_correct(sgpu_op *P, const value_t *e_coarse, value_t *u) {
    CHK(need_ctx());
    if (!P || !e_coarse || !u) return fail(SGPU_ERR_ARG, "null argument");
    return apply(P, sk::EPI_SUB, e_coarse, u, EpiArgs());
}

int sgpu_debug_pack(sgpu_op *op, const value_t *v, value_t *send_host) {
    CHK(need_ctx());
    if (!op || !v) return fail(SGPU_ERR_ARG, "null argument");
    if (op->vIndexSize == 0) return SGPU_OK;
    SGPU_LAUNCH(sk::k_pack, dim3((op->vIndexSize + sk::BLOCK - 1) / sk::BLOCK), dim3(sk::BLOCK), 0, g.cs,
                       v, op->vIndex, op->send_buf, op->vIndexSize, op->halo_fp32, (const uint64_t *)nullptr, (uint64_t)0);
    HIPCHK(hipGetLastError());
    return sgpu_vec_download(send_host, op->send_buf, (size_t)op->vIndexSize);
}

int sgpu_debug_gather_probe(sgpu_op *op, int mode, const value_t *x, int reps, float *ms) {
    CHK(need_ctx());
    if (!op || !x || !ms || reps < 1) return fail(SGPU_ERR_ARG, "bad argument");
    const long nnz = op->loc.nnz;
    const int grid = (int)((nnz + sk::BLOCK * 4 - 1) / (sk::BLOCK * 4));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, g.cs));
    for (int i = 0; i < reps; ++i)
        SGPU_LAUNCH(sk::k_gather_probe, dim3(grid), dim3(sk::BLOCK), 0, g.cs, op->loc.csr.col, x, g.dscalar, nnz, mode);
    HIPCHK(hipEventRecord(e1, g.cs));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipEventElapsedTime(ms, e0, e1));
    *ms /= reps;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return SGPU_OK;
}

int sgpu_debug_block_plan(const sgpu_op *op, int big, long *out) {
    if (!op || !out) return fail(SGPU_ERR_ARG, "null argument");
    const CsrPart &P = op->loc;
    if (big == 2) {                                            // the x-in-LDS plan (is_xlds_chunk)
        if (!P.xlp.xl_ok) return fail(SGPU_ERR_STATE, "the x-in-LDS plan was not built");
        long rmx = 0;
        for (size_t b = 0; b + 1 < P.xl_blk_h.size(); ++b) rmx = std::max(rmx, (long)(P.xl_blk_h[b + 1] - P.xl_blk_h[b]));
        out[0] = P.xl_nblk; out[1] = P.xl_maxt; out[2] = P.xl_win; out[3] = P.xl_acc_lds ? 1 : 0; out[4] = rmx; out[5] = out[6] = out[7] = 0;
        return SGPU_OK;
    }
    const std::vector<int> &blk = big ? P.h_blk_big : P.h_blk;
    if (blk.size() < 2 || P.h_rp.empty()) return fail(SGPU_ERR_STATE, "the operator keeps no host copy of its row-block plan");
    const int nb = (int)blk.size() - 1, cap = big ? sk::CAP_BIG : sk::CAP;
    long mn = LONG_MAX, mx = 0, rmn = LONG_MAX, rmx = 0, longrows = 0, rowmax = 0;
    for (int b = 0; b < nb; ++b) {
        const long e = (long)P.h_rp[(size_t)blk[(size_t)b + 1]] - P.h_rp[(size_t)blk[(size_t)b]], r = blk[(size_t)b + 1] - blk[(size_t)b];
        mn = std::min(mn, e); mx = std::max(mx, e); rmn = std::min(rmn, r); rmx = std::max(rmx, r);
        if (r == 1 && e > cap) ++longrows;
    }
    for (int r = 0; r < P.nrows; ++r) rowmax = std::max(rowmax, (long)(P.h_rp[(size_t)r + 1] - P.h_rp[(size_t)r]));
    out[0] = nb; out[1] = mn; out[2] = mx; out[3] = P.nnz; out[4] = rmn; out[5] = rmx; out[6] = longrows; out[7] = rowmax;
    return SGPU_OK;
}

int sgpu_debug_stream_ceiling(size_t read_bytes, size_t write_bytes, int reps, float *us, int *mode, size_t *bytes_moved) {
    CHK(need_ctx());
    if (!us || reps < 1 || write_bytes < 8 * 64 || read_bytes < 16) return fail(SGPU_ERR_ARG, "bad argument");
    const size_t n_w = write_bytes / 8;
    const int q = (int)std::max<size_t>(1, (read_bytes + 8 * n_w) / (16 * n_w));       // 16-byte loads per written double, rounded
    const size_t waves = (n_w + 63) / 64, n_r = waves * 64 * (size_t)q;                // (whole waves: every lane of the last wave has its run)
    DevArr<char> rd_; DevArr<double> wr_;
    HIPCHK(rd_.alloc(n_r * 16));
    if (wr_.alloc(n_w) != hipSuccess) return fail(SGPU_ERR_HIP, "hipMalloc of the ceiling's output failed");
    void *rd = rd_.get(); double *wr = wr_;
    struct Free { hipEvent_t e0 = nullptr, e1 = nullptr; ~Free() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); } } fr;
    HIPCHK(hipMemsetAsync(rd, 0, n_r * 16, g.cs));
    HIPCHK(hipEventCreate(&fr.e0)); HIPCHK(hipEventCreate(&fr.e1));
    const dim3 grid((unsigned)((n_w + sk::BLOCK - 1) / sk::BLOCK)), block(sk::BLOCK);
    auto launch = [&](int m) {
        const sk::ceil_d2 *r = static_cast<const sk::ceil_d2 *>(rd);
        switch (m) {
        case 0: SGPU_LAUNCH(sk::k_stream_ceiling<0>, grid, block, 0, g.cs, r, wr, n_w, q); break;
        case 1: SGPU_LAUNCH(sk::k_stream_ceiling<1>, grid, block, 0, g.cs, r, wr, n_w, q); break;
        case 2: SGPU_LAUNCH(sk::k_stream_ceiling<2>, grid, block, 0, g.cs, r, wr, n_w, q); break;
        default: SGPU_LAUNCH(sk::k_stream_ceiling<3>, grid, block, 0, g.cs, r, wr, n_w, q); break;
        }
    };
    float best = 1e30f; int bm = 0;
    for (int round = 0; round < 2; ++round)              // twice round the four forms: the first ones of a process run at ramping clocks
        for (int m = 0; m < 4; ++m) {
            for (int i = 0; i < 3; ++i) launch(m);
            HIPCHK(hipEventRecord(fr.e0, g.cs));
            for (int i = 0; i < reps; ++i) launch(m);
            HIPCHK(hipEventRecord(fr.e1, g.cs));
            HIPCHK(hipEventSynchronize(fr.e1));
            HIPCHK(hipGetLastError());
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, fr.e0, fr.e1));
            ms /= reps;
            if (ms < best) { best = ms; bm = m; }
        }
    *us = best * 1e3f;
    if (mode) *mode = bm;
    if (bytes_moved) *bytes_moved = n_r * 16 + n_w * 8;
    return SGPU_OK;
}

int sgpu_debug_inject_halo(sgpu_op *op, const value_t *recv_host) {
    CHK(need_ctx());
    if (!op) return fail(SGPU_ERR_ARG, "null argument");
    if (op->recvSize) CHK(sgpu_vec_upload(op->recv_buf, recv_host, (size_t)op->recvSize));
    op->injected = true;
    return SGPU_OK;
}

// ---- host-slice forms ----

int sgpu_spmv_host(sgpu_op *op, const value_t *v_host, value_t *w_host) {
    CHK(need_ctx());
    if (!op || !v_host || !w_host) return fail(SGPU_ERR_ARG, "null argument");
    DevArr<double> v, w;
    CHK(dev_alloc(v, op->N_local)); CHK(dev_alloc(w, op->M));
    CHK(sgpu_vec_upload(v, v_host, op->N_local));
    CHK(sgpu_spmv(op, v, w));
    return sgpu_vec_download(w_host, w, op->M);
}
int sgpu_jacobi_host(sgpu_op *op, int iter, value_t omega, value_t *u_host, const value_t *rhs_host) {
    CHK(need_ctx());
    if (!op || !u_host || !rhs_host) return fail(SGPU_ERR_ARG, "null argument");
    DevArr<double> u, r;
    CHK(dev_alloc(u, op->M)); CHK(dev_alloc(r, op->M));
    CHK(sgpu_vec_upload(u, u_host, op->M)); CHK(sgpu_vec_upload(r, rhs_host, op->M));
    CHK(sgpu_jacobi(op, iter, omega, u, r));
    return sgpu_vec_download(u_host, u, op->M);
}
int sgpu_chebyshev_host(sgpu_op *op, int iter, value_t eig_max, value_t *u_host, const value_t *rhs_host) {
    CHK(need_ctx());
    if (!op || !u_host || !rhs_host) return fail(SGPU_ERR_ARG, "null argument");
    DevArr<double> u, r;
    CHK(dev_alloc(u, op->M)); CHK(dev_alloc(r, op->M));
    CHK(sgpu_vec_upload(u, u_host, op->M)); CHK(sgpu_vec_upload(r, rhs_host, op->M));
    CHK(sgpu_chebyshev(op, iter, eig_max, u, r));
    return sgpu_vec_download(u_host, u, op->M);
}

} // extern "C"

// ===========================================================================
// multigrid
// a captured graph and its executable instance, destroyed together
struct CapturedGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    CapturedGraph() = default;
    CapturedGraph(CapturedGraph &&o) noexcept : graph(o.graph), exec(o.exec) { o.graph = nullptr; o.exec = nullptr; }
    CapturedGraph &operator=(CapturedGraph &&o) noexcept {
        if (this != &o) { drop_graph(); graph = o.graph; exec = o.exec; o.graph = nullptr; o.exec = nullptr; }
        return *this;
    }
    ~CapturedGraph() { drop_graph(); }
    void drop_graph() {
        if (exec) { hipGraphExecDestroy(exec); exec = nullptr; }
        if (graph) { hipGraphDestroy(graph); graph = nullptr; }
    }
};
// a captured V-cycle and the (u, rhs) pointer pair it was captured on
struct CapturedCycle : CapturedGraph { double *u = nullptr; const double *rhs = nullptr; bool u_zero = false; };

// block V-cycle / pCG state of a hierarchy for ONE K (sgpu_block.hip.inc): made at the first block call with that K
struct AmgBlock {
    int K = 0;
    std::vector<DevArr<double>> res, rhs, u, alt;   // block work vectors per level, as sgpu_amg's scalar ones
    DevArr<double> alt0, r, rho, hh, p;
    DevArr<double> cm;                        // coarsest CG: the K columns unpacked (rhs, then u), 2 * n * K
    DevArr<double> S, partials;               // device scalars [8][K]; dot partial sums [n_partials][K]
    PinArr<double> hS;                        // pinned mirror of one row of S
    std::vector<CapturedCycle> graphs;
    uint64_t graph_gen = 0, block_gen = 0;
    void drop_graphs() { graphs.clear(); }
};

// restarted FGMRES state of a hierarchy (sgpu_gmres.hip.inc): made at the first sgpu_solve_FGMRES with a given restart length;
// its graph: the V-cycle on (pout, pin) from a zero iterate, captured once
struct AmgGmres : CapturedGraph {
    int restart = 0;
    size_t ld = 0;                                   // leading dimension of V and Z: the rows rounded up to an even number
    DevArr<double> V, Z;                             // Krylov basis (restart + 1 columns), preconditioned vectors (restart columns)
    DevArr<double> pin, pout;                        // the fixed pair the V-cycle preconditions through
    DevArr<double> coef, partials;                   // device coefficients (two Gram-Schmidt sets and ||w||^2); the dots' partial sums
    PinArr<double> hcoef;                            // pinned mirror of coef
    uint64_t graph_gen = 0;
};

// LOBPCG state of a hierarchy for ONE K (sgpu_eig.hip.inc): made at the first sgpu_eigs_LOBPCG with that K; its graph: the block
// V-cycle on (W, R) from a zero iterate, captured once
struct AmgEig : CapturedGraph {
    int K = 0;
    DevArr<double> AX, R, W, AW, P, AP;              // block vectors (X is the caller's)
    DevArr<double> gpart, rpart;                     // partial sums: 12 Gram blocks [n_partials][K*K] each; the residual norms [n_partials][K]
    DevArr<double> coef;                             // device: 3 K*K mix coefficients | K lambda | K ||r_j||^2 | 12 Gram blocks of K*K
    PinArr<double> hmix, hlam, hdown;                // pinned: what goes up (coefficients, lambda), what comes down (norms, Gram blocks)
    uint64_t graph_gen = 0, block_gen = 0;
    int debug_stop = -1;                             // sgpu_debug_eig_stop: the iteration a test wants to look into
    // A x = lambda B x (amg_geig): made at the first sgpu_eigs_LOBPCG_gen with this K, never by the standard solve
    bool gen = false;
    DevArr<double> BX, BW, BP;                       // B times X, W, P, carried
    DevArr<double> bpart, bnrm;                      // ||(Bx)_j||^2: partial sums [n_partials][K], the K sums
    PinArr<double> hbn;                              // pinned mirror of bnrm
};

// what hard locking adds to LOBPCG (sgpu_eig_lock.hip.inc): made at the first locked solve with a locked column (or the first
// sgpu_eigs_LOBPCG_many), never by the unconstrained solves; shared by every K
struct AmgLock {
    DevArr<double> part;                             // the lock Gram's partial sums: LOCK_MAX / LOCK_C passes of [n_partials][LOCK_C * 8]
    DevArr<double> coef;                             // C = Z^T Y: LOCK_MAX * 8 doubles, device only
};

struct sgpu_amg {
    int nlevels = 0;
    std::vector<sgpu_op *> A, P, R;
    std::vector<double> eig;
    sgpu_amg_params prm;
    // per level l < nlevels-1: res[l] (A[l].M); per level l >= 1: rhs_l / u_l / alt_l (A[l].M)
    std::vector<DevArr<double>> res, rhs, u, alt;
    DevArr<double> alt0;      // ping-pong partner of the caller's level-0 u
    // solve work vectors (level 0)
    DevArr<double> r, rho, hh, p;
    DevArr<double> Ainv;      // dense inverse of the coarsest operator (coarse_solver == 1)
    bool coarse_local = true; // the coarsest operator has no halo on any rank
    // sgpu_amg_create_null_space: 0 none; 1 every level's operator annihilates constants.  Under 1 Ainv holds the pseudo-inverse, the CG
    // coarsest solvers get a centred right-hand side, and the solvers iterate on the centred right-hand side and centre u at the end
    int null_space = 0;
    DevArr<double> nsw;       // kind 1: level-0 work vector, the centred right-hand side where the caller's must stay as it is
    DevArr<double> ncw;       // kind 1 with a CG coarsest solver: the centred coarsest right-hand side when it is not the level's own buffer
    // captured V-cycles, one per (u, rhs) pointer pair (single rank): replaying a hipGraph removes
    // the ~70 launch gaps of a V-cycle, which weigh as much as a whole coarse level
    std::vector<CapturedCycle> graphs;
    // Multi-rank: the levels agglomerated onto this rank (no operator with a halo from level `tail_level` down) form a
    // sub-V-cycle without any communication; it is captured once and replayed as ONE graph launch per V-cycle instead
    // of ~8 launches per level.  Ranks that own no rows of those levels launch nothing at all for them.
    int  tail_level = -1;
    bool tail_capturing = false;
    CapturedGraph tail;
    double *tail_out = nullptr;        // which of u[tail_level] / alt[tail_level] holds the sub-V-cycle's result
    uint64_t graph_gen = 0;            // g_plan_generation the graphs were captured under
    bool coarse_host_driven = false;   // coarsest level too large for the LDS-resident solvers: host-driven CG, no graph capture
    bool coarse_device_cg = false;     // ... and coarse_solver == 2: the device-resident CG instead (sgpu_coarse_cg.hip.inc), capturable
    DevArr<double> dcg;                // its work space on a rank whose coarsest rows exceed CG_MAXN: res, dir, mt, partial sums, scalars
    int dcg_rows = 0;
    std::unique_ptr<AmgBlock> blk[3];  // K = 2, 4, 8
    std::unique_ptr<AmgGmres> gm;      // sgpu_solve_FGMRES
    std::unique_ptr<AmgEig> eigs[3];   // sgpu_eigs_LOBPCG, K = 2, 4, 8
    std::unique_ptr<AmgLock> lock;     // sgpu_eigs_LOBPCG_locked / _many
    void drop_graphs() {
        for (auto &b : blk) if (b) b->drop_graphs();
        if (gm) gm->drop_graph();
        for (auto &e : eigs) if (e) e->drop_graph();
        graphs.clear();
        tail.drop_graph();
    }
};

namespace {

int coarse_cg_single(sgpu_amg *h, sgpu_op *A, double *u, const double *rhs, int *iters) {
    if (A->M > sk::CG_MAXN) return fail(SGPU_ERR_ARG, "coarsest level has %d rows; the LDS-resident CG supports <= %d", A->M, sk::CG_MAXN);
    sk::CoarseCGArgs a;
    a.row_ptr = A->loc.csr.row_ptr; a.col = A->loc.csr.col; a.val = A->loc.csr.val; a.n = A->M;
    a.rhs = rhs; a.u = u; a.max_iter = h->prm.CG_coarsest_max_iter; a.tol = h->prm.CG_coarsest_tol;
    a.iters_out = iters ? g.dint + 1 : nullptr;
    SGPU_LAUNCH(sk::k_coarse_cg, dim3(1), dim3(sk::CG_BLOCK), 0, g.cs, a);
    HIPCHK(hipGetLastError());
    if (iters) {
        HIPCHK(hipMemcpyAsync(g.hint + 1, g.dint + 1, sizeof(int), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        *iters = g.hint[1];
    }
    return SGPU_OK;
}

// solve_coarsest_CG with a row-partitioned coarsest operator: host-driven loop
// over the distributed kernels (src/saena_object_solve.cpp:14-114).
int coarse_cg_dist(sgpu_amg *h, sgpu_op *A, double *u, const double *rhs, int *iters) {
    const size_t n = (size_t)A->M;
    DevArr<double> res, dir, mt;
    CHK(dev_alloc(res, n)); CHK(dev_alloc(dir, n)); CHK(dev_alloc(mt, n));
    CHK(sgpu_vec_copy(res, rhs, n)); CHK(sgpu_vec_copy(dir, rhs, n));
    const double tol = h->prm.CG_coarsest_tol;
    double initial_dot = 0, dot = 0, factor = 0, dot_prev = 0;
    CHK(sgpu_dot(res, res, n, &initial_dot));
    const double thres = initial_dot * tol * tol;
    dot = initial_dot;
    int max_iter = h->prm.CG_coarsest_max_iter;
    if (dot < tol * tol) max_iter = 0;
    int i = 1;
    while (i < max_iter) {
        CHK(sgpu_spmv(A, dir, mt));
        CHK(sgpu_dot(dir, mt, n, &factor));
        factor = dot / factor;
        CHK(sgpu_vec_axpby(factor, dir, 1.0, u, n));
        CHK(sgpu_vec_axpby(-factor, mt, 1.0, res, n));
        dot_prev = dot;
        CHK(sgpu_dot(res, res, n, &dot));
        if (dot < thres) break;
        factor = dot / dot_prev;
        CHK(sgpu_vec_axpby(1.0, res, factor, dir, n));
        i++;
    }
    if (i == max_iter && max_iter != 0) i--;
    if (iters) *iters = i;
    CHK(sgpu_device_sync());
    return SGPU_OK;
}

int ensure_dcg(sgpu_amg *h, int M);                                                         // sgpu_coarse_cg.hip.inc
int coarse_cg_device(sgpu_amg *h, sgpu_op *A, double *u, const double *rhs, int *iters);

int coarse_solve(sgpu_amg *h, double *u, const double *rhs, int *iters) {
    sgpu_op *A = h->A[h->nlevels - 1];
    if (h->Ainv) {
        SGPU_LAUNCH(sk::k_dense_solve, dim3(1), dim3(sk::CG_BLOCK), 0, g.cs, h->Ainv, rhs, u, (int)A->M);
        HIPCHK(hipGetLastError());
        if (iters) *iters = 0;
        return SGPU_OK;
    }
    if (h->null_space == 1 && A->M > 0) {
        // the constant null space: CG on the centred right-hand side (from a zero iterate on a symmetric operator it stays in the
        // complement of constants, so nothing is centred afterwards).  In place in the level's own buffer; a right-hand side that
        // is the caller's (a one-level hierarchy, sgpu_coarsest_solve) is centred into a work vector
        const int L = h->nlevels - 1;
        double *c = (L >= 1 && rhs == h->rhs[L].get()) ? h->rhs[L].get() : h->ncw.get();
        CHK(center_async(rhs, c, (size_t)A->M));
        rhs = c;
    }
    if (h->coarse_local && !h->coarse_host_driven) {
        if (A->M == 0) { if (iters) *iters = 0; return SGPU_OK; }      // this rank holds no coarsest rows
        if (h->coarse_device_cg && A->M > sk::CG_MAXN) return coarse_cg_device(h, A, u, rhs, iters);
        return coarse_cg_single(h, A, u, rhs, iters);
    }
    // row-partitioned coarsest operator, or one with more than CG_MAXN rows (coarsening stalled, max_level cut-off):
    // the reference's CG has no size limit (saena_object_solve.cpp:14-114) -- host-driven loop over the device kernels
    return coarse_cg_dist(h, A, u, rhs, iters);
}

int smooth_pp(sgpu_amg *h, int l, int iter, double *u, double *alt, const double *rhs, double **out, bool zero_first = false, bool zero_done = false) {
    if (h->prm.smoother == 0) {
        const double om = h->prm.jacobi_omega != 0.0 ? h->prm.jacobi_omega : JACOBI_OMEGA_REF;
        return jacobi_pp(h->A[l], iter, om, u, alt, rhs, out, zero_first, zero_done);
    }
    return cheby_pp(h->A[l], iter, h->eig[l], u, alt, rhs, out, zero_first, zero_done);
}

// saena_object::vcycle (src/saena_object_solve.cpp:961-1431).  u/alt are the two
// ping-pong buffers of this level; *out names the one holding the result.
// u_zero: the iterate is zero by construction (every coarse level, :1249; the fine level when the V-cycle
// preconditions CG, :2640) and the buffer's CONTENT is not read: the first pre-smoothing sweep then needs no
// pass over the matrix (k_zero_sweep) and the zero fill itself is skipped.  Results are those of the plain sweep.
int vcycle_level(sgpu_amg *h, int l, double *u, double *alt, const double *rhs, double **out, bool u_zero, bool zero_done = false);

// the communication-free sub-V-cycle from `tail_level` down as one graph launch (captured at its first use)
int tail_run(sgpu_amg *h, double **out) {
    const int l = h->tail_level;
    if (h->tail.exec && h->graph_gen != g_plan_generation) { HIPCHK(hipStreamSynchronize(g.cs)); h->drop_graphs(); }
    if (!h->tail.exec) {
        h->graph_gen = g_plan_generation;
        h->tail_capturing = true;
        hipError_t e = hipStreamBeginCapture(g.cs, hipStreamCaptureModeThreadLocal);
        int st = SGPU_OK;
        if (e == hipSuccess) {
            st = vcycle_level(h, l, h->u[l], h->alt[l], h->rhs[l], &h->tail_out, true);
            e = hipStreamEndCapture(g.cs, &h->tail.graph);
            if (e == hipSuccess && st == SGPU_OK) e = hipGraphInstantiate(&h->tail.exec, h->tail.graph, nullptr, nullptr, 0);
        }
        h->tail_capturing = false;
        if (e != hipSuccess || st != SGPU_OK) {          // not capturable here: run these levels eagerly from now on
            (void)hipGetLastError();
            h->drop_graphs();
            h->tail_level = -1;
            return vcycle_level(h, l, h->u[l], h->alt[l], h->rhs[l], out, true);
        }
    }
    ++g_launches;
    HIPCHK(hipGraphLaunch(h->tail.exec, g.cs));
    *out = h->tail_out;
    return SGPU_OK;
}

// zero_done: the first pre-smoothing sweep of this level (from its zero iterate) was written to `alt` by the epilogue of the
// restriction that produced `rhs` (EPI_RSWEEP: one launch fewer per coarse level; the same arithmetic on the same numbers)
int vcycle_level(sgpu_amg *h, int l, double *u, double *alt, const double *rhs, double **out, bool u_zero, bool zero_done) {
    const size_t n = (size_t)h->A[l]->M;
    if (l == h->tail_level && !h->tail_capturing && u_zero && u == h->u[l] && alt == h->alt[l] && rhs == h->rhs[l]) return tail_run(h, out);
    if (l == h->nlevels - 1) {                             // :991-1057
        if (u_zero && !h->Ainv) CHK(sgpu_vec_fill(u, 0.0, n));      // the CG solvers start from the iterate; the dense solve overwrites it
        CHK(coarse_solve(h, u, rhs, nullptr));
        *out = u;
        return SGPU_OK;
    }
    double *cur = u, *oth = alt, *t = nullptr;
    if (h->prm.preSmooth) {                                // :1105-1107
        CHK(smooth_pp(h, l, h->prm.preSmooth, cur, oth, rhs, &t, u_zero, u_zero && zero_done));
        if (t != cur) std::swap(cur, oth);
    } else if (u_zero) {
        CHK(sgpu_vec_fill(cur, 0.0, n));
    }
    {                                                      // :1140 residual
        EpiArgs e; e.rhs = rhs;
        CHK(apply(h->A[l], sk::EPI_RESIDUAL, cur, h->res[l], e));
    }
    // :1175 res_coarse = R res.  One rank, and a next level that smooths: the restriction's epilogue also writes that level's
    // first sweep from the zero iterate (k_zero_sweep's arithmetic on the value it has just summed) -- one launch fewer per
    // coarse level, which is what the small levels are made of (SAENA_NO_RSWEEP=1: two launches, as before round 3)
    const bool no_rsweep = std::getenv("SAENA_NO_RSWEEP") != nullptr;       // (read per call: a captured graph keeps what it was captured with)
    sgpu_op *An = h->A[l + 1];
    const bool fuse = !no_rsweep && !g.multi() && h->prm.preSmooth > 0 && l + 1 < h->nlevels - 1 && An->inv_diag && An->M > 0 &&
                      !h->R[l]->has_remote && !is_dense(h->R[l]->loc.variant);
    if (fuse) {
        EpiArgs e; e.inv_diag = An->inv_diag; e.y2 = h->alt[l + 1];
        if (h->prm.smoother == 0) { e.c0 = h->prm.jacobi_omega != 0.0 ? h->prm.jacobi_omega : JACOBI_OMEGA_REF; e.c1 = 0.0; }
        else {
            CHK(ensure_d(An));
            const double alpha = 0.13 * h->eig[l + 1], beta = h->eig[l + 1], theta = (beta + alpha) / 2.0;      // cheby_pp's constants
            e.d = An->dvec; e.c0 = 1.0 / theta; e.c1 = 1.0;
        }
        CHK(apply(h->R[l], sk::EPI_RSWEEP, h->res[l], h->rhs[l + 1], e));
    } else {
        CHK(apply(h->R[l], sk::EPI_SPMV, h->res[l], h->rhs[l + 1], EpiArgs()));
    }
    double *uc = nullptr;                                                     // :1249 uCorrCoarse = 0, :1254
    CHK(vcycle_level(h, l + 1, h->u[l + 1], h->alt[l + 1], h->rhs[l + 1], &uc, true, fuse));
    CHK(apply(h->P[l], sk::EPI_SUB, uc, cur, EpiArgs()));                     // :1325 + :1360-1361
    if (h->prm.postSmooth) {                               // :1397-1399
        CHK(smooth_pp(h, l, h->prm.postSmooth, cur, oth, rhs, &t));
        if (t != cur) std::swap(cur, oth);
    }
    *out = cur;
    return SGPU_OK;
}

int vcycle0_eager(sgpu_amg *h, double *u, const double *rhs, bool u_zero) {
    double *out = nullptr;
    CHK(vcycle_level(h, 0, u, h->alt0, rhs, &out, u_zero));
    if (out != u) HIPCHK(hipMemcpyAsync(u, out, (size_t)h->A[0]->M * sizeof(double), hipMemcpyDeviceToDevice, g.cs));
    return SGPU_OK;
}

// u_zero: the caller guarantees a zero iterate WITHOUT having written it (see vcycle_level)
int vcycle0(sgpu_amg *h, double *u, const double *rhs, bool u_zero = false) {
    if (!h->prm.use_graph || g.multi() || h->coarse_host_driven) return vcycle0_eager(h, u, rhs, u_zero);
    if (!h->graphs.empty() && h->graph_gen != g_plan_generation) {   // an operator was retuned since the capture: the graphs
        HIPCHK(hipStreamSynchronize(g.cs));                           // may launch kernels on freed plan buffers
        h->drop_graphs();
    }
    h->graph_gen = g_plan_generation;
    for (auto &c : h->graphs)
        if (c.u == u && c.rhs == rhs && c.u_zero == u_zero) { ++g_launches; HIPCHK(hipGraphLaunch(c.exec, g.cs)); return SGPU_OK; }
    CapturedCycle c;
    c.u = u; c.rhs = rhs; c.u_zero = u_zero;
    HIPCHK(hipStreamBeginCapture(g.cs, hipStreamCaptureModeThreadLocal));
    const int st = vcycle0_eager(h, u, rhs, u_zero);
    const hipError_t e = hipStreamEndCapture(g.cs, &c.graph);
    if (st != SGPU_OK) return st;
    if (e != hipSuccess) return fail(SGPU_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    HIPCHK(hipGraphInstantiate(&c.exec, c.graph, nullptr, nullptr, 0));
    if (h->graphs.size() >= 8) h->graphs.erase(h->graphs.begin());                  // bounded cache
    h->graphs.push_back(std::move(c));
    ++g_launches; HIPCHK(hipGraphLaunch(h->graphs.back().exec, g.cs));
    return SGPU_OK;
}

// dense inverse of a small one-rank operator by Gauss-Jordan with partial pivoting, on the host (the direct coarsest solve of
// sgpu_amg_create and sgpu_amg_set_operator); inv: row-major M x M
int dense_inverse(const sgpu_op *Ac, std::vector<double> &inv, bool pinv = false) {
    const int n = Ac->M;
    std::vector<double> a((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int k = Ac->loc.h_rp[i]; k < Ac->loc.h_rp[i + 1]; ++k) a[(size_t)i * n + Ac->loc.h_col[k]] = Ac->h_val[k];
    // the elimination itself: coarse_pinv.h.  pinv: the pseudo-inverse on the complement of constants (null_space == 1)
    if (pinv) {
        if (!coarse_pinv::pseudo_inverse(a, n, inv))
            return fail(SGPU_ERR_ARG, "coarsest operator: no pseudo-inverse (the mean of its diagonal is not positive, or A + (s/n) 1 1^T is singular: a null space larger than the constants)");
        return SGPU_OK;
    }
    if (!coarse_pinv::gauss_jordan_inverse(a, n, inv)) return fail(SGPU_ERR_ARG, "coarsest operator is singular");
    return SGPU_OK;
}

// how far a one-rank operator is from annihilating constants: max_i |(A 1)_i| / max_i |a_ii|, A 1 through sgpu_spmv on a vector of
// ones, downloaded.  The diagonal from inv_diag where the operator has one, from its CSR arrays otherwise.  Setup time only
int null_defect(sgpu_op *A, double *defect) {
    const size_t n = (size_t)A->M;
    *defect = 0.0;
    if (n == 0) return SGPU_OK;
    DevArr<double> one, w;
    CHK(dev_alloc(one, n)); CHK(dev_alloc(w, n));
    CHK(sgpu_vec_fill(one, 1.0, n));
    CHK(sgpu_spmv(A, one, w));
    std::vector<double> hw(n);
    CHK(sgpu_vec_download(hw.data(), w, n));
    double num = 0.0, den = 0.0;
    for (size_t i = 0; i < n; ++i) num = std::fabs(hw[i]) > num || hw[i] != hw[i] ? std::fabs(hw[i]) : num;      // (a NaN stays)
    if (A->inv_diag) {
        CHK(sgpu_vec_download(hw.data(), A->inv_diag, n));
        for (size_t i = 0; i < n; ++i) den = std::max(den, std::fabs(1.0 / hw[i]));
    } else {
        const size_t nnz = (size_t)A->loc.nnz;
        std::vector<int> rp(n + 1), col(nnz);
        std::vector<double> val(nnz);
        HIPCHK(hipMemcpyAsync(rp.data(), A->loc.csr.row_ptr, (n + 1) * sizeof(int), hipMemcpyDeviceToHost, g.cs));
        if (nnz) HIPCHK(hipMemcpyAsync(col.data(), A->loc.csr.col, nnz * sizeof(int), hipMemcpyDeviceToHost, g.cs));
        if (nnz) HIPCHK(hipMemcpyAsync(val.data(), A->loc.csr.val, nnz * sizeof(double), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        for (size_t i = 0; i < n; ++i)
            for (int k = rp[i]; k < rp[i + 1]; ++k) if ((size_t)col[k] == i) den = std::max(den, std::fabs(val[k]));
    }
    *defect = den > 0.0 ? num / den : (num == 0.0 ? 0.0 : INFINITY);
    return SGPU_OK;
}
const double NULL_DEFECT_MAX = 1e-10;     // 3.5 orders above what the setup's own hierarchies show, far below a pinned row's 1/6
int null_defect_check(sgpu_op *A, int level, const char *what) {
    double d = 0.0;
    CHK(null_defect(A, &d));
    if (!(d <= NULL_DEFECT_MAX))
        return fail(SGPU_ERR_ARG, "%s: the operator of level %d does not annihilate constants: max|A 1| / max|a_ii| = %.3e exceeds %.0e", what, level, d, NULL_DEFECT_MAX);
    return SGPU_OK;
}

} // namespace

extern "C" {

int sgpu_amg_default_params(sgpu_amg_params *p) {
    if (!p) return fail(SGPU_ERR_ARG, "null params");
    p->preSmooth = 3; p->postSmooth = 3; p->smoother = 1;          /* saena.hpp:151-155: "chebyshev", 3, 3 */
    p->jacobi_omega = 0.0; p->coarse_solver = 1;                   /* saena_object.h:165 direct_solver = "SuperLU" */
    p->CG_coarsest_max_iter = 150; p->CG_coarsest_tol = 1e-12;    /* saena_object.h:155-156 */
    p->solver_max_iter = 100; p->solver_tol = 1e-8; p->use_graph = 1;
    return SGPU_OK;
}

int sgpu_amg_create(int nlevels, sgpu_op *const *A, sgpu_op *const *P, sgpu_op *const *R, const value_t *eig_max,
                    const sgpu_amg_params *params, sgpu_amg **out) {
    return sgpu_amg_create_null_space(nlevels, A, P, R, eig_max, params, 0, out);
}

int sgpu_amg_create_null_space(int nlevels, sgpu_op *const *A, sgpu_op *const *P, sgpu_op *const *R, const value_t *eig_max,
                               const sgpu_amg_params *params, int null_space, sgpu_amg **out) {
    CHK(need_ctx());
    if (nlevels < 1 || !A || !out) return fail(SGPU_ERR_ARG, "bad hierarchy");
    if (null_space != 0 && null_space != 1) return fail(SGPU_ERR_ARG, "sgpu_amg_create_null_space: null_space is 0 (none) or 1 (constants), got %d", null_space);
    if (null_space == 1 && (g.nranks > 1 || g.multi()))
        return fail(SGPU_ERR_ARG, "sgpu_amg_create_null_space: a hierarchy that knows the constant null space runs on one rank (this context has %d)", g.nranks);
    std::unique_ptr<sgpu_amg> h(new sgpu_amg());
    h->nlevels = nlevels;
    h->null_space = null_space;
    if (params) h->prm = *params; else sgpu_amg_default_params(&h->prm);
    for (int l = 0; l < nlevels; ++l) {
        if (!A[l]) return fail(SGPU_ERR_ARG, "A[%d] is null", l);
        if (A[l]->M != A[l]->N_local) return fail(SGPU_ERR_ARG, "A[%d] is not square on this rank", l);
        h->A.push_back(A[l]);
        h->eig.push_back(eig_max ? eig_max[l] : 0.0);
        if (l < nlevels - 1) {
            if (!P || !R || !P[l] || !R[l]) return fail(SGPU_ERR_ARG, "P[%d]/R[%d] is null", l, l);
            if (P[l]->M != A[l]->M || P[l]->N_local != A[l + 1]->M) return fail(SGPU_ERR_ARG, "P[%d] shape mismatch", l);
            if (R[l]->M != A[l + 1]->M || R[l]->N_local != A[l]->M) return fail(SGPU_ERR_ARG, "R[%d] shape mismatch", l);
            h->P.push_back(P[l]); h->R.push_back(R[l]);
            if (!A[l]->inv_diag && A[l]->M > 0) return fail(SGPU_ERR_ARG, "A[%d] has no inv_diag", l);   // (no rows of this level on this rank: fine)
            if (h->prm.smoother == 1 && !(h->eig[l] > 0.0)) return fail(SGPU_ERR_ARG, "chebyshev needs eig_max[%d] > 0", l);
        }
    }
    if (null_space == 1) {
        // level 0 defines the problem, the coarsest level is the one that gets solved: both must annihilate constants
        for (int l = 0; l < nlevels; l += std::max(1, nlevels - 1)) {
            if (A[l]->has_remote || A[l]->recvSize || A[l]->vIndexSize) return fail(SGPU_ERR_ARG, "sgpu_amg_create_null_space: A[%d] has a remote part; one rank only", l);
            CHK(null_defect_check(A[l], l, "sgpu_amg_create_null_space"));
        }
    }
    h->res.resize(nlevels); h->rhs.resize(nlevels); h->u.resize(nlevels); h->alt.resize(nlevels);
    for (int l = 0; l < nlevels; ++l) {
        const size_t n = (size_t)A[l]->M;
        if (l < nlevels - 1) HIPCHK(alloc_vec(h->res[l], n));
        if (l >= 1) { HIPCHK(alloc_vec(h->rhs[l], n)); HIPCHK(alloc_vec(h->u[l], n)); HIPCHK(alloc_vec(h->alt[l], n)); }
    }
    // direct coarsest solve: one rank, or a coarsest level that lives whole on one rank (no halo on any rank:
    // the setup shrinks small levels onto rank 0, ranks holding zero rows have nothing to solve)
    bool coarse_local = !g.multi();
    bool coarse_big = A[nlevels - 1]->M > sk::CG_MAXN;   // more rows than the LDS-resident solvers hold (on any rank)
    if (g.multi()) {
        sgpu_op *Ac = A[nlevels - 1];
        double flags[2] = {(Ac->vIndexSize || Ac->recvSize) ? 1.0 : 0.0, coarse_big ? 1.0 : 0.0};
        CHK(global_sum(flags, 2));
        coarse_local = flags[0] == 0.0;
        coarse_big = flags[1] != 0.0;
    }
    h->coarse_local = coarse_local;
    // the same on every rank: the host-driven CG is collective.  coarse_solver == 2 keeps such a level on the device
    h->coarse_device_cg = h->prm.coarse_solver == 2 && coarse_local && coarse_big;
    h->coarse_host_driven = coarse_local && coarse_big && !h->coarse_device_cg;
    if (h->coarse_device_cg && A[nlevels - 1]->M > sk::CG_MAXN) CHK(ensure_dcg(h.get(), A[nlevels - 1]->M));   // no allocation may happen inside a graph capture
    if (h->prm.coarse_solver == 1 && coarse_local && A[nlevels - 1]->M > 0 && !h->coarse_host_driven) {
        // dense inverse by Gauss-Jordan with partial pivoting (host, once)
        std::vector<double> inv;
        CHK(dense_inverse(A[nlevels - 1], inv, null_space == 1));
        CHK(dev_upload(h->Ainv, inv.data(), inv.size()));
    }
    if (null_space == 1) {                         // (no allocation may happen inside a graph capture)
        HIPCHK(alloc_vec(h->nsw, (size_t)A[0]->M));
        if (!h->Ainv) HIPCHK(alloc_vec(h->ncw, (size_t)A[nlevels - 1]->M));
    }
    for (int l = 0; l < nlevels - 1; ++l)          // no allocation may happen inside a graph capture
        if (h->prm.smoother == 1) CHK(ensure_d(A[l]));
    if (g.multi() && h->prm.use_graph && h->coarse_local && !h->coarse_host_driven && !std::getenv("SAENA_NO_TAIL_GRAPH")) {
        auto halo_free = [](const sgpu_op *o) { return o->vIndexSize == 0 && o->recvSize == 0; };
        int Lt = nlevels;
        for (int l = nlevels - 1; l >= 1; --l) {
            if (!halo_free(A[l]) || (l < nlevels - 1 && (!halo_free(P[l]) || !halo_free(R[l])))) break;
            Lt = l;
        }
        if (Lt < nlevels && A[Lt]->M > 0) h->tail_level = Lt;      // (a rank without rows there has nothing to launch anyway)
    }
    const size_t n0 = (size_t)A[0]->M;
    HIPCHK(alloc_vec(h->alt0, n0));
    HIPCHK(alloc_vec(h->r, n0)); HIPCHK(alloc_vec(h->rho, n0)); HIPCHK(alloc_vec(h->hh, n0)); HIPCHK(alloc_vec(h->p, n0));
    *out = h.release();
    return SGPU_OK;
}

int sgpu_amg_destroy(sgpu_amg *h) {
    if (!h) return SGPU_OK;
    if (g.live) hipDeviceSynchronize();
    delete h;
    return SGPU_OK;
}

int sgpu_amg_get_null_space(const sgpu_amg *h, int *kind) {
    if (!h || !kind) return fail(SGPU_ERR_ARG, "sgpu_amg_get_null_space: null argument");
    *kind = h->null_space;
    return SGPU_OK;
}

int sgpu_amg_set_solve_params(sgpu_amg *h, int solver_max_iter, double solver_tol, int smoother, int preSmooth, int postSmooth) {
    CHK(need_ctx());
    if (!h) return fail(SGPU_ERR_ARG, "null hierarchy");
    if (solver_max_iter < 0 || preSmooth < 0 || postSmooth < 0 || (smoother != 0 && smoother != 1) || !(solver_tol >= 0.0))
        return fail(SGPU_ERR_ARG, "bad solve parameters");
    if (smoother == 1)
        for (int l = 0; l < h->nlevels - 1; ++l) {
            if (!(h->eig[l] > 0.0)) return fail(SGPU_ERR_ARG, "chebyshev needs eig_max[%d] > 0", l);
            CHK(ensure_d(h->A[l]));                      // no allocation may happen inside a graph capture
        }
    if (smoother != h->prm.smoother || preSmooth != h->prm.preSmooth || postSmooth != h->prm.postSmooth) {
        HIPCHK(hipStreamSynchronize(g.cs));
        h->drop_graphs();
    }
    h->prm.solver_max_iter = solver_max_iter; h->prm.solver_tol = solver_tol;
    h->prm.smoother = smoother; h->prm.preSmooth = preSmooth; h->prm.postSmooth = postSmooth;
    return SGPU_OK;
}

int sgpu_amg_profile_matvecs(sgpu_amg *h, int iter, double *us_per_level) {
    CHK(need_ctx());
    if (!h || !us_per_level || iter < 1) return fail(SGPU_ERR_ARG, "bad argument");
    for (int l = 0; l < h->nlevels; ++l) {
        sgpu_op *A = h->A[l];
        DevArr<double> v, w;
        CHK(dev_alloc(v, A->M)); CHK(dev_alloc(w, A->M));
        CHK(sgpu_vec_fill(v, 1.0, A->M));              // saena_object.cpp:625
        CHK(sgpu_spmv(A, v, w));                     // warm-up launch (code object load)
        float ms = 0;
        CHK(sgpu_time_kernel(A, 0, v, nullptr, w, iter, &ms));
        us_per_level[l] = (double)ms * 1e3;
    }
    return SGPU_OK;
}

int sgpu_vcycle(sgpu_amg *h, value_t *u, const value_t *rhs) {
    CHK(need_ctx());
    if (!h || !u || !rhs) return fail(SGPU_ERR_ARG, "null argument");
    return vcycle0(h, u, rhs);
}

int sgpu_coarsest_solve(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters) {
    CHK(need_ctx());
    if (!h || !u || !rhs) return fail(SGPU_ERR_ARG, "null argument");
    return coarse_solve(h, u, rhs, iters);
}

// ---- right-hand sides that give the outer loops nothing to iterate on (include/saena_gpu.h, "Degenerate right-hand sides") ----
// Roundings on the longest path from an element to the sum of k_sum_partial + k_reduce_partials on n elements, counted as
// tests/solver_ref.dot_roundings counts sgpu_dot's (the same grid and the same order of summation)
int sum_roundings(size_t n) {
    const size_t nb = (size_t)dot_nblocks(n);
    return (int)((n + sk::BLOCK * nb - 1) / (sk::BLOCK * nb)) + 1 + 6 + 4 + (int)((nb + sk::BLOCK - 1) / sk::BLOCK) + 6 + 4 + 1;
}
// Rule 2: is ||x - mean(x)||^2 = dot no more than the rounding error of the mean itself?  sum: what the centring's reduction left
// (n mean).  With k = sum_roundings(n) the centred entries of c 1 are at most k u |mean| each: dot <= n (k u |mean|)^2.
// False for a NaN on either side.
bool centred_is_dust(double dot, double sum, size_t n) {
    const double e = (double)sum_roundings(n) * 0x1p-53 * std::fabs(sum / (double)n);
    return dot <= (double)n * e * e;
}
// Rules 1 to 3 on the initial ||r_0||^2 (the rank-summed value, so every rank takes the same branch).  -> true: the solve ends at
// iteration 0 with *st (u is the zero vector the caller filled, nothing more is launched); false: iterate
bool solve_ends_at_start(const sgpu_amg *h, const char *who, double init_dot, size_t n, int *iters, value_t *hist, int cap, int *st) {
    if (!std::isfinite(init_dot)) {
        if (iters) *iters = 0;
        *st = fail(SGPU_ERR_NOCONV, "%s: non-finite residual at iteration 0", who);
        return true;
    }
    if (init_dot == 0.0 || (h->null_space == 1 && centred_is_dust(init_dot, g.hscalar[CENTER_SLOT], n))) {
        if (iters) *iters = 0;
        if (hist && cap > 0) hist[0] = 0.0;
        *st = SGPU_OK;
        return true;
    }
    return false;
}
// under null_space 1 the centring's sum comes down with the next sgpu_dot: one copy more in front of the same synchronisation
int fetch_center_sum(const sgpu_amg *h) {
    if (h->null_space == 1) HIPCHK(hipMemcpyAsync(g.hscalar + CENTER_SLOT, g.dscalar + CENTER_SLOT, sizeof(double), hipMemcpyDeviceToHost, g.cs));
    return SGPU_OK;
}
// rule 3 inside a loop: the dot after iteration k (1-based) is not finite
int nonfinite_stop(const char *who, int k, int *iters) {
    if (iters) *iters = k;
    return fail(SGPU_ERR_NOCONV, "%s: non-finite residual at iteration %d", who, k);
}

// saena_object::solve (src/saena_object_solve.cpp:1883-2014)
int sgpu_solve(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters, value_t *hist, int cap) {
    CHK(need_ctx());
    if (!h || !u || !rhs) return fail(SGPU_ERR_ARG, "null argument");
    sgpu_op *A = h->A[0];
    const size_t sz = (size_t)A->M;
    if (h->null_space == 1) { CHK(center_async(rhs, h->nsw, sz)); rhs = h->nsw; }      // A u = rhs - mean(rhs): rhs is read every iteration, a centred copy
    CHK(sgpu_vec_fill(u, 0.0, sz));                                   // :1926
    CHK(sgpu_residual(A, u, rhs, h->r));                              // :1942
    double init_dot = 0, current_dot = 0;
    CHK(fetch_center_sum(h));
    CHK(sgpu_dot(h->r, h->r, sz, &init_dot));
    if (hist && cap > 0) hist[0] = std::sqrt(init_dot);
    int st = SGPU_OK;
    if (solve_ends_at_start(h, "solve", init_dot, sz, iters, hist, cap, &st)) return st;
    const double THRSHLD = init_dot * h->prm.solver_tol * h->prm.solver_tol;
    int i = 0;
    for (; i < h->prm.solver_max_iter; ++i) {                         // :1957-1970
        CHK(vcycle0(h, u, rhs, i == 0));                              // the first V-cycle starts from the zero iterate set above
        CHK(sgpu_residual(A, u, rhs, h->r));
        CHK(sgpu_dot(h->r, h->r, sz, &current_dot));
        if (hist && i + 1 < cap) hist[i + 1] = std::sqrt(current_dot);
        if (current_dot < THRSHLD) break;
        if (!std::isfinite(current_dot)) return nonfinite_stop("solve", i + 1, iters);
    }
    if (h->null_space == 1) CHK(center_async(u, u, sz));              // the solution of zero mean
    const bool conv = current_dot < THRSHLD;
    if (i == h->prm.solver_max_iter) --i;
    if (iters) *iters = i + 1;
    return conv ? SGPU_OK : SGPU_ERR_NOCONV;
}

// saena_object::solve_smoother (src/saena_object_solve.cpp:2017-2117)
int sgpu_solve_smoother(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters, value_t *hist, int cap) {
    CHK(need_ctx());
    if (!h || !u || !rhs) return fail(SGPU_ERR_ARG, "null argument");
    sgpu_op *A = h->A[0];
    const size_t sz = (size_t)A->M;
    if (h->prm.smoother == 1 && !(h->eig[0] > 0.0)) return fail(SGPU_ERR_ARG, "chebyshev needs eig_max[0] > 0");
    if (h->prm.smoother == 1) CHK(ensure_d(A));
    if (h->null_space == 1) { CHK(center_async(rhs, h->nsw, sz)); rhs = h->nsw; }
    CHK(sgpu_vec_fill(u, 0.0, sz));                                   // :2051
    CHK(sgpu_residual(A, u, rhs, h->r));                              // :2060
    double init_dot = 0, current_dot = 0;
    CHK(fetch_center_sum(h));
    CHK(sgpu_dot(h->r, h->r, sz, &init_dot));
    current_dot = init_dot;
    if (hist && cap > 0) hist[0] = std::sqrt(init_dot);
    int st = SGPU_OK;
    if (solve_ends_at_start(h, "solve_smoother", init_dot, sz, iters, hist, cap, &st)) return st;
    const double THRSHLD = init_dot * h->prm.solver_tol * h->prm.solver_tol;
    int i = 0;
    for (; i < h->prm.solver_max_iter; ++i) {                         // :2072-2081
        double *out = nullptr;
        CHK(smooth_pp(h, 0, h->prm.preSmooth, u, h->alt0, rhs, &out));
        if (out != u) HIPCHK(hipMemcpyAsync(u, out, sz * sizeof(double), hipMemcpyDeviceToDevice, g.cs));
        CHK(sgpu_residual(A, u, rhs, h->r));
        CHK(sgpu_dot(h->r, h->r, sz, &current_dot));
        if (hist && i + 1 < cap) hist[i + 1] = std::sqrt(current_dot);
        if (current_dot < THRSHLD) break;
        if (!std::isfinite(current_dot)) return nonfinite_stop("solve_smoother", i + 1, iters);
    }
    if (h->null_space == 1) CHK(center_async(u, u, sz));
    const bool conv = current_dot < THRSHLD;
    if (i == h->prm.solver_max_iter) --i;
    if (iters) *iters = i + 1;
    return conv ? SGPU_OK : SGPU_ERR_NOCONV;
}

// saena_object::solve_pCG (src/saena_object_solve.cpp:2389-2801)
int sgpu_solve_pCG(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters, value_t *hist, int cap) {
    CHK(need_ctx());
    if (!h || !u || !rhs) return fail(SGPU_ERR_ARG, "null argument");
    sgpu_op *A = h->A[0];
    const size_t sz = (size_t)A->M;
    double *r = h->r, *rho = h->rho, *hh = h->hh, *p = h->p;
    CHK(sgpu_vec_fill(u, 0.0, sz));                                   // :2482
    CHK(sgpu_residual(A, u, rhs, r));                                 // :2497
    if (h->null_space == 1) CHK(center_async(r, r, sz));              // r_0 = rhs - mean(rhs); nothing is centred per iteration
    double init_dot = 0, current_dot = 0;
    CHK(fetch_center_sum(h));
    CHK(sgpu_dot(r, r, sz, &init_dot));
    if (hist && cap > 0) hist[0] = std::sqrt(init_dot);
    int st = SGPU_OK;
    if (solve_ends_at_start(h, "solve_pCG", init_dot, sz, iters, hist, cap, &st)) return st;
    CHK(vcycle0(h, rho, r, true));                                    // :2536-2537 (rho = 0, V-cycle)
    CHK(sgpu_vec_copy(p, rho, sz));
    const double THRSHLD = init_dot * h->prm.solver_tol * h->prm.solver_tol;
    current_dot = init_dot;
    // The scalars stay on the device (slots 4..7 of the scratch; slot 0 belongs to sgpu_dot, which the coarsest CG
    // of a V-cycle may call): S[a] = r.rho, S[5] = p.h, S[6] = r.r; alpha and beta are formed inside the
    // update kernels, so an iteration has ONE host synchronisation (the convergence test) instead of four.  The
    // reference's rho_res at the top of iteration i+1 (:2580) is the r.rho it computed for beta at the bottom of
    // iteration i (:2655) -- same vectors, same value -- so that dot is computed once.
    int a = 4, b = 7;
    CHK(dot_dev(r, rho, sz, a));                                      // :2580 (first iteration)
    int i = 0;
    for (i = 0; i < h->prm.solver_max_iter; i++) {                    // :2565
        CHK(sgpu_spmv(A, p, hh));                                     // :2571
        CHK(dot_dev(p, hh, sz, 5));                                   // :2581
        CHK(pcg_update_dev(a, 5, p, hh, u, r, sz, 6, &current_dot));  // alpha = rho_res / pdoth; :2593-2596; :2603
        if (hist && i + 1 < cap) hist[i + 1] = std::sqrt(current_dot);
        if (current_dot < THRSHLD) break;                             // :2620
        if (!std::isfinite(current_dot)) return nonfinite_stop("solve_pCG", i + 1, iters);
        CHK(vcycle0(h, rho, r, true));                                // :2640-2641 (rho = 0, V-cycle)
        CHK(dot_dev(r, rho, sz, b));                                  // :2655
        CHK(pcg_direction_dev(b, a, rho, p, sz));                     // beta = r.rho / rho_res; :2665-2667  p = rho + beta p
        std::swap(a, b);
    }
    if (h->null_space == 1) CHK(center_async(u, u, sz));              // the solution of zero mean
    const bool conv = current_dot < THRSHLD;
    if (i == h->prm.solver_max_iter) i--;
    if (iters) *iters = i + 1;
    return conv ? SGPU_OK : SGPU_ERR_NOCONV;
}

// saena_object::solve_CG (src/saena_object_solve.cpp:2119-2387): CG without a preconditioner (rho aliases r)
int sgpu_solve_CG(sgpu_amg *h, value_t *u, const value_t *rhs, int *iters, value_t *hist, int cap) {
    CHK(need_ctx());
    if (!h || !u || !rhs) return fail(SGPU_ERR_ARG, "null argument");
    sgpu_op *A = h->A[0];
    const size_t sz = (size_t)A->M;
    double *r = h->r, *hh = h->hh, *p = h->p;
    CHK(sgpu_vec_fill(u, 0.0, sz));
    CHK(sgpu_residual(A, u, rhs, r));
    if (h->null_space == 1) CHK(center_async(r, r, sz));
    double init_dot = 0, current_dot = 0;
    CHK(fetch_center_sum(h));
    CHK(sgpu_dot(r, r, sz, &init_dot));
    if (hist && cap > 0) hist[0] = std::sqrt(init_dot);
    int st = SGPU_OK;
    if (solve_ends_at_start(h, "solve_CG", init_dot, sz, iters, hist, cap, &st)) return st;
    CHK(sgpu_vec_copy(p, r, sz));
    const double THRSHLD = init_dot * h->prm.solver_tol * h->prm.solver_tol;
    current_dot = init_dot;
    // device-resident scalars as in solve_pCG: S[a] = r.r before the update (= rho_res), S[b] = r.r after it
    int a = 4, b = 7;
    CHK(dot_dev(r, r, sz, a));
    int i = 0;
    for (i = 0; i < h->prm.solver_max_iter; i++) {
        CHK(sgpu_spmv(A, p, hh));
        CHK(dot_dev(p, hh, sz, 5));
        CHK(pcg_update_dev(a, 5, p, hh, u, r, sz, b, &current_dot));
        if (hist && i + 1 < cap) hist[i + 1] = std::sqrt(current_dot);
        if (current_dot < THRSHLD) break;
        if (!std::isfinite(current_dot)) return nonfinite_stop("solve_CG", i + 1, iters);
        CHK(pcg_direction_dev(b, a, r, p, sz));                       // beta = current_dot / rho_res; p = r + beta p
        std::swap(a, b);
    }
    if (h->null_space == 1) CHK(center_async(u, u, sz));
    const bool conv = current_dot < THRSHLD;
    if (i == h->prm.solver_max_iter) i--;
    if (iters) *iters = i + 1;
    return conv ? SGPU_OK : SGPU_ERR_NOCONV;
}

// ---- bench.py safety net ----
static char  g_fatal_line[1 << 16];
static size_t g_fatal_len = 0;
static void fatal_handler(int sig) {
    if (g_fatal_len) { ssize_t r = write(1, g_fatal_line, g_fatal_len); (void)r; }
    char msg[64] = "libsaena_amd: fatal signal ";          // async-signal-safe: no stdio
    size_t n = strlen(msg);
    if (sig >= 10) msg[n++] = (char)('0' + sig / 10);
    msg[n++] = (char)('0' + sig % 10);
    msg[n++] = '\n';
    ssize_t r = write(2, msg, n); (void)r;
    _exit(128 + sig);                                     // the failure stays a failure for the launcher
}
int sgpu_debug_on_fatal_print(const char *line) {
    const int sigs[] = {SIGSEGV, SIGBUS, SIGABRT, SIGFPE, SIGILL};   // not SIGTERM: being told to stop is not a measured run
    if (!line) {
        for (int sg : sigs) signal(sg, SIG_DFL);
        g_fatal_len = 0;
        return SGPU_OK;
    }
    size_t n = strlen(line);
    if (n + 2 > sizeof g_fatal_line) return fail(SGPU_ERR_ARG, "line too long");
    memcpy(g_fatal_line, line, n);
    if (n && g_fatal_line[n - 1] != '\n') g_fatal_line[n++] = '\n';
    g_fatal_len = n;
    struct sigaction sa;
    memset(&sa, 0, sizeof sa);
    sa.sa_handler = fatal_handler;
    sigemptyset(&sa.sa_mask);
    for (int sg : sigs) sigaction(sg, &sa, nullptr);
    return SGPU_OK;
}

int sgpu_debug_device_info(char *buf, int len) {
    CHK(need_ctx());
    if (!buf || len < 2) return fail(SGPU_ERR_ARG, "bad argument");
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, g.device));
    snprintf(buf, (size_t)len, "%s (%s), %d CUs, %d MHz core, %d MHz memory x %d bit, L2 %d KiB, %.1f GiB", p.name, p.gcnArchName, p.multiProcessorCount,
             p.clockRate / 1000, p.memoryClockRate / 1000, p.memoryBusWidth, p.l2CacheSize / 1024, (double)p.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
    return SGPU_OK;
}

int sgpu_debug_chain_us(double *us) {
    CHK(need_ctx());
    if (!us) return fail(SGPU_ERR_ARG, "null argument");
    *us = g.chain_us;
    return SGPU_OK;
}

int sgpu_debug_exchange_mode(const sgpu_op *op, int *mode) {
    CHK(need_ctx());
    if (!op || !mode) return fail(SGPU_ERR_ARG, "null argument");
    *mode = exchange_mode(op, false);
    return SGPU_OK;
}

int sgpu_debug_op_storage(const sgpu_op *op, unsigned *group_mask, long long *live_bytes) {
    if (!group_mask || !live_bytes) return fail(SGPU_ERR_ARG, "null argument");
    *group_mask = op ? part_storage_mask(op->loc) : 0;
    *live_bytes = (long long)devmem::live_bytes.load();
    return SGPU_OK;
}

int sgpu_debug_launch_count(long *launches) {
    if (!launches) return fail(SGPU_ERR_ARG, "null argument");
    *launches = g_launches;
    return SGPU_OK;
}

int sgpu_debug_allow_local_only(sgpu_op *op, int allow) {
    if (!op) return fail(SGPU_ERR_ARG, "null op");
    op->local_only_ok = allow != 0;
    return SGPU_OK;
}

// ---- measurement ----
int sgpu_algorithmic_bytes(const sgpu_op *op, int kind, int64_t *bytes) {
    if (!op || !bytes) return fail(SGPU_ERR_ARG, "null argument");
    const int64_t M = op->M, N = op->N_local, nnz = op->loc.nnz + op->rem.nnz;
    int64_t b = 12 * nnz + 4 * (M + 1) + 8 * N + 8 * M;     // B_spmv, BASELINE.md section 3
    if (kind == 1) b += 16 * M;                             // jacobi: rhs, inv_diag
    else if (kind == 2) b += 8 * M;                         // residual: rhs
    else if (kind == 3) b += 32 * M;                        // chebyshev step: rhs, inv_diag, d r/w
    *bytes = b;
    return SGPU_OK;
}

int sgpu_time_kernel(sgpu_op *op, int kind, const value_t *x, const value_t *rhs, value_t *y, int reps, float *ms) {
    CHK(need_ctx());
    if (!op || !x || !y || !ms || reps < 1) return fail(SGPU_ERR_ARG, "bad argument");
    if (kind != 0 && !rhs) return fail(SGPU_ERR_ARG, "rhs needed");
    if ((kind == 1 || kind == 3) && !op->inv_diag) return fail(SGPU_ERR_ARG, "operator has no inv_diag");
    if (kind == 3) CHK(ensure_d(op));
    return time_reps(reps, ms, [&]() -> int {
        EpiArgs e; e.rhs = rhs; e.inv_diag = op->inv_diag; e.u = x; e.d = op->dvec;
        int epi = sk::EPI_SPMV;
        if (kind == 1) { epi = sk::EPI_JACOBI; e.c0 = JACOBI_OMEGA_REF; }
        else if (kind == 2) epi = sk::EPI_RESIDUAL;
        else if (kind == 3) { epi = sk::EPI_CHEBYK; e.c0 = 0.5; e.c1 = 0.25; }
        return apply(op, epi, x, y, e);
    });
}

} // extern "C"

#include "sgpu_block.hip.inc"
#include "sgpu_gmres.hip.inc"
#include "sgpu_eig.hip.inc"
#include "sgpu_eig_lock.hip.inc"
#include "sgpu_lanczos.hip.inc"
#include "sgpu_coarse_cg.hip.inc"

// sgpu_amg_set_operator (include/saena_gpu.h).  After the block helpers: the block work space of a hierarchy keeps a Chebyshev
// direction per operator and K, which the incoming operator does not have yet.
extern "C" int sgpu_amg_set_operator(sgpu_amg *h, int level, sgpu_op *A_new, value_t eig_max) {
    CHK(need_ctx());
    if (!h || !A_new) return fail(SGPU_ERR_ARG, "sgpu_amg_set_operator: null argument");
    if (g.nranks > 1 || g.multi()) return fail(SGPU_ERR_ARG, "sgpu_amg_set_operator: runs on one rank only (this context has %d)", g.nranks);
    if (level < 0 || level >= h->nlevels) return fail(SGPU_ERR_ARG, "sgpu_amg_set_operator: level %d is outside 0..%d", level, h->nlevels - 1);
    const bool coarsest = level == h->nlevels - 1;
    if (A_new->M != A_new->N_local) return fail(SGPU_ERR_ARG, "sgpu_amg_set_operator: the operator is not square (%d x %d)", A_new->M, A_new->N_local);
    if (A_new->M != h->A[level]->M) return fail(SGPU_ERR_ARG, "sgpu_amg_set_operator: the operator has %d rows, level %d has %d", A_new->M, level, h->A[level]->M);
    if (A_new->has_remote || A_new->recvSize || A_new->vIndexSize) return fail(SGPU_ERR_ARG, "sgpu_amg_set_operator: the operator has a remote part; runs on one rank only");
    if (!coarsest && !A_new->inv_diag && A_new->M > 0) return fail(SGPU_ERR_ARG, "sgpu_amg_set_operator: the operator has no inv_diag");
    if (!coarsest && h->prm.smoother == 1 && !(eig_max > 0.0)) return fail(SGPU_ERR_ARG, "sgpu_amg_set_operator: chebyshev needs eig_max > 0");
    // a hierarchy that knows the constant null space: the incoming operator of level 0 or of the coarsest level must annihilate constants too
    if (h->null_space == 1 && (level == 0 || coarsest)) CHK(null_defect_check(A_new, level, "sgpu_amg_set_operator"));
    // nothing in flight, then no captured launch that names the outgoing operator's arrays
    HIPCHK(hipStreamSynchronize(g.cs));
    HIPCHK(hipStreamSynchronize(g.hs));
    h->drop_graphs();
    // everything that can fail, aside
    DevArr<double> Ainv;
    const bool direct = coarsest && h->prm.coarse_solver == 1 && h->coarse_local && A_new->M > 0 && !(A_new->M > sk::CG_MAXN);
    if (direct) {
        if (A_new->h_val.size() != A_new->loc.h_col.size()) return fail(SGPU_ERR_ARG, "sgpu_amg_set_operator: the operator keeps no host copy of its values to factor");
        std::vector<double> inv;
        CHK(dense_inverse(A_new, inv, h->null_space == 1));
        CHK(dev_upload(Ainv, inv.data(), inv.size()));
    }
    if (coarsest && h->coarse_device_cg && A_new->M > sk::CG_MAXN) CHK(ensure_dcg(h, A_new->M));    // (kept: the row count is the outgoing operator's)
    // what a capture must not allocate: the Chebyshev direction (scalar, and per K of every block work space that exists)
    if (!coarsest && h->prm.smoother == 1) CHK(ensure_d(A_new));
    for (int K : {2, 4, 8})
        if (h->blk[block_slot(K)]) { CHK(ensure_blk_d(A_new, K)); CHK(ensure_blk_halo(A_new, K)); }
    // commit
    if (direct) h->Ainv = std::move(Ainv);
    h->A[(size_t)level] = A_new;
    h->eig[(size_t)level] = eig_max;
    return SGPU_OK;
}

// ===========================================================================
// Setup-time collectives of the host layer over the same RCCL communicator
// (the reference: MPI_Alltoall/Alltoallv/Allreduce/Allgather during assemble).
namespace {
struct RcclHostComm : saena_host::Comm {
    static void ok(int s, const char *what) { if (s != SGPU_OK) throw std::runtime_error(std::string(what) + ": " + g_err); }
    struct Buf {
        DevArr<char> arr;
        void *p = nullptr;
        explicit Buf(size_t n) { if (arr.alloc(std::max<size_t>(n, 8)) != hipSuccess) throw std::runtime_error("hipMalloc failed in RcclHostComm"); p = arr.get(); }
    };
    static int h2d(void *d, const void *h, size_t n) { if (n) HIPCHK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, g.cs)); return SGPU_OK; }
    static int d2h(void *h, const void *d, size_t n) {
        if (n) HIPCHK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        return SGPU_OK;
    }
    static int do_allgather(const void *ds, void *dr, size_t bytes) { NCCLCHK(ncclAllGather(ds, dr, bytes, ncclChar, g.comm, g.cs)); return SGPU_OK; }
    int do_alltoallv(const char *ds, const size_t *sc, const size_t *sd, char *dr, const size_t *rc, const size_t *rd) {
        NCCLCHK(ncclGroupStart());
        for (int p = 0; p < nranks; ++p) {
            if (p == rank) continue;
            if (sc[p]) NCCLCHK(ncclSend(ds + sd[p], sc[p], ncclChar, p, g.comm, g.cs));
            if (rc[p]) NCCLCHK(ncclRecv(dr + rd[p], rc[p], ncclChar, p, g.comm, g.cs));
        }
        NCCLCHK(ncclGroupEnd());
        if (sc[rank]) HIPCHK(hipMemcpyAsync(dr + rd[rank], ds + sd[rank], sc[rank], hipMemcpyDeviceToDevice, g.cs));
        return SGPU_OK;
    }
    template <class T>
    static int do_allreduce(T *d, int n, ncclDataType_t t) { NCCLCHK(ncclAllReduce(d, d, (size_t)n, t, ncclSum, g.comm, g.cs)); return SGPU_OK; }

    void allgather(const void *send, void *recv, size_t bytes) override {
        if (!g.comm) { memcpy(recv, send, bytes); return; }
        Buf s(bytes), r(bytes * nranks);
        ok(h2d(s.p, send, bytes), "allgather h2d");
        ok(do_allgather(s.p, r.p, bytes), "ncclAllGather");
        ok(d2h(recv, r.p, bytes * nranks), "allgather d2h");
    }
    void alltoallv(const void *send, const size_t *sc, const size_t *sd, void *recv, const size_t *rc, const size_t *rd) override {
        size_t sbytes = 0, rbytes = 0;
        for (int p = 0; p < nranks; ++p) { sbytes = std::max(sbytes, sd[p] + sc[p]); rbytes = std::max(rbytes, rd[p] + rc[p]); }
        if (!g.comm) { memcpy(static_cast<char *>(recv) + rd[0], static_cast<const char *>(send) + sd[0], sc[0]); return; }
        Buf s(sbytes), r(rbytes);
        ok(h2d(s.p, send, sbytes), "alltoallv h2d");
        ok(do_alltoallv(static_cast<const char *>(s.p), sc, sd, static_cast<char *>(r.p), rc, rd), "alltoallv send/recv");
        ok(d2h(recv, r.p, rbytes), "alltoallv d2h");
    }
    void allreduce_sum_i64(long *v, int n) override {
        if (!g.comm || n == 0) return;
        Buf b(sizeof(long) * n);
        ok(h2d(b.p, v, sizeof(long) * n), "allreduce h2d");
        ok(do_allreduce(static_cast<long *>(b.p), n, ncclInt64), "ncclAllReduce");
        ok(d2h(v, b.p, sizeof(long) * n), "allreduce d2h");
    }
    void allreduce_sum_f64(double *v, int n) override {
        if (!g.comm || n == 0) return;
        Buf b(sizeof(double) * n);
        ok(h2d(b.p, v, sizeof(double) * n), "allreduce h2d");
        ok(do_allreduce(static_cast<double *>(b.p), n, ncclDouble), "ncclAllReduce");
        ok(d2h(v, b.p, sizeof(double) * n), "allreduce d2h");
    }
};
} // namespace

extern "C" int sgpu_context_device() { return g.device; }

extern "C" saena_host::Comm *sgpu_new_host_comm() {
    if (!g.live) return nullptr;
    auto *c = new RcclHostComm();
    c->rank = g.rank; c->nranks = g.nranks;
    return c;
}
