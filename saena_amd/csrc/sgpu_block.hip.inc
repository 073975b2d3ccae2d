// sgpu_block.hip.inc -- block entry points of include/saena_gpu.h (sgpu_*_block): K right-hand sides through one pass over
// every operator.  Part of sgpu_runtime.hip (it shares that file's context, handles and helpers); kernels: kernels_block.hip.h.
//
// Nothing here touches the scalar path: no plan, no autotune choice, no plan-cache entry, no scalar graph.  The block kernel
// reads the plain CSR arrays every operator keeps for its whole life (CsrPart::row_ptr / col / val and the 16 KiB row-block
// plan blk_row); its own state is two lane counts and two lazily made buffers per K and operator, and an AmgBlock per (hierarchy, K).
// Across ranks (a communicator or a host transport) the K columns of an operator's halo cross in ONE exchange: apply_block mirrors
// apply()'s plain orderings with block halo buffers per K and operator, and the dots of the block pCG are summed over the ranks.
namespace {

uint64_t g_block_generation = 0;   // bumped by sgpu_op_set_block_lanes: captured BLOCK V-cycles are stale (the scalar ones are not)

int block_slot(int K) { return K == 2 ? 0 : K == 4 ? 1 : 2; }

// K, and -- with an operator -- that its halo can be fetched: through the context's communicator or host transport, or from a block
// halo a test injected for this K.  The same answer on every rank of a context (a refusal on one rank alone would leave the
// others waiting in the exchange): K is the caller's on all of them, and a context with a transport refuses no operator here.
int block_check(const sgpu_op *op, int K, const char *what) {
    if (K != 2 && K != 4 && K != 8) return fail(SGPU_ERR_ARG, "%s: a block holds 2, 4 or 8 columns (K = %d)", what, K);
    if (op && (op->has_remote || op->recvSize) && !g.multi() && !op->injected_blk[block_slot(K)])
        return fail(SGPU_ERR_ARG, "%s: the operator has a remote part (%d halo entries), and this context has neither a communicator nor a host transport "
                    "and no block halo was injected for K = %d", what, op->recvSize, K);
    return SGPU_OK;
}
// what stays on one rank (LOBPCG; FGMRES has gmres_check): no communicator, no host transport, no operator with a remote part
int block_one_rank_check(const sgpu_op *op, int K, const char *what) {
    CHK(block_check(nullptr, K, what));
    if (g.nranks > 1 || g.multi()) return fail(SGPU_ERR_ARG, "%s: runs on one rank only (this context has %d)", what, g.nranks);
    if (op && (op->has_remote || op->recvSize))
        return fail(SGPU_ERR_ARG, "%s: the operator has a remote part (%d halo entries); it takes single-rank operators only", what, op->recvSize);
    return SGPU_OK;
}

// lanes per row from the mean row length: a row block holds up to CAP = 2048 entries for 256 lanes, 8 entries per lane
int block_auto_lanes(const sgpu_op *op) {
    const double mean = op->M > 0 ? (double)op->loc.nnz / (double)op->M : 0.0;
    for (int G : {1, 4, 16})
        if ((double)G * 8.0 >= mean) return G;
    return 64;
}

using BlockFn = void (*)(const sk::BlockArgs);
// K columns in {2, 4, 8}; G lanes per row in {1, 4, 16}, anything else 64 (the pickers of sgpu_runtime.hip)
BlockFn pick_block(int K, int epi, int G) {
    return among<2, 4, 8>(K, [&](auto KK) { return per_epi_no_rsweep(epi, [&](auto E) { return among<1, 4, 16, 64>(G == 1 || G == 4 || G == 16 ? G : 64, [&](auto GG) -> BlockFn {
        return sk::k_csr_block<KK(), E(), GG()>; }); }); });
}

using BlockBndFn = void (*)(const sk::BlockBoundaryArgs);
BlockBndFn pick_block_bnd(int K, int epi, int G) {
    return among<2, 4, 8>(K, [&](auto KK) { return per_epi_no_rsweep(epi, [&](auto E) { return among<1, 4, 16, 64>(G == 1 || G == 4 || G == 16 ? G : 64, [&](auto GG) -> BlockBndFn {
        return sk::k_csr_boundary_block<KK(), E(), GG()>; }); }); });
}

int block_lanes_of(sgpu_op *op) {
    if (!op->block_lanes_auto) op->block_lanes_auto = block_auto_lanes(op);
    return op->block_lanes ? op->block_lanes : op->block_lanes_auto;
}

sk::BlockArgs block_args(const sgpu_op *op, const double *x, double *y, const EpiArgs &e) {
    sk::BlockArgs a;
    a.row_ptr = op->loc.csr.row_ptr; a.col = op->loc.csr.col; a.val = op->loc.csr.val; a.blk_row = op->loc.csr.blk_row; a.nblk = op->loc.nblk;
    a.x = x; a.y = y; a.rhs = e.rhs; a.inv_diag = e.inv_diag; a.u = e.u; a.d = e.d; a.c0 = e.c0; a.c1 = e.c1;
    a.skip = nullptr;
    return a;
}

// the block halo buffers of an operator for K columns: made once, at the first block apply with that K (never inside a graph
// capture: amg_block makes those of a hierarchy before its first V-cycle)
int ensure_blk_halo(sgpu_op *op, int K) {
    const int s = block_slot(K);
    if (op->blk_halo_made[s] || !(op->vIndexSize || op->recvSize)) return SGPU_OK;
    const size_t ns = (size_t)op->vIndexSize * K, nr = (size_t)op->recvSize * K;
    if (ns && op->send_blk[s].alloc(ns) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of a block send buffer (%d entries x %d columns) failed", op->vIndexSize, K);
    if (nr) {
        if (op->recv_blk[s].alloc(nr) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of a block receive buffer (%d entries x %d columns) failed", op->recvSize, K);
        // on cs and waited for: a memset of device memory on the null stream returns before it has run, and neither cs nor hs (both
        // non-blocking) waits for that stream -- it could land on top of the first exchange or of an injected halo
        HIPCHK(hipMemsetAsync(op->recv_blk[s], 0, nr * sizeof(double), g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
    }
    if (op->halo_fp32 && g.multi()) {
        if (ns && op->send_blk_f[s].alloc(ns) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of a block send buffer (float wire) failed");
        if (nr && op->recv_blk_f[s].alloc(nr) != hipSuccess) return fail(SGPU_ERR_NOMEM, "hipMalloc of a block receive buffer (float wire) failed");
    }
    op->blk_halo_made[s] = true;
    return SGPU_OK;
}

// rows without remote entries (all rows of an operator without a remote part): k_csr_block over the 16 KiB row-block plan on cs
int launch_block_interior(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e, int K) {
    if (op->M == 0 || op->loc.nblk == 0) return SGPU_OK;
    const BlockFn fn = pick_block(K, epi, block_lanes_of(op));
    if (!fn) return fail(SGPU_ERR_ARG, "block apply: no kernel for epilogue %d", epi);   // a missing kernel is an error, never a fall-back
    sk::BlockArgs a = block_args(op, x, y, e);
    a.skip = op->has_remote ? (const unsigned *)op->skip : nullptr;
    SGPU_LAUNCH(fn, dim3(op->loc.nblk), dim3(sk::BLOCK), 0, g.cs, a);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// the rows that own remote entries, whole (local + halo products, one epilogue), once the block halo has arrived
int launch_block_boundary(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e, int K, bool halo_is_f32, hipStream_t stream) {
    if (!op->has_remote || op->rem.nrows == 0) return SGPU_OK;
    const int G = block_lanes_of(op), s = block_slot(K);
    const BlockBndFn fn = pick_block_bnd(K, epi, G);
    if (!fn) return fail(SGPU_ERR_ARG, "block apply: no boundary kernel for epilogue %d", epi);
    sk::BlockBoundaryArgs b;
    b.b = block_args(op, x, y, e);
    b.rows = op->rem.csr.rows; b.nrows = op->rem.nrows;
    b.h_ptr = op->rem.csr.row_ptr; b.h_col = op->rem.csr.col; b.h_val = op->rem.csr.val;
    b.halo = op->recv_blk[s]; b.halo_f = halo_is_f32 ? (const float *)op->recv_blk_f[s] : nullptr;
    const int eg = G == 1 || G == 4 || G == 16 ? G : 64, rpb = sk::BLOCK / eg;
    SGPU_LAUNCH(fn, dim3((b.nrows + rpb - 1) / rpb), dim3(sk::BLOCK), 0, stream, b);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// send[t * K + j] = X[vIndex[t] * K + j] into the operator's block send buffer (the float one on an fp32 wire)
int pack_block(sgpu_op *op, const double *x, int K, bool f32, int as_float, hipStream_t stream) {
    if (!op->vIndexSize) return SGPU_OK;
    const int s = block_slot(K);
    const size_t pairs = (size_t)op->vIndexSize * (K / 2);
    const dim3 grid((unsigned)std::min<size_t>(sk::PACK_MAX_BLOCKS, (pairs + sk::BLOCK - 1) / sk::BLOCK));
    among<2, 4, 8>(K, [&](auto KK) {
        if (f32) SGPU_LAUNCH(sk::k_pack_block_f32<KK()>, grid, dim3(sk::BLOCK), 0, stream, x, (const int *)op->vIndex, op->send_blk_f[s].get(), op->vIndexSize);
        else SGPU_LAUNCH(sk::k_pack_block<KK()>, grid, dim3(sk::BLOCK), 0, stream, x, (const int *)op->vIndex, op->send_blk[s].get(), op->vIndexSize, as_float);
        return 0;
    });
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// exchange_group for a block: the same neighbours in the same order, every segment K times as long
int exchange_group_block(sgpu_op *op, int K, bool f32, hipStream_t st) {
    const int s = block_slot(K);
    const size_t k = (size_t)K;
    NCCLCHK(ncclGroupStart());
    for (size_t i = 0; i < op->sendRank.size(); ++i) {
        if (f32) NCCLCHK(ncclSend(op->send_blk_f[s] + op->sendDispl[i] * k, op->sendCount[i] * k, ncclFloat, op->sendRank[i], g.comm, st));
        else NCCLCHK(ncclSend(op->send_blk[s] + op->sendDispl[i] * k, op->sendCount[i] * k, ncclDouble, op->sendRank[i], g.comm, st));
    }
    for (size_t i = 0; i < op->recvRank.size(); ++i) {
        if (f32) NCCLCHK(ncclRecv(op->recv_blk_f[s] + op->recvDispl[i] * k, op->recvCount[i] * k, ncclFloat, op->recvRank[i], g.comm, st));
        else NCCLCHK(ncclRecv(op->recv_blk[s] + op->recvDispl[i] * k, op->recvCount[i] * k, ncclDouble, op->recvRank[i], g.comm, st));
    }
    NCCLCHK(ncclGroupEnd());
    ++g_launches;
    return SGPU_OK;
}

// apply_host_transport for a block: pack -> host -> callback (its counts x K, the same element size) -> device, then the interior
// and the boundary rows, all on cs
int apply_block_host_transport(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e, int K) {
    const bool f32 = op->halo_fp32 != 0;
    const int s = block_slot(K);
    const size_t eb = f32 ? sizeof(float) : sizeof(double);
    std::vector<char> hs((size_t)op->vIndexSize * K * eb), hr((size_t)op->recvSize * K * eb);
    std::vector<int> sc(op->sendCount), rc(op->recvCount);
    for (int &c : sc) c *= K;
    for (int &c : rc) c *= K;
    if (op->vIndexSize) {
        CHK(pack_block(op, x, K, f32, 0, g.cs));
        HIPCHK(hipMemcpyAsync(hs.data(), f32 ? (const void *)op->send_blk_f[s] : (const void *)op->send_blk[s], hs.size(), hipMemcpyDeviceToHost, g.cs));
    }
    HIPCHK(hipStreamSynchronize(g.cs));
    if (g.xchg(g.xuser, hs.data(), op->sendRank.data(), sc.data(), (int)op->sendRank.size(),
               hr.data(), op->recvRank.data(), rc.data(), (int)op->recvRank.size(), (int)eb) != 0)
        return fail(SGPU_ERR_RCCL, "host transport: exchange callback failed");
    if (op->recvSize) HIPCHK(hipMemcpyAsync(f32 ? (void *)op->recv_blk_f[s] : (void *)op->recv_blk[s], hr.data(), hr.size(), hipMemcpyHostToDevice, g.cs));
    CHK(launch_block_interior(op, epi, x, y, e, K));
    CHK(launch_block_boundary(op, epi, x, y, e, K, f32, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));                  // the staging vectors die with this frame
    return SGPU_OK;
}

// Y = epilogue(A X).  Without a halo: one launch of k_csr_block over the operator's 16 KiB row-block plan.  With one, apply()'s
// plain orderings (sgpu_runtime.hip), the K columns through ONE exchange chain:
//   host transport   apply_host_transport's sequence;
//   S (one stream)   pack -> grouped send/recv -> interior rows (k_csr_block with the skip mask) -> boundary rows, all on cs;
//   E (two streams)  interior rows on cs; pack, send/recv group and boundary rows on hs; ev_x and ev_halo order the two.
// No flag is polled and no stream value op is used here: nothing this path enqueues waits on a launch the host has yet to make.
// A rank takes part in the exchange whenever it has a neighbour, whether or not it has rows to launch for.
int apply_block(sgpu_op *op, int epi, const double *x, double *y, const EpiArgs &e, int K) {
    const bool halo = op->vIndexSize || op->recvSize;
    if (!halo) return launch_block_interior(op, epi, x, y, e, K);
    const int s = block_slot(K);
    // the block kernels read the plain CSR of both parts and the boundary mask, whatever form the scalar path is on (the dense
    // variant included); never the local part alone
    if (op->has_remote && (!op->loc.csr.row_ptr || !op->rem.csr.row_ptr || !op->rem.csr.rows || !op->skip))
        return fail(SGPU_ERR_STATE, "block apply: the operator does not hold the CSR arrays of its boundary rows");
    CHK(ensure_blk_halo(op, K));
    const bool inj = op->injected_blk[s];
    if (g.xchg && !inj) return apply_block_host_transport(op, epi, x, y, e, K);
    if (!g.comm || inj) {
        if (op->has_remote && !inj)
            return fail(SGPU_ERR_ARG, "block apply: the operator has a remote part (%d halo entries) and nothing to fetch it with", op->recvSize);
        CHK(launch_block_interior(op, epi, x, y, e, K));     // halo supplied by the caller (tests): same kernels, one stream
        return launch_block_boundary(op, epi, x, y, e, K, false, g.cs);
    }
    const bool f32 = op->halo_fp32 != 0;                 // both ends of a link must agree: the flag alone decides the wire type
    if (op->single_stream) {
        CHK(pack_block(op, x, K, f32, 0, g.cs));
        CHK(exchange_group_block(op, K, f32, g.cs));
        CHK(launch_block_interior(op, epi, x, y, e, K));
        return launch_block_boundary(op, epi, x, y, e, K, f32, g.cs);
    }
    // (RCCL connects a peer at the first exchange with it; the scalar path keeps its polling orderings off that one: tell it)
    if (g.peer_seen.size() != (size_t)g.nranks) g.peer_seen.assign((size_t)g.nranks, 0);
    for (int r : op->sendRank) g.peer_seen[(size_t)r] |= 1;
    for (int r : op->recvRank) g.peer_seen[(size_t)r] |= 2;
    HIPCHK(hipEventRecord(op->ev_x, g.cs));
    CHK(launch_block_interior(op, epi, x, y, e, K));
    HIPCHK(hipStreamWaitEvent(g.hs, op->ev_x, 0));
    CHK(pack_block(op, x, K, f32, 0, g.hs));
    CHK(exchange_group_block(op, K, f32, g.hs));
    CHK(launch_block_boundary(op, epi, x, y, e, K, f32, g.hs));
    // join: nothing later on cs may see y (or overwrite x and the send buffers) before hs is through
    HIPCHK(hipEventRecord(op->ev_halo, g.hs));
    HIPCHK(hipStreamWaitEvent(g.cs, op->ev_halo, 0));
    return SGPU_OK;
}

// the operator's block ping-pong buffer (the op-level smoother calls; a block V-cycle ping-pongs in its own work vectors) and its
// Chebyshev direction for K columns: made when first needed, each on its own
int ensure_blk_buf(DevArr<double> &p, const sgpu_op *op, int K) {
    if (p) return SGPU_OK;
    if (alloc_vec(p, (size_t)op->M * K) != hipSuccess)
        return fail(SGPU_ERR_NOMEM, "hipMalloc of a block work vector (%d rows x %d columns) failed", op->M, K);
    return SGPU_OK;
}
int ensure_blk_tmp(sgpu_op *op, int K) { return ensure_blk_buf(op->tmp_blk[block_slot(K)], op, K); }
int ensure_blk_d(sgpu_op *op, int K) { return ensure_blk_buf(op->dvec_blk[block_slot(K)], op, K); }

// jacobi_pp / cheby_pp on block vectors (no zero-iterate shortcut: a sweep from a zero-filled block gives the same numbers)
int jacobi_block_pp(sgpu_op *op, int iter, double omega, double *u, double *alt, const double *rhs, double **out, int K) {
    if (!op->inv_diag && op->M > 0) return fail(SGPU_ERR_ARG, "jacobi: operator has no inv_diag");
    double *cur = u, *nxt = alt;
    for (int j = 0; j < iter; ++j) {
        EpiArgs e; e.rhs = rhs; e.inv_diag = op->inv_diag; e.u = cur; e.c0 = omega;
        CHK(apply_block(op, sk::EPI_JACOBI, cur, nxt, e, K));
        std::swap(cur, nxt);
    }
    *out = cur;
    return SGPU_OK;
}
int cheby_block_pp(sgpu_op *op, int iter, double eig_max, double *u, double *alt, const double *rhs, double **out, int K) {
    if (!op->inv_diag && op->M > 0) return fail(SGPU_ERR_ARG, "chebyshev: operator has no inv_diag");
    const double alpha = 0.13 * eig_max, beta = eig_max;                          // cheby_pp's scalars
    const double delta = (beta - alpha) / 2.0, theta = (beta + alpha) / 2.0;
    const double s1 = theta / delta, twos1 = 2.0 * s1;
    double rhok = 1.0 / s1;
    double *cur = u, *nxt = alt;
    for (int i = 0; i < iter; ++i) {
        EpiArgs e; e.rhs = rhs; e.inv_diag = op->inv_diag; e.u = cur; e.d = op->dvec_blk[block_slot(K)];
        if (i == 0) { e.c0 = 1.0 / theta; CHK(apply_block(op, sk::EPI_CHEBY0, cur, nxt, e, K)); }
        else {
            const double rhokp1 = 1.0 / (twos1 - rhok);
            const double two_rhokp1 = 2.0 * rhokp1;
            e.c1 = rhokp1 * rhok; e.c0 = two_rhokp1 / delta;
            rhok = rhokp1;
            CHK(apply_block(op, sk::EPI_CHEBYK, cur, nxt, e, K));
        }
        std::swap(cur, nxt);
    }
    *out = cur;
    return SGPU_OK;
}

int block_pack(const double *cols, double *blk, size_t n, int K) {
    if (!n) return SGPU_OK;
    SGPU_LAUNCH(sk::k_block_pack, dim3(grid_for(2 * n)), dim3(sk::BLOCK), 0, g.cs, cols, blk, n, K);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}
int block_unpack(const double *blk, double *cols, size_t n, int K) {
    if (!n) return SGPU_OK;
    SGPU_LAUNCH(sk::k_block_unpack, dim3(grid_for(2 * n)), dim3(sk::BLOCK), 0, g.cs, blk, cols, n, K);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// Y = X - the column means of X, n rows of K interleaved columns (Y may be X): center_async per column -- the sums on the dot's grid,
// one workgroup per column for the partial sums, the subtraction.  Column j gets the bits of the scalar kernels on that column alone
int center_block_async(const double *X, double *Y, size_t n, int K) {
    if (n == 0) return SGPU_OK;
    const int nb = dot_nblocks(n), gd = grid_for(2 * n);
    double *part = g.cblk, *S = g.cblk + (size_t)g.n_partials * 8;
    SGPU_LAUNCH_COLS("k_sum_block_partial", K, per_K(K, [](auto k) { return sk::k_sum_block_partial<k()>; }), dim3(nb), dim3(sk::BLOCK), 0, g.cs, X, n, part);
    SGPU_LAUNCH(sk::k_reduce_partials_block, dim3(K), dim3(sk::BLOCK), 0, g.cs, (const double *)part, nb, K, S, (1u << K) - 1u);
    SGPU_LAUNCH_COLS("k_center_block", K, per_K(K, [](auto k) { return sk::k_center_block<k()>; }), dim3(gd), dim3(sk::BLOCK), 0, g.cs, (const double *)S, X, Y, n);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// ---- per-(hierarchy, K) state ----
int amg_block(sgpu_amg *h, int K, AmgBlock **out) {
    const int slot = block_slot(K);
    if (!h->blk[slot]) {
        std::unique_ptr<AmgBlock> B(new AmgBlock());
        B->K = K;
        const int L = h->nlevels;
        B->res.resize(L); B->rhs.resize(L); B->u.resize(L); B->alt.resize(L);
        for (int l = 0; l < L; ++l) {
            const size_t n = (size_t)h->A[l]->M * K;
            if (l < L - 1) HIPCHK(alloc_vec(B->res[l], n));
            if (l >= 1) { HIPCHK(alloc_vec(B->rhs[l], n)); HIPCHK(alloc_vec(B->u[l], n)); HIPCHK(alloc_vec(B->alt[l], n)); }
            CHK(ensure_blk_d(h->A[l], K));                     // (Chebyshev direction) no allocation may happen inside a graph capture
            CHK(ensure_blk_halo(h->A[l], K));                  // nor after the first collective of a solve: the halo buffers of every level
            if (l < L - 1) { CHK(ensure_blk_halo(h->P[l], K)); CHK(ensure_blk_halo(h->R[l], K)); }
        }
        const size_t n0 = (size_t)h->A[0]->M * K;
        HIPCHK(alloc_vec(B->alt0, n0)); HIPCHK(alloc_vec(B->r, n0)); HIPCHK(alloc_vec(B->rho, n0)); HIPCHK(alloc_vec(B->hh, n0)); HIPCHK(alloc_vec(B->p, n0));
        HIPCHK(alloc_vec(B->cm, 2 * (size_t)h->A[L - 1]->M * K));
        HIPCHK(alloc_vec(B->S, 8 * (size_t)K));              // (rows 0 and 1: where the dots of a multi-rank solve are summed over the ranks)
        HIPCHK(alloc_vec(B->partials, (size_t)g.n_partials * K));
        HIPCHK(B->hS.alloc(K));
        h->blk[slot] = std::move(B);
    }
    AmgBlock *B = h->blk[slot].get();
    *out = B;
    return SGPU_OK;
}

int amg_block_check(sgpu_amg *h, int K, const char *what) {
    CHK(block_check(nullptr, K, what));
    // (both flags are the same on every rank: sgpu_amg_create sums them over the ranks)
    if (!h->coarse_local) return fail(SGPU_ERR_ARG, "%s: the coarsest level is row-partitioned over the ranks and needs the distributed CG; block solves take hierarchies whose coarsest level lives on one rank", what);
    if (h->coarse_host_driven) return fail(SGPU_ERR_ARG, "%s: the coarsest level has %d rows and needs the host-driven CG; block solves take hierarchies whose coarsest level fits the LDS-resident solvers (<= %d rows)", what, h->A[h->nlevels - 1]->M, sk::CG_MAXN);
    for (int l = 0; l < h->nlevels; ++l) {
        CHK(block_check(h->A[l], K, what));
        if (l < h->nlevels - 1) { CHK(block_check(h->P[l], K, what)); CHK(block_check(h->R[l], K, what)); }
    }
    return SGPU_OK;
}

int coarse_solve_block(sgpu_amg *h, AmgBlock &B, double *u, const double *rhs, bool u_zero) {
    sgpu_op *A = h->A[h->nlevels - 1];
    const int n = A->M, K = B.K;
    if (n == 0) return SGPU_OK;
    if (h->Ainv) {
        const int C = std::min(K, pow2floor(std::max(1, sk::DS_CAP / n)));
        SGPU_LAUNCH_COLS("k_dense_solve_block", C, (among<1, 2, 4, 8>(C, [](auto c) { return sk::k_dense_solve_block<c()>; })), dim3(1), dim3(sk::CG_BLOCK), 0, g.cs,
                         (const double *)h->Ainv, rhs, u, n, K);
        HIPCHK(hipGetLastError());
        return SGPU_OK;
    }
    // LDS-resident CG: the existing one-workgroup solver, column by column (<= 1024 rows: not a hot path)
    double *crhs = B.cm, *cu = B.cm + (size_t)n * K;
    CHK(block_unpack(rhs, crhs, (size_t)n, K));
    if (u_zero) CHK(sgpu_vec_fill(cu, 0.0, (size_t)n * K)); else CHK(block_unpack(u, cu, (size_t)n, K));
    // the constant null space: every unpacked column centred in place by the scalar kernels, as coarse_solve does for one column
    if (h->null_space == 1) for (int j = 0; j < K; ++j) CHK(center_async(crhs + (size_t)j * n, crhs + (size_t)j * n, (size_t)n));
    // the device CG past CG_MAXN rows (coarse_solver == 2): the scalar solver again, so a column has the bits of its scalar solve
    const bool dev = h->coarse_device_cg && n > sk::CG_MAXN;
    for (int j = 0; j < K; ++j) CHK(dev ? coarse_cg_device(h, A, cu + (size_t)j * n, crhs + (size_t)j * n, nullptr)
                                        : coarse_cg_single(h, A, cu + (size_t)j * n, crhs + (size_t)j * n, nullptr));
    return block_pack(cu, u, (size_t)n, K);
}

int smooth_block_pp(sgpu_amg *h, int l, int iter, double *u, double *alt, const double *rhs, double **out, int K) {
    if (h->prm.smoother == 0) {
        const double om = h->prm.jacobi_omega != 0.0 ? h->prm.jacobi_omega : JACOBI_OMEGA_REF;
        return jacobi_block_pp(h->A[l], iter, om, u, alt, rhs, out, K);
    }
    return cheby_block_pp(h->A[l], iter, h->eig[l], u, alt, rhs, out, K);
}

// vcycle_level on block vectors, step for step (without its two launch-saving shortcuts, whose results are the plain sweep's)
int vcycle_block_level(sgpu_amg *h, AmgBlock &B, int l, double *u, double *alt, const double *rhs, double **out, bool u_zero) {
    const int K = B.K;
    const size_t n = (size_t)h->A[l]->M * K;
    if (l == h->nlevels - 1) {
        CHK(coarse_solve_block(h, B, u, rhs, u_zero));
        *out = u;
        return SGPU_OK;
    }
    double *cur = u, *oth = alt, *t = nullptr;
    if (u_zero) CHK(sgpu_vec_fill(cur, 0.0, n));
    if (h->prm.preSmooth) {
        CHK(smooth_block_pp(h, l, h->prm.preSmooth, cur, oth, rhs, &t, K));
        if (t != cur) std::swap(cur, oth);
    }
    { EpiArgs e; e.rhs = rhs; CHK(apply_block(h->A[l], sk::EPI_RESIDUAL, cur, B.res[l], e, K)); }
    CHK(apply_block(h->R[l], sk::EPI_SPMV, B.res[l], B.rhs[l + 1], EpiArgs(), K));
    double *uc = nullptr;
    CHK(vcycle_block_level(h, B, l + 1, B.u[l + 1], B.alt[l + 1], B.rhs[l + 1], &uc, true));
    CHK(apply_block(h->P[l], sk::EPI_SUB, uc, cur, EpiArgs(), K));
    if (h->prm.postSmooth) {
        CHK(smooth_block_pp(h, l, h->prm.postSmooth, cur, oth, rhs, &t, K));
        if (t != cur) std::swap(cur, oth);
    }
    *out = cur;
    return SGPU_OK;
}

int vcycle_block_eager(sgpu_amg *h, AmgBlock &B, double *u, const double *rhs, bool u_zero) {
    double *out = nullptr;
    CHK(vcycle_block_level(h, B, 0, u, B.alt0, rhs, &out, u_zero));
    if (out != u) HIPCHK(hipMemcpyAsync(u, out, (size_t)h->A[0]->M * B.K * sizeof(double), hipMemcpyDeviceToDevice, g.cs));
    return SGPU_OK;
}

// vcycle0 for blocks: captured once per (u, rhs, K) and replayed
int vcycle_block0(sgpu_amg *h, AmgBlock &B, double *u, const double *rhs, bool u_zero = false) {
    if (!h->prm.use_graph || g.multi()) return vcycle_block_eager(h, B, u, rhs, u_zero);
    if (!B.graphs.empty() && (B.graph_gen != g_plan_generation || B.block_gen != g_block_generation)) {
        HIPCHK(hipStreamSynchronize(g.cs));
        B.drop_graphs();
    }
    B.graph_gen = g_plan_generation; B.block_gen = g_block_generation;
    for (auto &c : B.graphs)
        if (c.u == u && c.rhs == rhs && c.u_zero == u_zero) { ++g_launches; HIPCHK(hipGraphLaunch(c.exec, g.cs)); return SGPU_OK; }
    CapturedCycle c;
    c.u = u; c.rhs = rhs; c.u_zero = u_zero;
    HIPCHK(hipStreamBeginCapture(g.cs, hipStreamCaptureModeThreadLocal));
    const int st = vcycle_block_eager(h, B, u, rhs, u_zero);
    const hipError_t e = hipStreamEndCapture(g.cs, &c.graph);
    if (st != SGPU_OK) return st;
    if (e != hipSuccess) return fail(SGPU_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    HIPCHK(hipGraphInstantiate(&c.exec, c.graph, nullptr, nullptr, 0));
    if (B.graphs.size() >= 8) B.graphs.erase(B.graphs.begin());
    B.graphs.push_back(std::move(c));
    ++g_launches; HIPCHK(hipGraphLaunch(B.graphs.back().exec, g.cs));
    return SGPU_OK;
}

// out[j] (K device scalars, this rank's share) summed over the ranks on the columns of `active`; the others keep their bits.  Summed
// into scratch (rows 0 and 1 of S) and copied under the mask: in place, a frozen column's stale slot would be multiplied by the
// rank count.  Every rank reads the same reduced bits, so the masks, iteration counts and histories agree on all of them.
int rank_sum_block(AmgBlock &B, double *out, unsigned active) {
    if (!g.multi()) return SGPU_OK;
    const int K = B.K;
    double *sum = B.S + K;
    if (g.comm) {
        NCCLCHK(ncclAllReduce(out, sum, (size_t)K, ncclDouble, ncclSum, g.comm, g.cs));
        ++g_launches;
    } else {
        HIPCHK(hipMemcpyAsync(B.hS, out, K * sizeof(double), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        CHK(host_allreduce(B.hS, K));
        HIPCHK(hipMemcpyAsync(sum, B.hS, K * sizeof(double), hipMemcpyHostToDevice, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));               // (hS is the mirror the caller fetches into next)
    }
    SGPU_LAUNCH(sk::k_copy_masked, dim3(1), dim3(64), 0, g.cs, (const double *)sum, out, K, active);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// out[j] = x_j . y_j on the columns of `active` (the others keep what they hold); this rank's rows
int dot_block(AmgBlock &B, const double *x, const double *y, size_t n, double *out, unsigned active) {
    const int nb = dot_nblocks(n), K = B.K;
    SGPU_LAUNCH_COLS("k_dot_block_partial", K, per_K(K, [](auto k) { return sk::k_dot_block_partial<k()>; }), dim3(nb), dim3(sk::BLOCK), 0, g.cs, x, y, n, B.partials);
    SGPU_LAUNCH(sk::k_reduce_partials_block, dim3(K), dim3(sk::BLOCK), 0, g.cs, (const double *)B.partials, nb, K, out, active);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// alpha_j = num[j] / den[j]; u -= alpha p, r -= alpha h and out[j] = r_j . r_j on the columns of `active`: the fused update on
// the dot's grid, then the dot's second kernel
int pcg_update_block(AmgBlock &B, const double *num, const double *den, const double *p, const double *hh, double *u, double *r, size_t n,
                     unsigned active, double *out) {
    const int nb = dot_nblocks(n), K = B.K;
    SGPU_LAUNCH_COLS("k_pcg_update_block", K, per_K(K, [](auto k) { return sk::k_pcg_update_block<k()>; }), dim3(nb), dim3(sk::BLOCK), 0, g.cs, num, den, p, hh, u, r, n, active, B.partials);
    SGPU_LAUNCH(sk::k_reduce_partials_block, dim3(K), dim3(sk::BLOCK), 0, g.cs, (const double *)B.partials, nb, K, out, active);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// beta_j = num[j] / den[j]; p = z + beta p on the columns of `active`
int pcg_direction_block(AmgBlock &B, const double *num, const double *den, const double *z, double *p, size_t n, unsigned active) {
    const int gd = grid_for(2 * n), K = B.K;
    SGPU_LAUNCH_COLS("k_pcg_direction_block", K, per_K(K, [](auto k) { return sk::k_pcg_direction_block<k()>; }), dim3(gd), dim3(sk::BLOCK), 0, g.cs, num, den, z, p, n, active);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// what the three sgpu_debug_block_* wrappers check: the hierarchy (for its AmgBlock), K and the column mask
int debug_block_args(sgpu_amg *h, int K, unsigned active, const char *what, AmgBlock **B) {
    CHK(need_ctx());
    if (!h) return fail(SGPU_ERR_ARG, "%s: null hierarchy", what);
    CHK(amg_block_check(h, K, what));
    if (active >> K) return fail(SGPU_ERR_ARG, "%s: the column mask 0x%x names columns past K = %d", what, active, K);
    return amg_block(h, K, B);
}

} // namespace

extern "C" {

// ---- measurement (tests/perf_block.py): sgpu_time_kernel's loop for the block kernel and for whole V-cycles, scalar or block:
// `reps` back-to-back enqueues inside the library between the context's two events (time_reps) ----
int sgpu_debug_time_block(sgpu_op *op, int kind, const value_t *X, const value_t *RHS, value_t *Y, int K, int reps, float *ms) {
    CHK(need_ctx());
    if (!op || !X || !Y || !ms || reps < 1 || (kind != 0 && kind != 1)) return fail(SGPU_ERR_ARG, "bad argument");
    if (kind == 1 && (!RHS || !op->inv_diag)) return fail(SGPU_ERR_ARG, "a Jacobi sweep needs rhs and inv_diag");
    CHK(block_check(op, K, "time_block"));
    return time_reps(reps, ms, [&]() -> int {
        EpiArgs e;
        if (kind == 1) { e.rhs = RHS; e.inv_diag = op->inv_diag; e.u = X; e.c0 = JACOBI_OMEGA_REF; }
        return apply_block(op, kind == 1 ? sk::EPI_JACOBI : sk::EPI_SPMV, X, Y, e, K);
    });
}
int sgpu_debug_time_vcycle(sgpu_amg *h, value_t *U, const value_t *RHS, int K, int reps, float *ms) {
    CHK(need_ctx());
    if (!h || !U || !RHS || !ms || reps < 1) return fail(SGPU_ERR_ARG, "bad argument");
    AmgBlock *B = nullptr;
    if (K != 0) { CHK(amg_block_check(h, K, "time_vcycle")); CHK(amg_block(h, K, &B)); }
    auto once = [&]() -> int { return K ? vcycle_block0(h, *B, U, RHS) : vcycle0(h, U, RHS); };
    CHK(once());                                                        // (captures the graph outside the interval)
    return time_reps(reps, ms, once);
}

// ---- tests (include/saena_gpu_debug.h): the launch code of the block dot and of the two pCG updates on the caller's vectors ----
int sgpu_debug_block_dot(sgpu_amg *h, const value_t *X, const value_t *Y, size_t n, int K, unsigned active, value_t *out_dev) {
    AmgBlock *B = nullptr;
    CHK(debug_block_args(h, K, active, "debug_block_dot", &B));
    if (!X || !Y || !out_dev) return fail(SGPU_ERR_ARG, "null argument");
    return dot_block(*B, X, Y, n, out_dev, active);
}

int sgpu_debug_block_pcg_update(sgpu_amg *h, const value_t *num, const value_t *den, const value_t *P, const value_t *H,
                                value_t *U, value_t *R, size_t n, int K, unsigned active, value_t *rr_dev) {
    AmgBlock *B = nullptr;
    CHK(debug_block_args(h, K, active, "debug_block_pcg_update", &B));
    if (!num || !den || !P || !H || !U || !R || !rr_dev) return fail(SGPU_ERR_ARG, "null argument");
    return pcg_update_block(*B, num, den, P, H, U, R, n, active, rr_dev);
}

int sgpu_debug_block_pcg_direction(sgpu_amg *h, const value_t *num, const value_t *den, const value_t *Z, value_t *P,
                                   size_t n, int K, unsigned active) {
    AmgBlock *B = nullptr;
    CHK(debug_block_args(h, K, active, "debug_block_pcg_direction", &B));
    if (!num || !den || !Z || !P) return fail(SGPU_ERR_ARG, "null argument");
    return pcg_direction_block(*B, num, den, Z, P, n, active);
}

// ---- tests: the block twins of sgpu_debug_pack / sgpu_debug_inject_halo ----
int sgpu_debug_pack_block(sgpu_op *op, const value_t *X, int K, value_t *send_host) {
    CHK(need_ctx());
    if (!op || !X) return fail(SGPU_ERR_ARG, "null argument");
    CHK(block_check(nullptr, K, "debug_pack_block"));
    if (op->vIndexSize == 0) return SGPU_OK;
    if (!send_host) return fail(SGPU_ERR_ARG, "null argument");
    CHK(ensure_blk_halo(op, K));
    CHK(pack_block(op, X, K, false, op->halo_fp32, g.cs));
    return sgpu_vec_download(send_host, op->send_blk[block_slot(K)], (size_t)op->vIndexSize * K);
}

int sgpu_debug_inject_halo_block(sgpu_op *op, int K, const value_t *recv_host) {
    CHK(need_ctx());
    if (!op) return fail(SGPU_ERR_ARG, "null argument");
    CHK(block_check(nullptr, K, "debug_inject_halo_block"));
    if (op->recvSize && !recv_host) return fail(SGPU_ERR_ARG, "null argument");
    CHK(ensure_blk_halo(op, K));
    if (op->recvSize) CHK(sgpu_vec_upload(op->recv_blk[block_slot(K)], recv_host, (size_t)op->recvSize * K));
    op->injected_blk[block_slot(K)] = true;
    return SGPU_OK;
}

int sgpu_block_pack(const value_t *cols_colmajor, value_t *blk, size_t n, int K) {
    CHK(need_ctx());
    if (!cols_colmajor || !blk) return fail(SGPU_ERR_ARG, "null argument");
    CHK(block_check(nullptr, K, "block_pack"));
    return block_pack(cols_colmajor, blk, n, K);
}

int sgpu_block_unpack(const value_t *blk, value_t *cols_colmajor, size_t n, int K) {
    CHK(need_ctx());
    if (!cols_colmajor || !blk) return fail(SGPU_ERR_ARG, "null argument");
    CHK(block_check(nullptr, K, "block_unpack"));
    return block_unpack(blk, cols_colmajor, n, K);
}

int sgpu_block_center(const value_t *X, value_t *Y, size_t n, int K) {
    CHK(need_ctx());
    if (!X || !Y) return fail(SGPU_ERR_ARG, "sgpu_block_center: null argument");
    CHK(block_check(nullptr, K, "block_center"));
    if (((uintptr_t)X | (uintptr_t)Y) & 15u) return fail(SGPU_ERR_ARG, "sgpu_block_center: X and Y must be 16-byte aligned (the kernels move pairs of columns)");
    if (g.nranks > 1) return fail(SGPU_ERR_ARG, "sgpu_block_center: the means are taken over this rank's rows; one rank only (this context has %d)", g.nranks);
    return center_block_async(X, Y, n, K);
}

int sgpu_op_set_block_lanes(sgpu_op *op, int lanes) {
    if (!op) return fail(SGPU_ERR_ARG, "null op");
    if (lanes != 0 && lanes != 1 && lanes != 4 && lanes != 16 && lanes != 64) return fail(SGPU_ERR_ARG, "block lanes per row must be 0 (auto), 1, 4, 16 or 64 (got %d)", lanes);
    op->block_lanes = lanes;
    ++g_block_generation;
    return SGPU_OK;
}

int sgpu_op_get_block_lanes(const sgpu_op *op, int *lanes) {
    if (!op || !lanes) return fail(SGPU_ERR_ARG, "null argument");
    *lanes = op->block_lanes ? op->block_lanes : (op->block_lanes_auto ? op->block_lanes_auto : block_auto_lanes(op));
    return SGPU_OK;
}

int sgpu_spmv_block(sgpu_op *op, const value_t *X, value_t *Y, int K) {
    CHK(need_ctx());
    if (!op || !X || !Y) return fail(SGPU_ERR_ARG, "null argument");
    CHK(block_check(op, K, "spmv_block"));
    return apply_block(op, sk::EPI_SPMV, X, Y, EpiArgs(), K);
}

int sgpu_residual_block(sgpu_op *op, const value_t *U, const value_t *RHS, value_t *RES, int K) {
    CHK(need_ctx());
    if (!op || !U || !RHS || !RES) return fail(SGPU_ERR_ARG, "null argument");
    CHK(block_check(op, K, "residual_block"));
    EpiArgs e; e.rhs = RHS;
    return apply_block(op, sk::EPI_RESIDUAL, U, RES, e, K);
}

int sgpu_jacobi_block(sgpu_op *op, int iter, value_t omega, value_t *U, const value_t *RHS, int K) {
    CHK(need_ctx());
    if (!op || !U || !RHS || iter < 0) return fail(SGPU_ERR_ARG, "bad argument");
    CHK(block_check(op, K, "jacobi_block"));
    if (omega == 0.0) omega = JACOBI_OMEGA_REF;
    CHK(ensure_blk_tmp(op, K));
    double *res = nullptr;
    CHK(jacobi_block_pp(op, iter, omega, U, op->tmp_blk[block_slot(K)], RHS, &res, K));
    if (res != U) HIPCHK(hipMemcpyAsync(U, res, (size_t)op->M * K * sizeof(double), hipMemcpyDeviceToDevice, g.cs));
    return SGPU_OK;
}

int sgpu_chebyshev_block(sgpu_op *op, int iter, value_t eig_max, value_t *U, const value_t *RHS, int K) {
    CHK(need_ctx());
    if (!op || !U || !RHS || iter < 0) return fail(SGPU_ERR_ARG, "bad argument");
    CHK(block_check(op, K, "chebyshev_block"));
    if (!(eig_max > 0.0)) return fail(SGPU_ERR_ARG, "chebyshev needs eig_max > 0");
    CHK(ensure_blk_tmp(op, K)); CHK(ensure_blk_d(op, K));
    double *res = nullptr;
    CHK(cheby_block_pp(op, iter, eig_max, U, op->tmp_blk[block_slot(K)], RHS, &res, K));
    if (res != U) HIPCHK(hipMemcpyAsync(U, res, (size_t)op->M * K * sizeof(double), hipMemcpyDeviceToDevice, g.cs));
    return SGPU_OK;
}

int sgpu_prolong_correct_block(sgpu_op *P, const value_t *E_coarse, value_t *U, int K) {
    CHK(need_ctx());
    if (!P || !E_coarse || !U) return fail(SGPU_ERR_ARG, "null argument");
    CHK(block_check(P, K, "prolong_correct_block"));
    return apply_block(P, sk::EPI_SUB, E_coarse, U, EpiArgs(), K);
}

int sgpu_vcycle_block(sgpu_amg *h, value_t *U, const value_t *RHS, int K) {
    CHK(need_ctx());
    if (!h || !U || !RHS) return fail(SGPU_ERR_ARG, "null argument");
    CHK(amg_block_check(h, K, "vcycle_block"));
    AmgBlock *B = nullptr;
    CHK(amg_block(h, K, &B));
    return vcycle_block0(h, *B, U, RHS);
}

// sgpu_solve_pCG's recurrence for K columns in lockstep.  Per column: its own rho, alpha, beta (device scalars, rows of S) and
// threshold (with a communicator or a host transport the dots are summed over the ranks, rank_sum_block); a column is frozen from the iteration at which its ||r||^2 drops below its threshold -- bit j of `active` leaves
// the mask every update kernel takes, and the column's u, r, p and scalars are not written again.  One host synchronisation
// per iteration: the K current dots (two more per dot under the host transport).
int sgpu_solve_pCG_block(sgpu_amg *h, value_t *U, const value_t *RHS, int K, int *iters, value_t *hist, int cap) {
    CHK(need_ctx());
    if (!h || !U || !RHS) return fail(SGPU_ERR_ARG, "null argument");
    CHK(amg_block_check(h, K, "solve_pCG_block"));
    AmgBlock *Bp = nullptr;
    CHK(amg_block(h, K, &Bp));
    AmgBlock &B = *Bp;
    sgpu_op *A = h->A[0];
    const size_t sz = (size_t)A->M, szK = sz * K;
    double *r = B.r, *rho = B.rho, *hh = B.hh, *p = B.p;
    double *Sa = B.S + 4 * K, *Sb = B.S + 7 * K, *Sph = B.S + 5 * K, *Srr = B.S + 6 * K;    // the slots of sgpu_solve_pCG, a row of K each
    const unsigned all = (1u << K) - 1u;
    auto fetch = [&](const double *row) -> int {
        HIPCHK(hipMemcpyAsync(B.hS, row, K * sizeof(double), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        return SGPU_OK;
    };
    CHK(sgpu_vec_fill(U, 0.0, szK));
    { EpiArgs e; e.rhs = RHS; CHK(apply_block(A, sk::EPI_RESIDUAL, U, r, e, K)); }
    if (h->null_space == 1) CHK(center_block_async(r, r, sz, K));        // r_0 = RHS - its column means; nothing is centred per iteration
    CHK(dot_block(B, r, r, sz, Srr, all));
    CHK(rank_sum_block(B, Srr, all));
    // under null_space 1 the K sums the centring left come down in front of the same synchronisation (one rank: slots 8.. are free)
    if (h->null_space == 1) HIPCHK(hipMemcpyAsync(g.hscalar + 8, g.cblk + (size_t)g.n_partials * 8, K * sizeof(double), hipMemcpyDeviceToHost, g.cs));
    CHK(fetch(Srr));
    double thr[8], cur[8];
    int it[8];
    unsigned active = 0, failed = 0;
    int bad_col = -1, bad_it = 0;                  // the first column with a non-finite dot (rule 3), for the message
    for (int j = 0; j < K; ++j) {
        const double init = B.hS[j];
        if (hist && cap > 0) hist[(size_t)j * cap] = std::sqrt(init);
        thr[j] = init * h->prm.solver_tol * h->prm.solver_tol;
        cur[j] = init;
        it[j] = 0;
        // rules 1 to 3 of include/saena_gpu.h per column, as sgpu_solve_pCG takes them: a zero right-hand side, or one that is zero
        // after centring up to the rounding of its mean, has u = 0 as its solution; a non-finite one fails.  All are frozen at iteration 0
        if (!std::isfinite(init)) { failed |= 1u << j; if (bad_col < 0) bad_col = j; }
        else if (init == 0.0 || (h->null_space == 1 && centred_is_dust(init, g.hscalar[8 + j], sz))) { if (hist && cap > 0) hist[(size_t)j * cap] = 0.0; }
        else active |= 1u << j;
    }
    if (active && h->prm.solver_max_iter > 0) {
        CHK(vcycle_block0(h, B, rho, r, true));
        CHK(sgpu_vec_copy(p, rho, szK));
        CHK(dot_block(B, r, rho, sz, Sa, active));
        CHK(rank_sum_block(B, Sa, active));
        for (int i = 0; i < h->prm.solver_max_iter && active; ++i) {
            CHK(apply_block(A, sk::EPI_SPMV, p, hh, EpiArgs(), K));
            CHK(dot_block(B, p, hh, sz, Sph, active));
            CHK(rank_sum_block(B, Sph, active));
            CHK(pcg_update_block(B, Sa, Sph, p, hh, U, r, sz, active, Srr));
            CHK(rank_sum_block(B, Srr, active));
            CHK(fetch(Srr));
            for (int j = 0; j < K; ++j) {
                if (!((active >> j) & 1u)) continue;
                cur[j] = B.hS[j];
                it[j] = i + 1;
                if (hist && i + 1 < cap) hist[(size_t)j * cap + i + 1] = std::sqrt(cur[j]);
                if (cur[j] < thr[j]) active &= ~(1u << j);
                else if (!std::isfinite(cur[j])) {                 // rule 3: frozen here and failed; the others go on
                    active &= ~(1u << j); failed |= 1u << j;
                    if (bad_col < 0) { bad_col = j; bad_it = i + 1; }
                }
            }
            if (!active || i + 1 == h->prm.solver_max_iter) break;
            CHK(vcycle_block0(h, B, rho, r, true));
            CHK(dot_block(B, r, rho, sz, Sb, active));
            CHK(rank_sum_block(B, Sb, active));
            CHK(pcg_direction_block(B, Sb, Sa, rho, p, sz, active));
            std::swap(Sa, Sb);
        }
    }
    if (h->null_space == 1) CHK(center_block_async(U, U, sz, K));    // every column: the solution of zero mean
    failed |= active;                              // still above their thresholds at solver_max_iter
    if (iters) for (int j = 0; j < K; ++j) iters[j] = it[j];
    if (bad_col >= 0) return fail(SGPU_ERR_NOCONV, "solve_pCG_block: non-finite residual at iteration %d (column %d)", bad_it, bad_col);
    return failed ? SGPU_ERR_NOCONV : SGPU_OK;
}

} // extern "C"
