"""The block halo exchange over RCCL on ONE GPU (run as a subprocess by tests/test_gpu_block_rccl.py).

tests/rccl_loopback.py's operator -- rank 0's share of a 2-rank Poisson 14^3 operator, its neighbour rewired to the rank itself
over a 1-rank communicator -- under sgpu_spmv_block, one Jacobi sweep and a 3-step Chebyshev smoother for K = 2 and 8 columns, on
the fp64 and the fp32 wire: pack_block -> ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd of K times the scalar counts ->
k_csr_block with the boundary mask -> k_csr_boundary_block.  The reference is the host formula A_loop v = local v + remote v[vIndex]
applied per column.  SAENA_SINGLE_STREAM_NNZ in the environment picks the ordering: unset, one stream; 0, two streams and events."""
import os
import sys

if "--torch" in sys.argv:
    import torch  # noqa: F401

import numpy as np

from oracle import oracle as orc
from saena_amd import capi
from tests import inputs


def main():
    capi.init(0, 0, 1, capi.get_unique_id())
    capi.check(capi.lib().sgpu_barrier())
    entries, M = orc.laplacian3d(14)
    O = orc.OracleOp(entries, M, M, orc.split_even(M, 2))
    R = O.rank(0)
    arr = lambda name, cnt, dt: O.rank_array(0, name, cnt, dt)     # noqa: E731
    assert R.numSendProc == 1 and R.numRecvProc == 1 and R.vIndexSize == R.recvSize
    n = int(R.M)
    npr = arr("nnzPerRow_local", n, np.int32)
    rows = np.repeat(np.arange(n), npr)
    cols = np.repeat(np.arange(R.col_remote_size), arr("nnzPerCol_remote", R.col_remote_size, np.int32))
    vi, invd = arr("vIndex", R.vIndexSize, np.int32), arr("inv_diag", n, np.float64)
    lc, lv = arr("col_local", R.nnz_l_local, np.int32), arr("val_local", R.nnz_l_local, np.float64)
    rr, rv = arr("row_remote", R.nnz_l_remote, np.int32), arr("val_remote", R.nnz_l_remote, np.float64)
    omega = float(np.float32(2.0 / 3))
    for fp32 in (False, True):
        op = capi.Operator(
            M=n, N_local=n, col_offset=0, nnzPerRow_local=npr, col_local=lc, val_local=lv,
            nnzPerCol_remote=arr("nnzPerCol_remote", R.col_remote_size, np.int32), row_remote=rr, val_remote=rv,
            recvProcRank=[0], recvProcCount=arr("recvProcCount", 1, np.int32),
            sendProcRank=[0], sendProcCount=arr("sendProcCount", 1, np.int32),
            vIndex=vi, inv_diag=invd, halo_fp32=fp32)

        def A_loop(v):
            out = np.zeros(n)
            np.add.at(out, rows, lv * v[lc])
            h = v[vi].astype(np.float32).astype(np.float64) if fp32 else v[vi]
            np.add.at(out, rr, rv * h[cols])
            return out

        def cheby3(x, rhs, eig):
            alpha, beta = 0.13 * eig, eig
            delta, theta = (beta - alpha) / 2, (beta + alpha) / 2
            s1 = theta / delta
            rhok = 1 / s1
            u = x.copy()
            d = (1 / theta) * invd * (rhs - A_loop(u))
            u = u + d
            for _ in range(2):
                rhokp1 = 1 / (2 * s1 - rhok)
                d = rhokp1 * rhok * d + (2 * rhokp1 / delta) * invd * (rhs - A_loop(u))
                u = u + d
                rhok = rhokp1
            return u

        for K in (2, 8):
            X = np.stack([inputs.v2(n, ofs=101 * j) * (1.0 + 0.25 * j) for j in range(K)], axis=1)
            B = np.stack([inputs.rhs2(n, ofs=17 * j) + 0.5 * j for j in range(K)], axis=1)
            want = np.stack([A_loop(X[:, j]) for j in range(K)], axis=1)
            dX, dY, dB = capi.BlockVector(n, K, X), capi.BlockVector(n, K), capi.BlockVector(n, K, B)
            for rep in range(3):                      # repeated exchanges reuse the block buffers and the operator's events
                op.spmv_block(dX, dY)
                got = dY.download()
                for j in range(K):
                    err = np.max(np.abs(got[:, j] - want[:, j]))
                    assert err <= 1e-12 * np.max(np.abs(want[:, j])), ("spmv_block", fp32, K, j, rep, err)
            dU = capi.BlockVector(n, K, X)
            op.jacobi_block(1, dU, dB)
            got = dU.download()
            for j in range(K):
                w = X[:, j] - (invd * omega) * (want[:, j] - B[:, j])
                assert np.max(np.abs(got[:, j] - w)) <= 1e-12 * np.max(np.abs(w)), ("jacobi_block", fp32, K, j)
            tol = 1e-6 if fp32 else 1e-12       # the fp32 wire rounds the halo of every step
            for rep in range(3):
                dU.upload(X)
                op.chebyshev_block(3, 2.0, dU, dB)
                got = dU.download()
                for j in range(K):
                    w = cheby3(X[:, j], B[:, j], 2.0)
                    err = np.max(np.abs(got[:, j] - w))
                    assert err <= tol * np.max(np.abs(w)), ("chebyshev_block", fp32, K, j, rep, err)
            print(f"block loopback halo ok (fp32={fp32}, K={K}, SAENA_SINGLE_STREAM_NNZ={os.environ.get('SAENA_SINGLE_STREAM_NNZ')}): "
                  f"{R.vIndexSize * K} values each way", flush=True)
    capi.finalize()
    print("RCCL_LOOPBACK_BLOCK_OK", flush=True)


if __name__ == "__main__":
    main()
