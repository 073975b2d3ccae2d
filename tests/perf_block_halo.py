"""K scalar applies against one block apply on an operator WITH a halo, exchange included, on ONE GPU: the RCCL loopback operator
of tests/rccl_loopback.py (rank 0's share of a 2-rank Poisson 14^3 operator, its neighbour rewired to the rank itself over a 1-rank
communicator).  The scalar side pays K exchange chains, the block side one; the wire is a device-local copy, so this isolates the
chain's launch and group overhead and says nothing about a link between two devices.

Both sides run as back-to-back launches inside the library between device events (sgpu_time_kernel / sgpu_debug_time_block),
alternated after a warm-up, `ROUNDS` times; printed: the best and the second-best time of each side (the run's own spread).  The
table is meant for profiles/block_halo_loopback.log.

python -m tests.perf_block_halo [--torch] [m]          (SAENA_SINGLE_STREAM_NNZ=0: the two-stream event ordering)
"""
import os
import sys

if "--torch" in sys.argv:
    import torch  # noqa: F401

import numpy as np

from oracle import oracle as orc
from saena_amd import capi
from tests import inputs

ROUNDS, REPS = 7, 200


def operator(m, fp32):
    entries, M = orc.laplacian3d(m)
    O = orc.OracleOp(entries, M, M, orc.split_even(M, 2))
    R = O.rank(0)
    arr = lambda name, cnt, dt: O.rank_array(0, name, cnt, dt)     # noqa: E731
    assert R.numSendProc == 1 and R.numRecvProc == 1
    op = capi.Operator(
        M=R.M, N_local=R.M, col_offset=0,
        nnzPerRow_local=arr("nnzPerRow_local", R.M, np.int32), col_local=arr("col_local", R.nnz_l_local, np.int32),
        val_local=arr("val_local", R.nnz_l_local, np.float64),
        nnzPerCol_remote=arr("nnzPerCol_remote", R.col_remote_size, np.int32),
        row_remote=arr("row_remote", R.nnz_l_remote, np.int32), val_remote=arr("val_remote", R.nnz_l_remote, np.float64),
        recvProcRank=[0], recvProcCount=arr("recvProcCount", 1, np.int32),
        sendProcRank=[0], sendProcCount=arr("sendProcCount", 1, np.int32),
        vIndex=arr("vIndex", R.vIndexSize, np.int32), inv_diag=arr("inv_diag", R.M, np.float64), halo_fp32=fp32)
    return op, int(R.M), int(R.vIndexSize)


def two_best(v):
    v = sorted(v)
    return v[0], v[1]


def main():
    m = next((int(a) for a in sys.argv[1:] if a.isdigit()), 14)
    capi.init(0, 0, 1, capi.get_unique_id())
    print(f"# block halo loopback, Poisson {m}^3 share of 2 ranks, SAENA_SINGLE_STREAM_NNZ={os.environ.get('SAENA_SINGLE_STREAM_NNZ')}; {capi.device_info()}")
    print("# wire  K  kind     K scalar applies us (best, 2nd)   one block apply us (best, 2nd)   ratio of the bests")
    for fp32 in (False, True):
        op, n, nhalo = operator(m, fp32)
        x, rhs, y = capi.DeviceVector(n, inputs.v2(n)), capi.DeviceVector(n, inputs.rhs2(n)), capi.DeviceVector(n)
        for K in (2, 4, 8):
            X = capi.BlockVector(n, K, np.stack([inputs.v2(n, ofs=j) for j in range(K)], axis=1))
            B = capi.BlockVector(n, K, np.stack([inputs.rhs2(n, ofs=j) for j in range(K)], axis=1))
            Y = capi.BlockVector(n, K)
            for kind, name in ((0, "spmv"), (1, "jacobi")):
                op.time_kernel(kind, x, rhs, y, 20)
                op.time_block(kind, X, B, Y, 20)
                ts, tb = [], []
                for _ in range(ROUNDS):                     # alternated: both sides see the same clocks
                    ts.append(K * op.time_kernel(kind, x, rhs, y, REPS) * 1e3)
                    tb.append(op.time_block(kind, X, B, Y, REPS) * 1e3)
                (s0, s1), (b0, b1) = two_best(ts), two_best(tb)
                print(f"  {'fp32' if fp32 else 'fp64'}  {K}  {name:7s}  {s0:9.2f} {s1:9.2f}                {b0:9.2f} {b1:9.2f}              {s0 / b0:5.2f}", flush=True)
        print(f"# {n} rows, halo {nhalo} values per column each way")
        op.destroy()
    capi.finalize()


if __name__ == "__main__":
    main()
