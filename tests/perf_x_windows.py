"""The x-window launch mode of k_vidx (variant 17 + set_x_windows) against its direct gathers on the Poisson m^3 fine level
(development aid):
    python -m tests.perf_x_windows [m] [trials] [reps]
Per mode (direct, 256 / 512 / 1024 rows per workgroup), in alternating trials: the SpMV and the Jacobi-sweep time, next to the
streaming ceiling of the bytes the form stores, measured in the same run (capi.stream_ceiling).  Both modes store the same bytes
(codes, pattern ids, x read; y written), so one ceiling serves all of them.  The outputs of every mode are compared bit for bit."""
import os
import sys

import numpy as np

os.environ.setdefault("SAENA_KEEP_HOST_VALUES", "1")
from saena_amd import capi, host  # noqa: E402


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    trials = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 400
    capi.init(0)
    print("device:", capi.device_info(), flush=True)
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(m).assemble()
    op = host.device_operator(A)
    info = op.info()
    M, nnz = info["M"], info["nnz_local"]
    x, y = capi.DeviceVector(M, np.sin(0.001 * np.arange(M))), capi.DeviceVector(M)
    rhs = capi.DeviceVector(M, np.cos(0.002 * np.arange(M)))
    slices = (M + 63) // 64
    rd = 1 * 8 * 64 * slices + 2 * M + 8 * M          # a byte per code position (8 per row), a 16-bit pattern id per row, x
    us_c, mode_c, _ = capi.stream_ceiling(rd, 8 * M)
    us_cj, mode_cj, _ = capi.stream_ceiling(rd + 16 * M, 8 * M)       # a Jacobi sweep reads rhs and the inverse diagonal as well
    print(f"Poisson {m}^3: {M} rows, {nnz} entries; stored {rd / 1e6:.1f} MB read + {8 * M / 1e6:.1f} MB written; streaming ceiling "
          f"{us_c:.2f} us ({mode_c}), of a Jacobi sweep {us_cj:.2f} us ({mode_cj})", flush=True)
    op.set_variant(17)
    modes = [0]
    for rows in (256, 512, 1024):
        try:
            op.set_x_windows(rows)
            modes.append(rows)
        except capi.SgpuError as e:
            print(f"x windows at {rows} rows per workgroup refused: {e}", flush=True)
    ref = {}
    for t in range(trials):
        for rows in modes:
            op.set_x_windows(rows)
            assert op.x_windows() == rows and op.variant()[0] == 17
            op.spmv(x, y)
            u = capi.DeviceVector(M, np.sin(0.001 * np.arange(M)))
            op.jacobi(1, u, rhs)
            got = (y.download(), u.download())
            ref.setdefault("out", got)
            assert np.array_equal(got[0], ref["out"][0]) and np.array_equal(got[1], ref["out"][1]), f"mode {rows} differs"
            us = op.time_kernel(0, x, None, y, reps) * 1e3
            us_j = op.time_kernel(1, x, rhs, y, reps) * 1e3
            name = "direct gathers" if rows == 0 else f"x windows {rows:4d}"
            print(f"trial {t} {name:14s}: SpMV {us:7.2f} us (frac of ceiling {us_c / us:.3f}), Jacobi sweep {us_j:7.2f} us (frac {us_cj / us_j:.3f})", flush=True)


if __name__ == "__main__":
    main()
