"""Value-indexed row patterns (k_vidx, variant 17) against k_sellp (11) on the Poisson m^3 fine level (development aid):
    python -m tests.perf_value_index [m] [trials]
Per form: the bytes it stores (read: codes or values, pattern ids, x; written: y), its SpMV time, and the streaming ceiling of
THOSE bytes measured in the same run (capi.stream_ceiling) -- bench.py's roofline takes its byte count from a table that does not
know k_vidx, so its `frac` for this form is not the ratio to the form's own bytes."""
import os
import sys

import numpy as np

os.environ.setdefault("SAENA_KEEP_HOST_VALUES", "1")
from saena_amd import capi, host  # noqa: E402


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    trials = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    capi.init(0)
    print("device:", capi.device_info(), flush=True)
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(m).assemble()
    op = host.device_operator(A)
    info = op.info()
    M, nnz = info["M"], info["nnz_local"]
    x, y = capi.DeviceVector(M, np.sin(0.001 * np.arange(M))), capi.DeviceVector(M)
    slices = (M + 63) // 64
    # bytes read per launch: k_sellp 8 B per stored value position (7 per row here), k_vidx 1 B per code position (8 per row: groups
    # of 8), both a 16-bit pattern id per row and x; written: y
    forms = {11: ("k_sellp", 8 * 7 * 64 * slices + 2 * M + 8 * M), 17: ("k_vidx", 1 * 8 * 64 * slices + 2 * M + 8 * M)}
    ref = None
    for t in range(trials):
        for v, (name, rd) in forms.items():
            op.set_variant(v)
            op.spmv(x, y)
            got = y.download()
            if ref is None:
                ref = got
            assert np.array_equal(got, ref), f"{name} differs"
            ms = op.time_kernel(0, x, x, y, 400)
            us_c, mode, moved = capi.stream_ceiling(rd, 8 * M)
            print(f"trial {t} {name:8s} stored {rd / 1e6:7.1f} MB read + {8 * M / 1e6:5.1f} MB written ({(rd + 8 * M) / nnz:5.2f} B per entry): "
                  f"{ms * 1e3:6.2f} us, streaming ceiling of these bytes {us_c:6.2f} us ({mode}), frac {us_c / (ms * 1e3):.3f}", flush=True)


if __name__ == "__main__":
    main()
