"""Bitwise-distinct values per workgroup of rows of every operator of a Poisson hierarchy (host library only; the host setup
with SAENA_HOST_SPGEMM=1).  Decides which operators the value-indexed form (k_vidx: 8-bit codes into a dictionary of at most
256 values per workgroup) is offered to:
    SAENA_HOST_SPGEMM=1 python tools/value_dict_count.py 64 128 > profiles/r05_value_dict_count.log"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("SAENA_HOST_SPGEMM", "1")
from saena_amd import host  # noqa: E402


def distinct_per_group(npr, val, rows_per_group):
    """-> number of bitwise-distinct values in each group of `rows_per_group` consecutive rows"""
    M = len(npr)
    ng = (M + rows_per_group - 1) // rows_per_group
    if len(val) == 0:
        return np.zeros(ng, np.int64)
    grp = np.repeat(np.arange(M, dtype=np.int64) // rows_per_group, npr)
    bits = np.ascontiguousarray(val, np.float64).view(np.uint64)
    order = np.lexsort((bits, grp))
    g, b = grp[order], bits[order]
    new = np.ones(len(b), bool)
    new[1:] = (g[1:] != g[:-1]) | (b[1:] != b[:-1])
    return np.bincount(g[new], minlength=ng)


def report(m):
    L = host.load("host")
    A = host.Matrix(host.Comm("host", "self")).laplacian3D(m).assemble()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001))
    print(f"# Poisson {m}^3: {S.num_levels} levels; distinct fp64 bit patterns per workgroup of 256 / 1024 rows")
    print(f"{'op':<6}{'rows':>10}{'nnz':>12}{'per row':>9}{'op total':>10}"
          f"{'max/256':>9}{'mean/256':>10}{'>256 @256':>11}{'max/1024':>10}{'>256 @1024':>12}  distribution @256 (<=2, <=16, <=64, <=256, >256)")
    for l in range(S.num_levels):
        for which, name in ((0, "A"), (2, "R"), (1, "P")):
            if which and l == S.num_levels - 1:
                continue
            d = S.level_layout(l, which)
            npr, val = d["nnzPerRow_local"], d["val_local"]
            M, nnz = len(npr), len(val)
            c256, c1024 = distinct_per_group(npr, val, 256), distinct_per_group(npr, val, 1024)
            tot = len(np.unique(np.ascontiguousarray(val).view(np.uint64)))
            hist = [int(np.sum(c256 <= 2)), int(np.sum((c256 > 2) & (c256 <= 16))), int(np.sum((c256 > 16) & (c256 <= 64))),
                    int(np.sum((c256 > 64) & (c256 <= 256))), int(np.sum(c256 > 256))]
            print(f"{name}{l:<5}{M:>10}{nnz:>12}{nnz / max(1, M):>9.1f}{tot:>10}{int(c256.max()):>9}{c256.mean():>10.1f}"
                  f"{int(np.sum(c256 > 256)):>11}{int(c1024.max()):>10}{int(np.sum(c1024 > 256)):>12}  {hist}")
    S.free()
    A.free()


if __name__ == "__main__":
    for arg in sys.argv[1:] or ["64"]:
        report(int(arg))
        sys.stdout.flush()
