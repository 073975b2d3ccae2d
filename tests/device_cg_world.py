"""The three-rank worlds of tests/test_gpu_device_cg_multirank.py as data (test infrastructure: no GPU, no library call).

Poisson 32^3 under options001 with the coarsening cut after two steps: three levels, the coarsest of 1 420 rows -- past the 1 024
the LDS-resident coarsest solvers hold, so the rank that owns it takes the large-coarsest-level path (the host-driven CG under
coarse_solver 0 / 1, the device-resident CG under 2).  Three agglomeration policies (host/amg_setup.h, read from the environment)
give the three ownerships that path has across ranks; tests/test_device_cg_multirank_cases.py asserts rows and owners on the CPU
by running the host setup, so that a change of the shrink policy fails there and not as a GPU failure that is hard to read."""

WORLD = 3
M = 32                                                   # laplacian3D(32): 30^3 rows
OPTIONS = dict(dynamic_levels=0, max_level=2)            # over host.OPTIONS001
ROWS = [27000, 13500, 1420]
ALL = [0, 1, 2]

CONFIGS = {
    # the default cost model: both coarse levels on rank 0 -- the tail graph holds level 1 and the coarsest solve
    "model": dict(env={}, owners=[ALL, [0], [0]]),
    # levels of <= 4096 rows on rank 0: level 1 exchanges halos around a tail that is the coarsest solve alone
    "rows4096": dict(env={"SAENA_SHRINK_CHAIN_US": "0", "SAENA_SHRINK_ROWS": "4096"}, owners=[ALL, ALL, [0]]),
    # the coarsest level stays row-partitioned: the distributed CG, whatever coarse_solver says
    "rows300": dict(env={"SAENA_SHRINK_CHAIN_US": "0", "SAENA_SHRINK_ROWS": "300"}, owners=[ALL, ALL, ALL]),
}


def options(host_module, L, **more):
    """the OptionsC of every hierarchy of these worlds"""
    return host_module.options(L, **dict(host_module.OPTIONS001, **OPTIONS, **more))


def owners_of(S, world=WORLD):
    """per level, the ranks that own rows of it"""
    out = []
    for l in range(S.num_levels):
        s = S.level_split(l)
        out.append([r for r in range(world) if s[r + 1] > s[r]])
    return out
