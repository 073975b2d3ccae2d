"""What the library's table of SpMV forms (saena_amd/csrc/forms.h) says, restated by variant number.  No GPU here:
tests/test_forms_header.py holds the header to it on the host, tests/test_gpu_plan_storage.py holds the library to it on the device."""

XWIN = {256: "xwin256", 512: "xwin512", 1024: "xwin1024"}
# what the plan that settles on a variant keeps (csr: always; variant 17 also the x-window tables of the workgroup size in use)
KEEPS = {
    0: set(), 1: set(), 2: set(), 6: set(),
    3: {"cc0"}, 4: {"cc1"}, 5: {"dense"},
    7: {"cc0", "cm0"}, 8: {"cc1", "cm1"},
    9: {"sell_values", "sell_columns"},
    10: {"xlds_plan", "xlds_columns"}, 16: {"xlds_plan", "xlds_columns"},
    11: {"sell_values", "sellp"},
    12: {"xlds_plan", "sellx"},
    13: {"rowt"},
    14: {"sellp", "sellp2"},
    15: {"sell_values", "sellp", "sellpx"},
    17: {"sellp", "vidx"},
}


def kept(variant, xw=0):
    """the storage groups of a plan settled on `variant`, launched with x windows of `xw` rows per workgroup (0: none)"""
    return {"csr"} | KEEPS[variant] | ({XWIN[xw]} if variant == 17 and xw in XWIN else set())


def plan_line_valid(variant, lanes, xw):
    """a line of the plan cache: variant in range, 1..64 lanes, and x-window rows that variant 17 alone may carry"""
    return 0 <= variant <= 17 and 1 <= lanes <= 64 and (xw == 0 or (variant == 17 and xw in XWIN))
