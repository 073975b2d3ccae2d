"""The autotune's decision (choose_plan in saena_amd/csrc/forms.h), restated plainly in numpy.float32.  A table is a list of
(form, lanes, xwin_rows, ms); the order that breaks ties is ascending form, direct gathers before x windows, then lanes or rows."""
import numpy as np

F32 = np.float32
SEQUENTIAL = {9, 11, 13, 14, 15, 17}        # a lane per row: the reference's row sum
TILE_FORMS = {0, 1, 3, 4, 7, 8}             # ... and these at one lane per row
COLUMN_MAJOR = {7, 8}


def choose(table, fallback, direct_lanes):
    """-> (chosen (form, lanes, xwin), its ms, runner-up (form, lanes, xwin) or None, its ms, fastest ms of the family that competed)"""
    rows = sorted(((f, xw, l), F32(ms)) for f, l, xw, ms in table)
    big = F32(1e30)
    best = min([t for k, t in rows if k[0] not in COLUMN_MAJOR], default=big)
    best_cm = min([t for k, t in rows if k[0] in COLUMN_MAJOR], default=big)
    cm_wins = bool(best_cm < F32(0.95) * best)
    fastest = best_cm if cm_wins else best
    bar = F32(1.03) * fastest
    band = [(k, t) for k, t in rows if (k[0] in COLUMN_MAJOR) == cm_wins and not t > bar]
    seq = [(k, t) for k, t in band if k[0] in SEQUENTIAL or (k[2] == 1 and k[0] in TILE_FORMS)]
    if seq:
        pick = min(seq, key=lambda kt: kt[1])                  # the fastest; min() keeps the first of equals
    elif band:
        pick = band[0]
    else:
        pick = ((fallback[0], fallback[2], fallback[1]), F32(0))
    if pick[0][0] == 17 and pick[0][1]:                        # x windows: direct gathers inside the band come first
        direct = [(k, t) for k, t in band if k == (17, 0, direct_lanes)]
        pick = direct[0] if direct else pick
    others = [(k, t) for k, t in rows if k != pick[0]]
    ru = min(others, key=lambda kt: kt[1]) if others else None
    unkey = lambda k: (k[0], k[2], k[1])
    return unkey(pick[0]), pick[1], (unkey(ru[0]) if ru else None), (ru[1] if ru else F32(0)), fastest
