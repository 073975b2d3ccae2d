"""Pins of tests/xwin_ref.py: the geometry the x-window mode of k_vidx has on each named operator of tests/test_gpu_x_windows.py --
row-loop turns, slice widths, windows, staging passes, LDS bytes, verdict.  Each operator exists to reach one path of k_vidxw or
build_xwin; if an edit moves it off that path, this file fails on a machine without a GPU."""
import numpy as np
import pytest

from tests import xwin_ref as X

LDS, WIN = X.LDS_CAP, X.TOO_MANY_WINDOWS
# name -> (slice widths, uniform, per R in (256, 512, 1024): (windows, S, staging passes) or the reason of the refusal)
TABLE = {
    "wide19": ({24}, True, [(1, 274, 1), (1, 530, 1), (1, 1042, 1)]),
    "steps": ({8, 16}, False, [(1, 268, 1), (1, 524, 1), (1, 1036, 1)]),
    "four": ({8}, True, [(4, 1024, 1), (4, 2048, 1), (4, 4096, 1)]),
    "five": ({8}, True, [(5, 1280, 2), (5, 2560, 2), (5, 5120, 2)]),
    "seven": ({8}, True, [(7, 1792, 2), (7, 3584, 2), LDS]),
    "sixteen": ({8, 16}, False, [(16, 4096, 4), LDS, LDS]),
    "seventeen": ({16, 24}, False, [WIN, WIN, WIN]),
    "comb": ({8, 16}, False, [(1, 2256, 3), (1, 2512, 2), (1, 3024, 1)]),
    "gaps": ({8}, True, [(4, 1792, 2), (1, 2561, 2), (1, 3073, 1)]),
    "tall": ({8}, True, [(3, 768, 1), (1, 1212, 1), (1, 1724, 1)]),
    "flat": ({8}, True, [(3, 768, 1), (1, 1212, 1), (1, 1724, 1)]),
    "holes": ({8}, True, [(1, 258, 1), (1, 514, 1), (1, 1026, 1)]),
    "tiny": ({8}, True, [(1, 258, 1), (1, 514, 1), (1, 1026, 1)]),
}


def test_the_table_names_every_operator():
    assert set(TABLE) == set(X.OPERATORS)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_geometry_of_the_named_operators(name):
    w8, uniform, per_r = TABLE[name]
    st = X.named_structure(name)
    assert set(st["w8"]) == w8 and st["uniform"] == uniform
    assert st["one_table"] and st["padding"] <= X.SELL_PAD              # the pattern forms take it
    for R, want in zip(X.ROWS, per_r):
        g = X.named_geometry(name, R)
        if isinstance(want, str):
            assert g["verdict"] == want, (name, R)
        else:
            assert g["verdict"] == X.OK and (g["nwin"], g["S"], g["passes"]) == want, (name, R)


def test_the_paths_the_operators_were_written_for():
    g = X.named_geometry
    assert max(X.named_structure("wide19")["w8"]) // 8 == 3                       # the row loop turns three times: two code hand-overs
    assert X.named_structure("steps")["npat"] * 14 <= X.SP_MAX_TABLE and not X.named_structure("steps")["uniform"]     # a.vcptr, not a.uw
    assert g("four", 256)["nwin"] == 4 and g("five", 256)["nwin"] == 5            # the register slots end at four windows
    assert g("sixteen", 256)["nwin"] == X.SPX_MAXWIN and g("seventeen", 1024)["nwin"] == X.SPX_MAXWIN + 1
    assert g("seven", 1024)["lds"] == 65680 and g("sixteen", 512)["lds"] == 70192 and X.VW_MAX_LDS == 65536
    assert g("sixteen", 256)["passes"] == 4 and g("comb", 256)["passes"] == 3
    # the gap rule at its edge: at 256 rows the gaps of 256 merge and those of 257 and 512 split; at 512 rows every gap merges
    assert g("gaps", 256)["windows"] == [(-1025, -1025), (-513, -257), (0, 512), (1024, 1024)]
    assert g("gaps", 512)["windows"] == [(-1025, 1024)]
    assert all(g(n, R)["clamped"] for n in ("tall", "flat") for R in X.ROWS)      # windows that leave [0, ncols), ncols != nrows
    assert abs(X.named_structure("holes")["padding"] - 1.061) < 5e-4 and (X.named_structure("holes")["lens"] == 0).sum() == 200
    tiny = X.named_structure("tiny")
    assert len(tiny["w8"]) == 1 and len(tiny["lens"]) == 60                       # one partial slice; R / 64 - 1 waves without one


def test_windows_and_lds_formula_on_a_hand_case():
    """offsets -3, 0, 300 on 1000 rows at R = 256: the gap of 300 splits; S = (256 + 3) + 256; three patterns of at most three entries"""
    r = np.arange(1000)
    rows = np.concatenate([r[r >= 3], r, r[r + 300 < 1000]])
    cols = np.concatenate([r[r >= 3] - 3, r, r[r + 300 < 1000] + 300])
    g = X.geometry(rows, cols, 1000, 1000, 256)
    assert g["patterns"] == [(0, 300), (-3, 0, 300), (-3, 0)] and g["W"] == 3
    assert g["windows"] == [(-3, 0), (300, 300)] and g["S"] == 515 and g["passes"] == 1
    assert g["lds"] == 516 * 8 + 2048 + 2 * (8 + 3 * 8) and g["verdict"] == X.OK
    assert X.setup_line(g) == (256, 2, 515, "6.1")
    assert X.geometry(rows, cols, 1000, 1000, 512)["windows"] == [(-3, 300)]
