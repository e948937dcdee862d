"""The history-comparison problems of tests/test_gpu_bicgstabl_multi.py (BiCGStab(l) on a multi-device plan), shared with
tests/test_bicgstabl_multi_cases_cpu.py, which checks the input condition of every one of them.

A multi-device plan is a 3D grid cut into z slabs, so the problems of tests/bicgstabl_ref.py are mapped onto the grid sizes
through group_map: the grouped problem (331 groups, rho = 0.7) at l = 1, 2, 4 and the option problem (1025 groups, l = 2)."""
import numpy as np

import bicgstabl_ref as br

# (grid, ranks): one reduction block per rank (16^3 / 4 = 1024 entries), several blocks (32^3: 16 at P = 2, 4 at P = 8), unequal axes
GRIDS = [((16, 16, 16), 1), ((16, 16, 16), 2), ((16, 16, 16), 4), ((32, 32, 32), 2), ((32, 32, 32), 8), ((64, 16, 32), 4)]
OPTION_GRIDS = [((16, 16, 16), 4), ((32, 32, 32), 8)]
LS = [1, 2, 4]
OPTIONS = ["shadow", "x0", "x0-initially-zero", "cap"]
OPTION_GROUPS = 1025
CAP = 14


def size(grid):
    return int(np.prod(grid))


def grouped_label(N, l):
    return f"grouped-N{N}-l{l}"


def option_label(N, option):
    return f"{option}-N{N}"


def cases():
    """label -> (keyword arguments of bicgstabl_ref with per-group vectors and counts, the map entry -> group)"""
    out = {}
    lam, b = br.grouped_problem()
    for N in sorted({size(g) for g, _ in GRIDS}):
        gmap = br.group_map(N, br.GROUPS)
        for l in LS:
            out[grouped_label(N, l)] = (dict(b=b, pl=lam, l=l, max_mv_products=br.MAX_MV, counts=br.group_counts(gmap, br.GROUPS)), gmap)
    lam, b, x0, shadow = br.option_problem()
    for N in sorted({size(g) for g, _ in OPTION_GRIDS}):
        gmap = br.group_map(N, OPTION_GROUPS)
        base = dict(b=b, pl=lam, l=2, counts=br.group_counts(gmap, OPTION_GROUPS))
        out[option_label(N, "shadow")] = (dict(base, r_shadow=shadow), gmap)
        out[option_label(N, "x0")] = (dict(base, x0=x0), gmap)
        out[option_label(N, "x0-initially-zero")] = (dict(base, x0=x0, initially_zero=True), gmap)
        out[option_label(N, "cap")] = (dict(base, max_mv_products=CAP), gmap)
    return out
