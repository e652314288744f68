"""The grids of the map tests, without a GPU.  The states are those of tests/profile_cases.py (its CASES, ZONES and
case_data); every case is binned under every grid below, truncated to the case's dimension.  tests/test_map_ref.py holds
every (case, grid) to `undecided == 0` on the CPU, which is what lets the GPU tests demand exact counts."""
import numpy as np

from profile_cases import CASES, IDS, ZONES, case_data  # noqa: F401 - the cases are the profile's

# name: (cells, lo, hi), per axis x, y, z
GRIDS = {
    "unit": ((7, 5, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "one": ((1, 1, 1), (-1.0, -1.0, -1.0), (2.0, 2.0, 2.0)),
    "fine": ((40, 24, 16), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "partial": ((6, 4, 5), (0.25, 0.1, 0.3), (0.8, 0.6, 1.5)),
    "slab": ((9, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
}


def grid(name, dim):
    """(name, cells, lo, hi) of a grid, truncated to the dimension"""
    cells, lo, hi = GRIDS[name]
    return (name, cells[:dim], lo[:dim], hi[:dim])


def slab_wide(dim):
    """`slab` with the one cell across y and z wide enough to hold every point: the grid under which a map IS the profile
    along x with 9 bins over [0, 1] (under `slab` itself the points that the curved boundary carries across y or z = 0, 1 are
    outside)"""
    return ("slab-wide", (9, 1, 1)[:dim], (0.0, -1.0, -1.0)[:dim], (1.0, 2.0, 2.0)[:dim])


# the columns a map row and a profile row along x have in common: n, vol, mass, ie, ke, mom_x <-> mom, pv, rho_min, rho_max
SLAB_COLS = [0, 1, 2, 3, 4, 5, 8, 9, 10]
PROFILE_COLS = [0, 1, 2, 3, 4, 5, 6, 8, 9]


def grids(dim):
    return [grid(name, dim) for name in GRIDS]


def points(d, S=None, m=None):
    """map_ref.point_data of the case data d; m defaults to ones (the binning does not read it)"""
    from map_ref import point_data
    m = np.ones(d["NE"] * d["NQ"]) if m is None else m
    return point_data(d["dim"], d["NE"], d["N"], d["D"], d["L"], d["h1map"], d["S"] if S is None else S, m, d["gamma"], d["W"], d["B"], d["G"],
                      d["Bl"])


def reference(pd, g):
    """map_ref.bin_points of the points pd under the grid g"""
    from map_ref import bin_points
    return bin_points(pd, g[1], g[2], g[3])
