"""tests/map_ref.py, the numpy restatement the GPU tests of lgh_map compare against, on its own (no GPU): closed forms on an
undeformed box, the decidedness of every (case, grid) the GPU tests use, and its agreement with tests/profile_ref.py where a
map is a profile.

Bounds: as tests/test_profile_ref.py - a cell made of whole zones of the box has the zones' volume to (dim + 3 + ND) 2^-52,
because a tensor Gauss rule integrates a constant over a zone exactly and the row's fsum is correctly rounded."""
import numpy as np
import pytest

import map_cases as mc
import map_ref as mr
import profile_ref as pr
from test_profile_ref import box

EPS = 2.0 ** -52


def ref_of(d, S, m, g):
    return mr.map_reference(d["dim"], d["NE"], d["N"], d["D"], d["L"], d["h1map"], S, m, d["gamma"], d["W"], d["B"], d["G"], d["Bl"], g[1], g[2], g[3])


@pytest.mark.parametrize("zones", [(4,), (4, 2), (4, 2, 2)], ids=["1D", "2D", "3D"])
def test_cells_of_a_box(zones):
    """the undeformed box under a grid whose cells are whole zones, and under one of two zones per cell along x: volume and
    mass of a cell are the cell's volume, mom / mass is centre - o (v = x - o), e = 1, rho = 1, nothing is outside"""
    d, S, m, o = box(zones)
    dim = d["dim"]
    for nx in (4, 2):
        cells = (nx,) + tuple(zones[1:])
        ref = ref_of(d, S, m, ("box", cells, (0.0,) * dim, (1.0,) * dim))
        assert mr.undecided(ref) == 0 and ref["n_excluded"] == 0
        rows = ref["rows"]
        ncells = int(np.prod(cells))
        assert rows.shape == (ncells + 1, 11) and np.all(rows[0, :9] == 0) and rows[0, 9] == np.inf and rows[0, 10] == -np.inf
        assert np.all(rows[1:, 0] == d["NE"] * d["NQ"] // ncells)
        tol = (dim + 3 + d["ND"]) * EPS
        vol = 1.0 / ncells
        full = list(cells) + [1] * (3 - dim)
        for r in range(1, ncells + 1):
            b = ((r - 1) % full[0], ((r - 1) // full[0]) % full[1], (r - 1) // (full[0] * full[1]))
            assert abs(rows[r, 1] - vol) <= tol * vol and abs(rows[r, 2] - vol) <= tol * vol and abs(rows[r, 3] - rows[r, 2]) <= tol * vol
            for c in range(3):
                if c < dim:
                    assert abs(rows[r, 5 + c] / rows[r, 2] - ((b[c] + 0.5) / full[c] - o[c])) <= 4 * tol
                else:
                    assert rows[r, 5 + c] == 0.0 and not np.signbit(rows[r, 5 + c])
            assert abs(rows[r, 9] - 1.0) <= tol and abs(rows[r, 10] - 1.0) <= tol


@pytest.mark.parametrize("zones_id,order", mc.CASES, ids=mc.IDS)
def test_every_gpu_case_is_decided(zones_id, order):
    """no point of a (case, grid) of tests/test_gpu_map.py sits within 1e-9 of a cell edge or of detJ = 0; the counts add up;
    `partial` leaves points on both sides of the box; the slab is the profile along x"""
    d = mc.case_data(mc.ZONES[zones_id], *order)
    dim, npts = d["dim"], d["NE"] * d["NQ"]
    pd = mc.points(d)
    for g in mc.grids(dim):
        ref = mc.reference(pd, g)
        assert mr.undecided(ref) == 0, g[0]
        assert ref["rows"].shape == (int(np.prod(g[1])) + 1, 11)
        assert ref["n_excluded"] * 100 < npts and ref["rows"][:, 0].sum() + ref["n_excluded"] == npts, g[0]
        assert np.all(ref["cond"] >= ref["abs"] * (1 - 8 * EPS))
        if g[0] == "one":                                            # (the curved boundary leaves [0, 1]^d, never [-1, 2]^d)
            assert ref["rows"][0, 0] == 0 and ref["rows"][1, 0] == npts - ref["n_excluded"]
    if d["NE"] >= 3:
        part = mc.reference(pd, mc.grid("partial", dim))["rows"]
        assert part[0, 0] > 0 and part[1:, 0].sum() > 0
        if dim > 1:                                                   # (1D: the box is 55 % of the domain)
            assert 0.5 * npts <= part[0, 0] <= 0.85 * npts
    prof = pr.profile_reference(dim, d["NE"], d["N"], d["D"], d["L"], d["h1map"], d["S"], np.ones(npts), d["gamma"], d["W"], d["B"], d["G"],
                                d["Bl"], 0, 9, 0.0, 1.0)
    wide = mc.reference(pd, mc.slab_wide(dim))
    assert mr.undecided(wide) == 0
    # the same addends in the same rows: fsum gives the same bits (columns n, vol, mass, ie, ke, mom_x <-> mom, pv, rho_min, rho_max)
    assert np.array_equal(wide["rows"][1:, mc.SLAB_COLS], prof["rows"][1:-1, mc.PROFILE_COLS])
    # `slab` itself ends at y, z = 0 and 1, which the curved boundary crosses: those points are outside for the map and in their
    # bin for the profile, so the two agree in the rows that lose no point (in 1D: in all of them)
    slab = mc.reference(pd, mc.grid("slab", dim))["rows"][1:]
    same = slab[:, 0] == prof["rows"][1:-1, 0]
    assert np.array_equal(slab[same][:, mc.SLAB_COLS], prof["rows"][1:-1][same][:, mc.PROFILE_COLS]) and (dim > 1 or same.all())


def test_inverted_points_are_covered():
    """3D-5x5x3 Q3Q2 and 3D-2x2x1 Q5Q4 hold inverted points: the exclusion rule is in play in the plain cases"""
    for zid, order in (("3D-5x5x3", (3, 2)), ("3D-2x2x1", (5, 4))):
        assert mc.points(mc.case_data(mc.ZONES[zid], *order))["n_excluded"] > 0
