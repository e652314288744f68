"""tests/profile_ref.py, the numpy restatement the GPU tests of lgh_profile compare against, on its own (no GPU):
closed forms on an undeformed box, the decidedness of every (case, spec) the GPU tests use, and the reader of the driver's
files.

Bounds: a bin of the box holds n points whose addends w_q detJ_q are products of 1 + dim exact-to-rounding factors; the
row's fsum is correctly rounded, so |vol - exact| <= (dim + 3) 2^-52 vol for the quadrature's exactness to hold the rest:
a tensor Gauss rule integrates the constant 1 over a zone exactly, so a bin made of whole zones has the zones' volume.  The
spherical shells in 1D are segments: the same."""
import os

import numpy as np
import pytest

import profile_cases as pc
import profile_ref as pr

EPS = 2.0 ** -52


def box(zones, ok=2, ot=1):
    """the undeformed box [0, 1]^dim with rho = 1 (m_q = w_q detJ_q) and v = x - o, e = 1"""
    d = pc.case_data(zones, ok, ot)
    dim, N = d["dim"], d["N"]
    o = np.array([0.25, 0.5, 0.125])[:dim]
    S = d["S"].copy()
    S[:dim * N] = d["x0"]
    for c in range(dim):
        S[(dim + c) * N:(dim + c + 1) * N] = d["x0"][c * N:(c + 1) * N] - o[c]
    S[2 * dim * N:] = 1.0
    vol = np.prod([1.0 / n for n in zones])
    m = np.tile(d["W"] * vol, d["NE"])
    return d, S, m, o


@pytest.mark.parametrize("zones", [(4,), (4, 2), (4, 2, 2)], ids=["1D", "2D", "3D"])
def test_slabs_of_a_box_along_x(zones):
    """4 zones along x under 4 bins (bin = one layer of zones) and under 2 bins: volume and mass of a bin are the slab's
    volume; mxi / mass is the slab's centre (a Gauss rule integrates x exactly); v = x - o gives mom / mass = centre - o_x"""
    d, S, m, o = box(zones)
    dim = d["dim"]
    for nbins in (4, 2):
        ref = pr.profile_reference(dim, d["NE"], d["N"], d["D"], d["L"], d["h1map"], S, m, d["gamma"], d["W"], d["B"], d["G"], d["Bl"], 0, nbins, 0.0, 1.0)
        assert pr.undecided(ref) == 0 and ref["n_excluded"] == 0
        rows = ref["rows"]
        assert np.all(rows[[0, -1], :8] == 0) and np.all(np.isposinf(rows[[0, -1], 8])) and np.all(np.isneginf(rows[[0, -1], 9]))
        assert rows[:, 0].sum() == d["NE"] * d["NQ"] and np.all(rows[1:-1, 0] == d["NE"] * d["NQ"] // nbins)
        tol = (dim + 3 + d["ND"]) * EPS
        for b in range(nbins):
            r = rows[1 + b]
            centre = (b + 0.5) / nbins
            assert abs(r[1] - 1.0 / nbins) <= tol / nbins and abs(r[2] - 1.0 / nbins) <= tol / nbins
            assert abs(r[7] / r[2] - centre) <= 4 * tol and abs(r[5] / r[2] - (centre - o[0])) <= 4 * tol
            assert abs(r[3] - r[2]) <= tol * r[2]                       # e = 1
            assert abs(r[8] - 1.0) <= tol and abs(r[9] - 1.0) <= tol   # rho = 1


def test_shells_in_1d():
    """r = |x - 0.25| on 8 zones of [0, 1] under 3 bins of [0, 0.75): shell b is the two segments at distance [b/4, (b+1)/4)
    on either side of the origin where they lie inside the domain; v . n = r"""
    d, S, m, _ = box((8,))
    o = 0.25
    N = d["N"]
    S[N:2 * N] = d["x0"] - o
    ref = pr.profile_reference(1, d["NE"], N, d["D"], d["L"], d["h1map"], S, m, d["gamma"], d["W"], d["B"], d["G"], d["Bl"], 3, 3, 0.0, 0.75, (o,))
    assert pr.undecided(ref) == 0
    rows = ref["rows"]
    tol = (4 + d["ND"]) * EPS
    for b, vol in enumerate((0.5, 0.25, 0.25)):
        assert abs(rows[1 + b, 1] - vol) <= tol and abs(rows[1 + b, 2] - vol) <= tol
        assert abs(rows[1 + b, 5] - rows[1 + b, 7]) <= 4 * tol       # v . n = r: mom = mxi
    assert rows[0, 0] == 0 and rows[-1, 0] == 0


@pytest.mark.parametrize("zones_id,order", pc.CASES, ids=pc.IDS)
def test_every_gpu_case_is_decided(zones_id, order):
    """no point of a (case, spec) of tests/test_gpu_profile.py sits within 1e-9 of a bin edge, of detJ = 0 or of the origin"""
    d = pc.case_data(pc.ZONES[zones_id], *order)
    for spec in pc.specs(d["dim"]):
        ref = pc.reference(d, spec)
        assert pr.undecided(ref) == 0, spec[0]
        # (the random curving inverts a point of 3D-5x5x3 Q3Q2 and 27 of 3D-2x2x1 Q5Q4: the exclusion rule is in play in the plain cases too)
        assert ref["n_excluded"] * 100 < d["NE"] * d["NQ"] and ref["rows"][:, 0].sum() + ref["n_excluded"] == d["NE"] * d["NQ"], spec[0]
        if d["NE"] >= 12:
            assert (ref["rows"][1:-1, 0] > 0).sum() >= 3, spec[0]      # the points spread over the bins
    outside = pc.reference(d, pc.specs(d["dim"])[-1])
    if d["NE"] >= 3:
        assert outside["rows"][0, 0] > 0 and outside["rows"][1:-1, 0].sum() > 0   # r-outside: points below lo and inside


def test_the_reader_round_trips(tmp_path):
    text = ("# cycle t axis origin_x origin_y origin_z lo hi nbins n_excluded 6 0.0125 r 0 0 0 0 1.5 2 3\n"
            "row lo hi n vol mass ie ke mom pv mxi rho_min rho_max rho e v p xi rho_exact v_exact p_exact\n")
    rows = np.array([[0, 0, 0, 0, 0, 0, 0, 0, np.inf, -np.inf], [5, .5, .25, .125, 1e-3, -2e-3, .0625, .2, .4, .6],
                     [2, .25, .5, 1.0, 0, 0, .125, .6, 1.9, 2.1], [0, 0, 0, 0, 0, 0, 0, 0, np.inf, -np.inf]])
    exact = [[np.nan] * 3, [1.0, 0.5, 0.25], [6.0, 0.1, 0.3], [np.nan] * 3]
    text += "".join(pr.format_row(r, 2, 0.0, 1.5, rows[r], exact[r]) for r in range(4))
    path = os.path.join(tmp_path, "x_profile_000006.csv")
    open(path, "w").write(text)
    head, columns, got, lines = pr.read_profile(path)
    assert head == dict(cycle=6, t=0.0125, axis="r", origin_x=0.0, origin_y=0.0, origin_z=0.0, lo=0.0, hi=1.5, nbins=2, n_excluded=3)
    assert columns == pr.FILE_COLUMNS + pr.EXACT_COLUMNS and len(got) == 4 and "".join(lines) == text
    assert got[0]["lo"] == -np.inf and got[0]["hi"] == 0.0 and got[3]["hi"] == np.inf and got[1]["lo"] == 0.0 and got[1]["hi"] == 0.75
    assert got[1]["n"] == 5 and got[1]["rho"] == 0.25 / 0.5 and got[1]["xi"] == 0.2 / 0.25 and np.isnan(got[0]["rho"]) and np.isnan(got[0]["rho_exact"])
    assert got[2]["rho_exact"] == 6.0 and got[2]["p"] == 0.125 / 0.25 and got[0]["rho_min"] == np.inf and got[3]["rho_max"] == -np.inf
    for r in range(4):   # a row formatted again from the values read back is the line itself: every value reads back exactly
        d = [got[r][k] for k in pr.COLS]
        assert pr.format_row(r, 2, 0.0, 1.5, d, [got[r][k] for k in pr.EXACT_COLUMNS]) == lines[2 + r]
