"""The gauges without a GPU: the numpy reference (tests/gauges_ref.py) against itself in long double, to a quarter of the bars
tests/test_gpu_gauges.py holds the GPU to, as tests/test_derived_ref.py does for the lattice; the host library's bases at an
arbitrary abscissa against the formulas and against its own lattice tables; its location of a point in the initial mesh against
the restated rule - at break points, corners, the closed last interval, outside points and NaN; and the text of the file."""
import numpy as np
import pytest

import gauges_ref as gr
from derived_ref import TOL, curved_state

ZONES = {"1D-1": (1,), "1D-257": (257,), "2D-3x2": (3, 2), "3D-3x2x2": (3, 2, 2), "3D-5x5x3": (5, 5, 3)}
ORDERS = [(1, 0), (2, 1), (3, 2)]
CASES = [(z, o) for z in ZONES for o in ORDERS] + [("2D-3x2", (4, 3)), ("3D-3x2x2", (5, 4))]   # those of tests/test_gpu_gauges.py


def gauges_of(c, n=13):
    rng = np.random.default_rng(100 * c["dim"] + c["NE"])
    zone = rng.integers(0, c["NE"], n)
    xi = rng.uniform(0.02, 0.98, (n, c["dim"]))
    for g in range(0, n, 3):
        xi[g, rng.integers(0, c["dim"])] = float(rng.integers(0, 2))
    xi[0], xi[n - 1] = 0.0, 1.0
    return zone, xi


@pytest.mark.parametrize("zones_id,order", CASES, ids=[f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES])
def test_reference_in_long_double_against_itself(zones_id, order):
    c = curved_state(ZONES[zones_id], *order)
    dim, N = c["dim"], c["N"]
    zone, xi = gauges_of(c)
    rho0 = np.random.default_rng(1).uniform(0.5, 2.0, c["NE"] * c["L"] ** dim)
    out = {}
    for dt in (np.float64, np.longdouble):
        T = gr.tables_at(c["ok"], c["ot"], xi, dt)
        m, r0 = gr.gauges_mass_reference(dim, c["NE"], N, c["D"], c["L"], c["h1map"], c["S"][:dim * N], rho0, zone, *T)
        out[dt] = (gr.gauges_reference(dim, c["NE"], N, c["D"], c["L"], c["h1map"], c["S"], c["gamma"], zone, *T, m), m, r0)
    (a, ma, ra), (b, mb, rb) = out[np.float64], out[np.longdouble]
    assert b["rows"].dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
    H1V = dim * N
    err = np.abs((a["rows"] - b["rows"]).astype(np.float64))
    scale = {0: np.abs(c["S"][:H1V]).max(), 3: np.abs(c["S"][H1V:2 * H1V]).max(), 7: np.abs(c["S"][2 * H1V:]).max()}
    assert err[:, 0:3].max() <= 0.25 * TOL * scale[0] and err[:, 3:6].max() <= 0.25 * TOL * scale[3] and err[:, 7].max() <= 0.25 * TOL * scale[7]
    rD, rL = np.max(err[:, 10] / (TOL * a["bound_det"])), np.max(err[:, 11] / (dim * TOL * a["bound_L"]))
    print(f"{zones_id} Q{order[0]}Q{order[1]}: reference error / bound: detj {rD:.4f}, div_v {rL:.4f}")
    assert rD <= 0.25 and rL <= 0.25
    # the mass: rho0 to a quarter of TOL of its largest dof, the determinant to a quarter of its bound
    bar = TOL * (np.abs(rho0).max() * np.abs(a["rows"][:, 10]) + np.abs(ra) * a["bound_det"])
    assert np.all(np.abs((ma - mb).astype(np.float64)) <= 0.25 * bar)
    # what follows from them, in the reference's own numbers: rho m_g / detj, p and cs from rho, e and gamma
    g = c["gamma"][zone]
    assert np.array_equal(a["rows"][:, 6], ma / a["rows"][:, 10])
    assert np.array_equal(a["rows"][:, 8], (g - 1) * a["rows"][:, 6] * np.maximum(a["rows"][:, 7], 0))
    assert np.array_equal(a["rows"][:, 9], np.sqrt((g * (g - 1)) * np.maximum(a["rows"][:, 7], 0)))
    assert not a["rows"][:, dim:3].any() and not a["rows"][:, 3 + dim:6].any()


def test_reference_on_closed_forms():
    """An affine velocity v = A x + b on the curved mesh has div v = tr A at every gauge; x(xi) at a corner is the node there"""
    from derived_ref import affine_velocity
    c = curved_state((3, 2, 2), 3, 2)
    A, b = np.random.default_rng(2).uniform(-1, 1, (3, 3)), np.array([1.0, 2.0, 3.0])
    S = affine_velocity(c["S"], 3, c["N"], A, b)
    zone, xi = gauges_of(c)
    T = gr.tables_at(3, 2, xi)
    ref = gr.gauges_reference(3, c["NE"], c["N"], 4, 3, c["h1map"], S, c["gamma"], zone, *T, np.ones(len(zone)))
    assert np.all(np.abs(ref["rows"][:, 11] - np.trace(A)) <= 3 * TOL * ref["bound_L"])
    assert np.all(np.abs(ref["rows"][:, 3:6] - (ref["rows"][:, 0:3] @ A.T + b)) <= 1e-13 * 10)
    hm = np.asarray(c["h1map"]).reshape(c["NE"], 4, 4, 4)
    X = c["S"][:3 * c["N"]].reshape(3, c["N"])
    assert np.array_equal(ref["rows"][0, 0:3], X[:, hm[zone[0], 0, 0, 0]]) and np.array_equal(ref["rows"][-1, 0:3], X[:, hm[zone[-1], 3, 3, 3]])


@pytest.mark.parametrize("order", [(1, 0), (2, 1), (3, 2), (4, 3), (8, 7)])
def test_host_bases_at_an_abscissa(order):
    from laghos_amd import host_lib
    ok, ot = order
    xs = np.concatenate([[0.0, 1.0, 0.5, 1.0 / 3.0], np.random.default_rng(3).uniform(0, 1, 9)])
    want = gr.tables_at(ok, ot, xs.reshape(-1, 1))
    for k, x in enumerate(xs):
        Bh, Gh, Bl = host_lib.host_basis_at(ok, ot, x)
        # (the two sides take other nodes - Newton against numpy's roots - that agree to a few ulp: tests/test_derived_ref.py)
        assert np.abs(Bh - want[0][k, 0]).max() <= 1e-12 and np.abs(Bl - want[2][k, 0]).max() <= 1e-12
        assert np.abs(Gh - want[1][k, 0]).max() <= 1e-12 * np.abs(want[1][k, 0]).max()
        assert abs(Bh.sum() - 1) <= 1e-13 and abs(Bl.sum() - 1) <= 1e-13 and abs(Gh.sum()) <= 1e-12 * np.abs(Gh).max()
    # at r / R it is row r of the lattice tables, to the bit: a gauge at a lattice point has the tables of the dumps
    for R in (1, 2, 8):
        Bh_lat, Bl_lat = host_lib.host_lattice_tables(ok, ot, R)
        Gh_lat = host_lib.host_lattice_grad_table(ok, R)
        for r in range(R + 1):
            Bh, Gh, Bl = host_lib.host_basis_at(ok, ot, r / R)
            assert np.array_equal(Bh, Bh_lat[r]) and np.array_equal(Gh, Gh_lat[r]) and np.array_equal(Bl, Bl_lat[r])
    T = host_lib.host_gauge_tables(ok, ot, np.array([[0.25, 0.75], [1.0, 0.0]]))
    assert [t.shape for t in T] == [(2, 2, ok + 1), (2, 2, ok + 1), (2, 2, ot + 1)]
    assert np.array_equal(T[0][1, 0], host_lib.host_basis_at(ok, ot, 1.0)[0]) and np.array_equal(T[2][0, 1], host_lib.host_basis_at(ok, ot, 0.75)[2])


def graded(n, seed, lo=-0.5, length=2.0):
    w = 1.0 + 0.25 * np.random.default_rng(seed).uniform(-1, 1, n)
    b = lo + length * np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
    b[-1] = lo + length
    return b


@pytest.mark.parametrize("shape", [(1,), (7,), (4, 3), (3, 2, 5)])
def test_host_location_in_the_initial_mesh(shape):
    from laghos_amd import host_lib
    dim = len(shape)
    breaks = [graded(n, 10 * a + n) for a, n in enumerate(shape)]
    rng = np.random.default_rng(4)
    pts = [[b[0] for b in breaks], [b[-1] for b in breaks]]                                   # the two far corners
    pts += [[b[rng.integers(0, len(b))] for b in breaks] for _ in range(12)]                  # break points: corners of zones
    pts += [[rng.uniform(b[0], b[-1]) for b in breaks] for _ in range(12)]                    # interior points
    pts += [[b[-1] if a == k % dim else rng.uniform(b[0], b[-1]) for a, b in enumerate(breaks)] for k in range(3)]   # on the closed last faces
    for X in pts:
        got, (ijk, xi) = host_lib.host_locate_initial(breaks, X), gr.locate_initial(breaks, X)
        assert got is not None and got[0] == ijk and got[1] == xi, X                           # the same zone, the same bits
        for a, b in enumerate(breaks):
            assert 0 <= ijk[a] < shape[a] and 0.0 <= xi[a] <= 1.0
            last = ijk[a] == shape[a] - 1
            assert xi[a] < 1.0 or (last and X[a] == b[-1])                                     # [brk_i, brk_i+1), the last interval closed
            if X[a] in b[:-1]:
                assert xi[a] == 0.0 and b[ijk[a]] == X[a]                                      # a break point opens its interval
            assert abs(b[ijk[a]] + xi[a] * (b[ijk[a] + 1] - b[ijk[a]]) - X[a]) <= 4 * np.finfo(float).eps * max(abs(X[a]), 1.0)
    assert host_lib.host_locate_initial(breaks, [b[-1] for b in breaks])[0] == [n - 1 for n in shape]
    assert host_lib.host_locate_initial(breaks, [b[-1] for b in breaks])[1] == [1.0] * dim
    inside = [0.5 * (b[0] + b[-1]) for b in breaks]
    for a, b in enumerate(breaks):
        for bad in (np.nextafter(b[0], -np.inf), np.nextafter(b[-1], np.inf), b[0] - 1.0, b[-1] + 10.0, np.nan, np.inf, -np.inf):
            X = list(inside)
            X[a] = bad
            assert host_lib.host_locate_initial(breaks, X) is None, (a, bad)
            with pytest.raises(ValueError):
                gr.locate_initial(breaks, X)


def test_host_text_of_a_sample():
    from laghos_amd import host_lib
    assert host_lib.host_gauges_header() == gr.HEADER == " ".join(host_lib.GAUGES_FILE_COLUMNS)
    rows = np.random.default_rng(5).uniform(-1, 1, (3, 12)) * 10.0 ** np.random.default_rng(6).integers(-12, 12, (3, 12))
    rows[0, 2] = rows[0, 5] = 0.0
    rows[1, 6:] = [np.nan, -np.inf, np.inf, -0.0, 1e-310, -np.nan]
    text = host_lib.host_gauges_text(12, 0.1 + 0.2, rows)
    assert text == gr.gauges_text(12, 0.1 + 0.2, rows)
    lines = text.splitlines()
    assert len(lines) == 3 and [l.split()[2] for l in lines] == ["0", "1", "2"] and all(l.startswith("12 0.30000000000000004 ") for l in lines)
    cells = lines[1].split()[9:]
    assert cells[:4] == ["nan", "-inf", "inf", "-0"] and cells[5] == "nan"
    for l, r in zip(lines, rows):                                                              # every finite value reads back exactly
        back = np.array([float(x) for x in l.split()[3:]])
        assert np.array_equal(back[np.isfinite(r)], r[np.isfinite(r)])
