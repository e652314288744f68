"""Host side of the `-paraview` dumps, no GPU: the lattice tables of the visualisation sampling (fem.cpp LatticeTables)
against a numpy restatement (tests/lattice_ref.py), and the VTK writers (vtk_output.cpp) read back by a parser of the
tests' own - XML header plus the raw appended blocks (tests/vtu_reader.py)."""
import os
import re

import numpy as np
import pytest

from laghos_amd import host_lib
from lattice_ref import bernstein_table, gll_nodes, lagrange_table
from vtu_reader import read_vtu


# ---- lattice tables -------------------------------------------------------------------------------------
ORDERS = [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4)]


@pytest.mark.parametrize("R", [1, 2, 5, 8])
@pytest.mark.parametrize("ok,ot", ORDERS)
def test_lattice_tables_match_numpy(ok, ot, R):
    Bh, Bl = host_lib.host_lattice_tables(ok, ot, R)
    pts = np.arange(R + 1) / R
    assert Bh.shape == (R + 1, ok + 1) and Bl.shape == (R + 1, ot + 1)
    assert np.abs(Bh - lagrange_table(gll_nodes(ok + 1), pts)).max() < 1e-14
    assert np.abs(Bl - bernstein_table(ot, pts)).max() < 1e-14
    # partition of unity at every abscissa
    assert np.abs(Bh.sum(axis=1) - 1.0).max() < 1e-14
    assert np.abs(Bl.sum(axis=1) - 1.0).max() < 1e-14
    # the end points are nodes: unit vectors
    e0, e1 = np.zeros(ok + 1), np.zeros(ok + 1)
    e0[0], e1[-1] = 1.0, 1.0
    assert np.abs(Bh[0] - e0).max() < 1e-15 and np.abs(Bh[R] - e1).max() < 1e-15


# ---- writer round trip ------------------------------------------------------------------------------------
GRID = {1: (3, 1, 1), 2: (3, 2, 1), 3: (3, 2, 2)}


def lattice_points(dim, R1):
    """the undeformed lattice of a grid of unit zones: x[c, e * R1^dim + rx + R1 (ry + R1 rz)]"""
    nx, ny, nz = GRID[dim]
    NE, NPZ = nx * ny * nz, R1 ** dim
    x = np.zeros((dim, NE * NPZ))
    for e in range(NE):
        org = (e % nx, (e // nx) % ny, e // (nx * ny))
        for pt in range(NPZ):
            r = (pt % R1, (pt // R1) % R1, pt // (R1 * R1))
            for c in range(dim):
                x[c, e * NPZ + pt] = org[c] + r[c] / (R1 - 1)
    return NE, x


@pytest.mark.parametrize("R1", [2, 4])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_vtu_round_trip(dim, R1, tmp_path):
    NE = int(np.prod(GRID[dim]))
    NPZ, R = R1 ** dim, R1 - 1
    NP, NCZ = NE * NPZ, R ** dim
    rng = np.random.default_rng(100 * dim + R1)
    x, v = rng.standard_normal((dim, NP)), rng.standard_normal((dim, NP))
    e, rho, p = rng.standard_normal(NP), rng.standard_normal(NP), rng.standard_normal(NP)
    path = host_lib.host_write_vtu(tmp_path / "a" / "b_paraview", dim, NE, R1, x, v, e, rho, p, cycle=12, time=0.3125)
    assert os.path.basename(path) == "cycle_000012.vtu" and os.path.exists(path)
    f = read_vtu(path)
    assert f["attrs"]["byte_order"] == "LittleEndian" and f["attrs"]["header_type"] == "UInt64"
    assert f["npoints"] == NP and f["ncells"] == NE * NCZ
    a = f["arrays"]
    for name in ("Points", "density", "velocity", "specific_internal_energy", "pressure"):
        assert a[name].dtype == np.float64, name
    pad = lambda s: np.concatenate([s, np.zeros((3 - dim, NP))]).T
    assert np.array_equal(a["Points"], pad(x)) and np.array_equal(a["velocity"], pad(v))       # bit for bit
    assert np.array_equal(a["density"], rho) and np.array_equal(a["specific_internal_energy"], e)
    assert np.array_equal(a["pressure"], p)
    # cells
    nv = 2 ** dim
    conn, offs, types = a["connectivity"], a["offsets"], a["types"]
    assert np.array_equal(offs, nv * np.arange(1, NE * NCZ + 1))
    assert np.all(types == {1: 3, 2: 9, 3: 12}[dim])
    assert conn.min() >= 0 and conn.max() < NP
    cells = conn.reshape(NE * NCZ, nv)
    assert np.array_equal(cells // NPZ, np.repeat(np.arange(NE), NCZ)[:, None] * np.ones(nv, dtype=np.int64))  # own points only
    assert a["zone"].dtype == np.int32 and a["rank"].dtype == np.int32
    assert np.array_equal(a["zone"], np.repeat(np.arange(NE), NCZ)) and np.all(a["rank"] == 0)
    assert a["TIME"].dtype == np.float64 and a["TIME"][0] == 0.3125
    assert a["CYCLE"].dtype == np.int32 and a["CYCLE"][0] == 12
    # every point of a zone is used, every cell once
    for z in range(NE):
        assert set(cells[z * NCZ:(z + 1) * NCZ].ravel()) == set(range(z * NPZ, (z + 1) * NPZ))
    assert len({tuple(sorted(c)) for c in cells}) == NE * NCZ


@pytest.mark.parametrize("R1", [2, 4])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_vtu_corner_order_on_the_undeformed_lattice(dim, R1, tmp_path):
    """VTK's corner order: along x; counter-clockwise quads; hexahedra bottom face counter-clockwise, then the top face -
    every cell of the undeformed lattice is the axis-aligned box of edge 1/R with positive signed volume"""
    NE, x = lattice_points(dim, R1)
    NP = x.shape[1]
    z = np.zeros(NP)
    path = host_lib.host_write_vtu(tmp_path, dim, NE, R1, x, x, z, z, z, cycle=0, time=0.0)
    a = read_vtu(path)["arrays"]
    P = a["Points"][a["connectivity"].reshape(-1, 2 ** dim)]       # (cells, corners, 3)
    h = 1.0 / (R1 - 1)
    ex, ey, ez = np.array([h, 0, 0]), np.array([0, h, 0]), np.array([0, 0, h])
    want = {1: [0 * ex, ex], 2: [0 * ex, ex, ex + ey, ey],
            3: [0 * ex, ex, ex + ey, ey, ez, ex + ez, ex + ey + ez, ey + ez]}[dim]
    for k, off in enumerate(want):
        assert np.abs(P[:, k] - P[:, 0] - off).max() < 1e-14, (k, "corner order")
    if dim == 1:
        vol = P[:, 1, 0] - P[:, 0, 0]
    elif dim == 2:   # shoelace formula
        nxt = np.roll(P, -1, axis=1)
        vol = 0.5 * np.sum(P[:, :, 0] * nxt[:, :, 1] - nxt[:, :, 0] * P[:, :, 1], axis=1)
    else:
        vol = np.linalg.det(np.stack([P[:, 1] - P[:, 0], P[:, 3] - P[:, 0], P[:, 4] - P[:, 0]], axis=1))
    assert np.all(vol > 0) and np.abs(vol - h ** dim).max() < 1e-13


# ---- several ranks, collections -----------------------------------------------------------------------------
def test_multirank_piece_pvtu_and_pvd(tmp_path):
    dim, R1 = 2, 3
    NE, x = lattice_points(dim, R1)
    z = np.zeros(x.shape[1])
    d = tmp_path / "run_paraview"
    for rank in (0, 1):
        path = host_lib.host_write_vtu(d, dim, NE, R1, x, x, z, z, z, cycle=7, time=0.5, rank=rank, nranks=2)
        assert os.path.basename(path) == f"cycle_000007.{rank}.vtu" and os.path.exists(path)
        assert np.all(read_vtu(path)["arrays"]["rank"] == rank)
    pvtu = host_lib.host_write_pvtu(d, 7, 0.5, 2)
    assert os.path.basename(pvtu) == "cycle_000007.pvtu"
    txt = open(pvtu).read()
    assert 'type="PUnstructuredGrid"' in txt
    assert re.findall(r'<Piece Source="([^"]+)"', txt) == ["cycle_000007.0.vtu", "cycle_000007.1.vtu"]
    piece = read_vtu(path)
    declared = {m.group(2): (m.group(1), m.group(3)) for m in
                re.finditer(r'<PDataArray type="(\w+)" Name="(\w+)"(?: NumberOfComponents="(\d+)")?', txt)}
    # (the point and cell arrays and the points; TIME and CYCLE are field data of each piece)
    assert set(declared) == set(piece["arrays"]) - {"connectivity", "offsets", "types", "TIME", "CYCLE"}
    for name, (typ, ncomp) in declared.items():
        assert typ == piece["types"][name], name
        if ncomp is not None:
            assert int(ncomp) == piece["ncomp"][name], name
    # the collection: dumps in order, with their times
    times, cycles = [0.0, 0.1234567890123456, 0.3], [0, 2, 3]
    for nranks, ext in ((1, "vtu"), (2, "pvtu")):
        pvd = tmp_path / f"run{nranks}.pvd"
        host_lib.host_write_pvd(pvd, "run_paraview", times, cycles, nranks)
        txt = open(pvd).read()
        assert 'type="Collection"' in txt
        sets = re.findall(r'<DataSet timestep="([^"]+)"[^>]* file="([^"]+)"', txt)
        assert [float(t) for t, _ in sets] == times
        assert [f for _, f in sets] == [f"run_paraview/cycle_{c:06d}.{ext}" for c in cycles]
