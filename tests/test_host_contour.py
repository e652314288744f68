"""The host side of `-pv-iso` / `-pv-plane` without a GPU: WriteVtuContour, its .pvtu and the .pvd held to tests/vtu_reader.py (a
reader that knows nothing of the writer) - the bits of every array, cell types, offsets, ISO_VALUE, in 2D and 3D, for an empty piece
and for several ranks - and every refusal of the two options through the `laghos` executable, as tests/test_host_cli.py holds the
others: exit status 1, nothing on stdout but the 1D line, the complete stderr, nothing created."""
import os
import re
import subprocess

import numpy as np
import pytest

from vtu_reader import read_vtu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")
TO_FA = "Laghos does not support PA in 1D. Switching to FA.\n"
FIELDS = "density, energy, pressure, speed, x, y, z, div_v, detj or sound_speed"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def piece_arrays(dim, nprims, seed):
    rng = np.random.default_rng(seed)
    nv = dim * nprims
    a = dict(zone=rng.integers(0, 50, nprims).astype(np.int32), x=rng.normal(size=(dim, nv)), v=rng.normal(size=(dim, nv)), e=rng.normal(size=nv),
             rho=rng.uniform(1, 2, nv), p=rng.uniform(0, 1, nv))
    extra = [("div_v", 1, rng.normal(size=nv)), ("vorticity", 3, rng.normal(size=(nv, 3))), ("detJ", 1, rng.uniform(0.1, 1, nv))]
    return a, extra


@pytest.mark.parametrize("dim,nprims,rank,nranks", [(3, 7, 0, 1), (2, 5, 0, 1), (3, 0, 0, 1), (2, 0, 1, 3), (3, 4, 2, 3)])
def test_contour_piece(tmp_path, dim, nprims, rank, nranks):
    from laghos_amd import host_lib
    a, extra = piece_arrays(dim, nprims, 10 * dim + nprims)
    iso, cycle, time = 1.0 / 3.0, 12, 0.1 + 1e-17
    path = host_lib.host_write_vtu_contour(tmp_path / "c", dim, a["zone"], a["x"], a["v"], a["e"], a["rho"], a["p"], extra, iso, cycle, time, rank, nranks)
    assert os.path.basename(path) == "cycle_000012" + (f".{rank}" if nranks > 1 else "") + ".vtu"
    f = read_vtu(path)
    A, nv = f["arrays"], dim * nprims
    assert (f["npoints"], f["ncells"]) == (nv, nprims)
    assert [n for n, s in f["section"].items() if s == "FieldData"] == ["TIME", "CYCLE", "ISO_VALUE"]
    assert [n for n, s in f["section"].items() if s == "PointData"] == ["density", "velocity", "specific_internal_energy", "pressure", "div_v", "vorticity", "detJ"]
    assert [n for n, s in f["section"].items() if s == "CellData"] == ["zone", "rank"]
    assert bits(A["TIME"])[0] == bits(np.array([time]))[0] and A["CYCLE"][0] == cycle and bits(A["ISO_VALUE"])[0] == bits(np.array([iso]))[0]
    assert f["types"]["ISO_VALUE"] == "Float64" and f["types"]["zone"] == "Int32" and f["types"]["connectivity"] == "Int64"
    # cells: triangles (5) or lines (3) on points of their own
    assert np.all(A["types"] == (5 if dim == 3 else 3)) and len(A["types"]) == nprims
    assert np.array_equal(A["offsets"], dim * np.arange(1, nprims + 1)) and np.array_equal(A["connectivity"], np.arange(nv))
    assert np.array_equal(A["zone"], a["zone"]) and np.all(A["rank"] == rank) and len(A["rank"]) == nprims
    pad = lambda s: np.concatenate([s, np.zeros((3 - dim, nv))]).T
    want = {"Points": pad(a["x"]), "velocity": pad(a["v"]), "density": a["rho"], "specific_internal_energy": a["e"], "pressure": a["p"]}
    want.update({k: d for k, _, d in extra})
    for k, w in want.items():
        assert A[k].shape == np.asarray(w).shape and np.array_equal(bits(A[k]), bits(w)), k


def test_collections(tmp_path):
    from laghos_amd import host_lib
    d = tmp_path / "out" / "run_iso0_density"
    p = host_lib.host_write_pvtu_contour(d, 4, 0.25, 3, [("div_v", 1), ("vorticity", 3)])
    txt = open(p).read()
    assert os.path.basename(p) == "cycle_000004.pvtu"
    assert re.findall(r'<Piece Source="([^"]+)"/>', txt) == [f"cycle_000004.{r}.vtu" for r in range(3)]
    assert re.findall(r'<PDataArray type="(\w+)" Name="(\w+)" NumberOfComponents="(\d)"/>', txt) == [
        ("Float64", "Points", "3"), ("Float64", "density", "1"), ("Float64", "velocity", "3"), ("Float64", "specific_internal_energy", "1"),
        ("Float64", "pressure", "1"), ("Float64", "div_v", "1"), ("Float64", "vorticity", "3"), ("Int32", "zone", "1"), ("Int32", "rank", "1")]
    pvd = str(d) + ".pvd"
    host_lib.host_write_pvd(pvd, "run_iso0_density", [0.0, 0.25], [0, 4], 3)
    sets = re.findall(r'<DataSet timestep="([^"]+)" group="" part="0" file="([^"]+)"/>', open(pvd).read())
    assert sets == [("0", "run_iso0_density/cycle_000000.pvtu"), ("0.25", "run_iso0_density/cycle_000004.pvtu")]


def test_a_bad_piece_is_refused(tmp_path):
    from laghos_amd import host_lib
    a, extra = piece_arrays(3, 2, 1)
    with pytest.raises(RuntimeError):
        host_lib.host_write_vtu_contour(tmp_path / "c", 1, a["zone"], a["x"][:1, :2], a["v"][:1, :2], a["e"][:2], a["rho"][:2], a["p"][:2], [], 0.0, 0, 0.0)
    with pytest.raises(RuntimeError):
        host_lib.host_write_vtu_contour(tmp_path / "c", 3, a["zone"], a["x"], a["v"], a["e"], a["rho"], a["p"], [("", 1, a["e"])], 0.0, 0, 0.0)
    assert not os.path.exists(tmp_path / "c")


EIGHT_ISOS = sum((["-pv-iso", "density", str(k)] for k in range(8)), [])
EIGHT_PLANES = sum((["-pv-plane", "1", "0", "0", str(k)] for k in range(8)), [])
NO_1D = ": contours are formed in 2D and 3D, this mesh is 1D"

# (arguments, stderr without `laghos: ` and its newline[, stdout])
REFUSED = [
    (["-pv-iso"], "missing value for -pv-iso FIELD VALUE"),
    (["-pv-iso", "density"], "missing value for -pv-iso FIELD VALUE"),
    (["--paraview-iso", "density"], "missing value for --paraview-iso FIELD VALUE"),
    (["-pv-iso", "enstrophy", "1"], f"-pv-iso: unknown field enstrophy ({FIELDS})"),
    (["-pv-iso", "rho", "1"], f"-pv-iso: unknown field rho ({FIELDS})"),
    (["-pv-iso", "density", "abc"], "-pv-iso density abc: the value must be a finite number"),
    (["-pv-iso", "density", "1.5x"], "-pv-iso density 1.5x: the value must be a finite number"),
    (["-pv-iso", "pressure", "nan"], "-pv-iso pressure nan: the value must be a finite number"),
    (["-pv-iso", "pressure", "-inf"], "-pv-iso pressure -inf: the value must be a finite number"),
    (["-pv-iso", "density", "2", "-pv-iso", "energy", "2", "-pv-iso", "density", "2.0"], "-pv-iso density 2.0 is given twice"),
    (EIGHT_ISOS + ["-pv-iso", "energy", "0"], "-pv-iso energy 0: at most 8 iso-surfaces, this is the ninth"),
    (["-pv-plane"], "-pv-plane NX NY [NZ] D needs three numbers in 2D and four in 3D, got 0"),
    (["-pv-plane", "1", "2"], "-pv-plane NX NY [NZ] D needs three numbers in 2D and four in 3D, got 2"),
    (["-pv-plane", "1", "x", "2"], "-pv-plane NX NY [NZ] D needs three numbers in 2D and four in 3D, got 1"),
    (["-pv-plane", "0", "0", "0", "1"], "-pv-plane 0 0 0 1: the normal is zero"),
    (["-pv-plane", "0", "-0", "1"], "-pv-plane 0 -0 1: the normal is zero"),
    (["-pv-plane", "1", "inf", "0", "1"], "-pv-plane 1 inf 0 1: the normal and D must be finite numbers"),
    (["-pv-plane", "1", "1", "1", "nan"], "-pv-plane 1 1 1 nan: the normal and D must be finite numbers"),
    (["-pv-plane", "1", "1", "1", "1.5", "--paraview-plane", "1", "1", "1", "1.5"], "-pv-plane 1 1 1 1.5 is given twice"),
    (EIGHT_PLANES + ["-pv-plane", "0", "1", "0", "0.5"], "-pv-plane 0 1 0 0.5: at most 8 planes, this is the ninth"),
    (["-pv-iso", "density", "1", "-vr", "9"], "-vr / --vis-refine must be between 1 and 8, got 9"),
    (["-pv-plane", "1", "1", "1", "1.5", "-pv-fields", "nonsense"], "-pv-fields: unknown field nonsense (div_v, vorticity, grad_v, detj, sound_speed or all)"),
    # what the mesh decides
    (["-dim", "2", "-pv-plane", "1", "1", "1", "1.5"], "-pv-plane (plane0) has 4 numbers, a mesh of 2 dimensions needs 3"),
    (["-pv-plane", "1", "1", "1.5"], "-pv-plane (plane0) has 3 numbers, a mesh of 3 dimensions needs 4"),
    (["-pv-plane", "1", "1", "1", "1.5", "-pv-plane", "1", "2", "1"], "-pv-plane (plane1) has 3 numbers, a mesh of 3 dimensions needs 4"),
    (["-dim", "1", "-pv-iso", "density", "2"], "-pv-iso" + NO_1D, TO_FA),
    (["-dim", "1", "-pv-plane", "1", "0", "0.5"], "-pv-plane" + NO_1D, TO_FA),
    (["-m", "data/segment01.mesh", "-fa", "-pv-iso", "x", "0.5"], "-pv-iso" + NO_1D),
    (["-dim", "2", "-pv-iso", "z", "0.5"], "-pv-iso z: the mesh has 2 dimensions, there is no z axis"),
    (["-m", "data/square01_quad.mesh", "-pv-iso", "x", "0.5", "-pv-iso", "z", "0.5"], "-pv-iso z: the mesh has 2 dimensions, there is no z axis"),
    # -vr and -pv-fields are accepted with the two options alone: the refusal is the one further along the line
    (["-pv-iso", "density", "1", "-vr", "3", "-pv-fields", "div_v", "-bogus"], "unsupported option: -bogus"),
    (["-pv-plane", "1", "1", "1", "1.5", "-pv-fields", "all", "-dim", "1"], "-pv-plane" + NO_1D, TO_FA),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: " ".join(c[0])[:70])
def test_the_driver_refuses(case, tmp_path):
    args, message = case[0], case[1]
    stdout = case[2] if len(case) > 2 else ""
    env = {k: v for k, v in os.environ.items() if k != "LGH_FORCE_MULTI"}
    base = tmp_path / "base"
    base.mkdir()
    p = subprocess.run([EXE, "-k", str(base / "out" / "run")] + args, capture_output=True, text=True, timeout=60, cwd=ROOT, env=env)
    assert (p.returncode, p.stdout, p.stderr) == (1, stdout, "laghos: " + message + "\n")
    assert os.listdir(base) == []


def test_pv_fields_alone_is_still_refused(tmp_path):
    p = subprocess.run([EXE, "-k", str(tmp_path / "run"), "-pv-fields", "div_v"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert (p.returncode, p.stderr) == (1, "laghos: -pv-fields adds fields to the -paraview dumps: it needs -paraview\n")
