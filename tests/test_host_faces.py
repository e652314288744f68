"""The parts of the surface / slice dumps that need no GPU: lgh_mesh_boundary_faces_host against a brute-force search over node
sets, the float64 reference of the area vector (tests/faces_ref.py) against itself in long double on the cases of
tests/test_gpu_faces.py, the face writer read back (tests/faces_ref.py on tests/vtu_reader.py), and the driver's refusals, which
come before anything touches the GPU."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from derived_ref import TOL, curved_state, derived_reference, lattice_tables3
from faces_ref import area_normal_reference, brute_boundary_faces, face_volume_index, read_face_vtu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

MESHES = {"3D-1x1x1": (1, 1, 1), "3D-3x2x2": (3, 2, 2), "2D-3x2": (3, 2), "2D-1x1": (1, 1)}


def mesh(zones, order, renumber):
    from laghos_amd import host_lib
    d = host_lib.host_disc("cartesian", 0, order, max(order - 1, 0), 1, zones=zones, renumber=renumber, seed=3)
    hm = d["h1map"]
    return len(zones), int(np.prod(zones)), int(hm.max()) + 1, order + 1, hm, d


@pytest.mark.parametrize("renumber", [None, "mfem", "random"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("mesh_id", list(MESHES))
def test_boundary_faces_against_brute_force(mesh_id, order, renumber):
    from laghos_amd.context import boundary_faces_host
    zones = MESHES[mesh_id]
    dim, NE, N, D, hm, d = mesh(zones, order, renumber)
    got = boundary_faces_host(dim, NE, N, D, hm)
    want = brute_boundary_faces(dim, NE, D, hm)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # ascending (zone, face), and as many as the box has: 2 sum over axes of the product of the other zone counts
    assert np.array_equal(got, got[np.lexsort((got[:, 1], got[:, 0]))])
    assert len(got) == 2 * sum(NE // n for n in zones)
    # ... and they are the faces on the box: a structured zone (ex, ey, ez) has face 2a at e_a == 0, 2a + 1 at e_a == n_a - 1
    perm = d["elem_perm"] if len(d["elem_perm"]) else np.arange(NE)
    expect = []
    for j in range(NE):
        l = int(perm[j])
        for a, n in enumerate(zones):
            if l % n == 0:
                expect.append((j, 2 * a))
            if l % n == n - 1:
                expect.append((j, 2 * a + 1))
            l //= n
    assert np.array_equal(got, np.array(expect, np.int32))


@pytest.mark.parametrize("dim", [2, 3])
def test_boundary_faces_of_two_blocks_without_a_common_node(dim):
    from laghos_amd.context import boundary_faces_host
    za, zb = ((3, 2, 2), (1, 2, 1)) if dim == 3 else ((3, 2), (2, 1))
    _, NEa, Na, D, ha, _ = mesh(za, 2, "random")
    _, NEb, Nb, _, hb, _ = mesh(zb, 2, None)
    hm = np.concatenate([ha, hb + Na]).astype(np.int32)
    got = boundary_faces_host(dim, NEa + NEb, Na + Nb, D, hm)
    assert np.array_equal(got, brute_boundary_faces(dim, NEa + NEb, D, hm))
    assert len(got) == 2 * sum(NEa // n for n in za) + 2 * sum(NEb // n for n in zb)
    # the blocks touching at one face: that face of both is interior
    shared = hm.copy().reshape(NEa + NEb, -1)
    from faces_ref import face_nodes
    lo, hi = face_nodes(dim, D, 0), face_nodes(dim, D, 1)
    e_hi = next(e for e in range(NEa) if (e, 1) in {tuple(x) for x in got.tolist()})
    shared[NEa][lo] = shared[e_hi][hi]
    got2 = boundary_faces_host(dim, NEa + NEb, Na + Nb, D, shared.reshape(-1))
    assert np.array_equal(got2, brute_boundary_faces(dim, NEa + NEb, D, shared))
    gone = {tuple(x) for x in got.tolist()} - {tuple(x) for x in got2.tolist()}
    assert gone == {(e_hi, 1), (NEa, 0)}


def test_boundary_faces_refuses_a_node_out_of_range():
    from laghos_amd._lib import LghError
    from laghos_amd.context import boundary_faces_host
    hm = np.arange(8, dtype=np.int32)
    assert len(boundary_faces_host(3, 1, 8, 2, hm)) == 6
    hm[5] = 8
    with pytest.raises(LghError, match=r"h1_map\[5\] = 8"):
        boundary_faces_host(3, 1, 8, 2, hm)


# ---- the reference of the area vector -------------------------------------------------------------------------------
ZONES = {"2D-1x1": (1, 1), "2D-3x2": (3, 2), "3D-1x1x1": (1, 1, 1), "3D-3x2x2": (3, 2, 2), "3D-5x5x3": (5, 5, 3)}
SMALL = ("2D-1x1", "2D-3x2", "3D-1x1x1")
CASES = [(z, o) for z in ZONES for o in [(1, 0), (2, 1), (3, 2)]] + [(z, (4, 3)) for z in SMALL]   # those of tests/test_gpu_faces.py
R1S = [2, 3, 6, 9]


def all_faces(dim, NE):
    return np.stack([np.repeat(np.arange(NE), 2 * dim), np.tile(np.arange(2 * dim), NE)], 1).astype(np.int32)


def normal_bound(c, R1, faces):
    """The bound tests/test_gpu_derived.py applies to det J, per face lattice point: TOL |A_J|_F |J^-1|_F |det J| (the entries of
    adj(J) are sub-determinants of the same J: |A_J|_F |adj J|_F is this very product)"""
    T = lattice_tables3(c["ok"], c["ot"], R1 - 1)
    ref = derived_reference(c["dim"], c["NE"], c["N"], c["D"], c["L"], c["h1map"], c["S"], c["gamma"], *T)
    return TOL * ref["bound_det"][face_volume_index(c["dim"], R1, faces)]


@pytest.mark.parametrize("zones_id,order", CASES, ids=[f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES])
def test_area_normal_reference_in_long_double_against_itself(zones_id, order):
    """The float64 reference carries its own rounding: against the same formulas in long double it stays within a quarter of
    the bound the GPU is held to, on every case of the GPU test."""
    c = curved_state(ZONES[zones_id], *order)
    dim, faces = c["dim"], all_faces(c["dim"], c["NE"])
    assert np.finfo(np.longdouble).eps < 1e-18
    for R1 in R1S:
        Bh, Gh, _ = lattice_tables3(c["ok"], c["ot"], R1 - 1)
        Bq, Gq, _ = lattice_tables3(c["ok"], c["ot"], R1 - 1, np.longdouble)
        a = area_normal_reference(dim, c["NE"], c["N"], c["D"], c["h1map"], c["S"], Bh, Gh, faces)
        b = area_normal_reference(dim, c["NE"], c["N"], c["D"], c["h1map"], c["S"], Bq, Gq, faces)
        assert b.dtype == np.longdouble
        err = np.sqrt(((a - b).astype(np.float64) ** 2).sum(0))
        r = np.max(err / normal_bound(c, R1, faces))
        print(f"{zones_id} Q{order[0]}Q{order[1]} R1={R1}: reference error / bound {r:.4f}")
        assert r <= 0.25


def test_area_normal_reference_closes_every_zone():
    """On x = A xi + b the area vector is constant on a face, the sgn-signed a-th row of adj(A / n), and the vectors of a zone's
    faces sum to zero (its surface is closed): a wrong sign or (a, i) order in the reference would show."""
    for zones in ((3, 2), (3, 2, 2)):
        c = curved_state(zones, 2, 1)
        dim, NE, N = c["dim"], c["NE"], c["N"]
        rng = np.random.default_rng(5)
        A = rng.uniform(-1, 1, (dim, dim)) + 2 * np.eye(dim)
        S = c["S"].copy()
        # an affine map of the undisplaced nodes
        from oracle.fem import Problem
        p = Problem(breaks=[np.linspace(0.0, 1.0, n + 1) for n in zones], order_v=2, order_e=1, problem=1)
        X = p.initial_state()[0][:p.H1V].reshape(dim, N)
        S[:dim * N] = (A @ X).reshape(-1)
        Bh, Gh, _ = lattice_tables3(2, 1, 2)
        faces = all_faces(dim, NE)
        Nf = area_normal_reference(dim, NE, N, c["D"], c["h1map"], S, Bh, Gh, faces).reshape(dim, NE, 2 * dim, -1)
        total = Nf.mean(-1).sum(2)          # per zone: the sum over its faces of the mean area vector
        assert np.abs(total).max() <= 1e-13 * np.abs(Nf).max()
        # and on side 1 of axis a it is the a-th row of adj(A / n): outward where det > 0
        J = A / np.array(zones)[None, :]
        adj = np.linalg.det(J) * np.linalg.inv(J)
        for a in range(dim):
            assert np.abs(Nf[:, :, 2 * a + 1, :] - adj[a][:, None, None]).max() <= 1e-13
            assert np.abs(Nf[:, :, 2 * a, :] + adj[a][:, None, None]).max() <= 1e-13


# ---- the writer -----------------------------------------------------------------------------------------------------
def unit_box_faces(dim, R1):
    """One unit zone, all its faces on R1 points per direction: x on the lattice, the outward unit normals as area vectors"""
    faces = all_faces(dim, 1)
    NPF = R1 ** (dim - 1)
    x = np.zeros((dim, len(faces) * NPF))
    an = np.zeros_like(x)
    p = np.arange(NPF)
    for k, (_, f) in enumerate(faces):
        a, s = f >> 1, f & 1
        other = [b for b in range(dim) if b != a]
        sl = slice(k * NPF, (k + 1) * NPF)
        x[a, sl] = s
        x[other[0], sl] = (p % R1) / (R1 - 1)
        if dim == 3:
            x[other[1], sl] = (p // R1) / (R1 - 1)
        an[a, sl] = 2 * s - 1
    return faces, x, an


@pytest.mark.parametrize("dim", [2, 3])
def test_face_writer_read_back(dim, tmp_path):
    from laghos_amd import host_lib
    R1 = 3
    faces, x, an = unit_box_faces(dim, R1)
    nf, NPF, R = len(faces), R1 ** (dim - 1), R1 - 1
    NPt = nf * NPF
    rng = np.random.default_rng(11)
    v, e, rho, p = rng.uniform(-1, 1, (dim, NPt)), rng.uniform(-1, 1, NPt), rng.uniform(1, 2, NPt), rng.uniform(0, 1, NPt)
    extra = [("vorticity", 3, rng.uniform(-1, 1, (NPt, 3))), ("detJ", 1, rng.uniform(0, 1, NPt))]
    faces[:, 0] = 7   # (the zone id is the caller's: the writer passes it on)
    path = host_lib.host_write_vtu_faces(tmp_path / "s", dim, faces, R1, x, v, e, rho, p, extra, an, 12, 0.25)
    assert path.endswith("cycle_000012.vtu")
    f = read_face_vtu(path, dim)
    A = f["arrays"]
    assert f["npoints"] == NPt and f["ncells"] == nf * R ** (dim - 1)
    assert A["TIME"][0] == 0.25 and A["CYCLE"][0] == 12
    pad = lambda a: np.concatenate([a.T, np.zeros((NPt, 3 - dim))], 1)
    # the bits of every block
    assert np.array_equal(A["Points"], pad(x)) and np.array_equal(A["velocity"], pad(v)) and np.array_equal(A["area_normal"], pad(an))
    for name, want in (("density", rho), ("specific_internal_energy", e), ("pressure", p), ("vorticity", extra[0][2]), ("detJ", extra[1][2])):
        assert np.array_equal(A[name], want), name
        assert f["types"][name] == "Float64"
    assert [n for n, s in f["section"].items() if s == "PointData"] == ["density", "velocity", "specific_internal_energy", "pressure", "vorticity",
                                                                        "detJ", "area_normal"]
    cells_per_face = R ** (dim - 1)
    assert np.array_equal(f["cell_faces"], np.repeat(faces, cells_per_face, 0)) and np.all(A["rank"] == 0)
    # every cell lies on its own face's points and covers it: each point of a face is a corner of some cell of that face
    owner = f["conn"] // NPF
    assert np.array_equal(owner, np.repeat(np.arange(nf), cells_per_face)[:, None] * np.ones_like(owner))
    assert np.array_equal(np.unique(f["conn"]), np.arange(NPt))
    # outward-consistent corners: the cell's normal is a positive multiple of the outward normal, its size the cell's area
    n_out = np.repeat(np.array([[(2 * (fc & 1) - 1) * (b == fc >> 1) for b in range(3)] for fc in faces[:, 1]], float), cells_per_face, 0)
    assert np.allclose(f["cell_normals"], n_out / R ** (dim - 1), rtol=0, atol=1e-15)
    # the piece of a rank among several, and the .pvtu that names the pieces
    p1 = host_lib.host_write_vtu_faces(tmp_path / "m", dim, faces, R1, x, v, e, rho, p, extra, an, 3, 0.5, rank=1, nranks=2)
    assert p1.endswith("cycle_000003.1.vtu") and np.all(read_face_vtu(p1, dim)["arrays"]["rank"] == 1)
    txt = open(host_lib.host_write_pvtu_faces(tmp_path / "m", 3, 0.5, 2, [(n, c) for n, c, _ in extra])).read()
    ppd = re.search(r"<PPointData.*?</PPointData>", txt, flags=re.S).group(0)
    assert re.findall(r'Name="([^"]+)" NumberOfComponents="(\d+)"', ppd) == [("density", "1"), ("velocity", "3"), ("specific_internal_energy", "1"),
                                                                             ("pressure", "1"), ("vorticity", "3"), ("detJ", "1"), ("area_normal", "3")]
    pcd = re.search(r"<PCellData.*?</PCellData>", txt, flags=re.S).group(0)
    assert re.findall(r'Name="([^"]+)"', pcd) == ["zone", "face", "rank"]
    assert re.findall(r'<Piece Source="([^"]+)"/>', txt) == ["cycle_000003.0.vtu", "cycle_000003.1.vtu"]


@pytest.mark.parametrize("dim", [2, 3])
def test_face_writer_empty_piece(dim, tmp_path):
    """a rank without faces writes a piece with no points and no cells that still names every array"""
    from laghos_amd import host_lib
    z = np.zeros(0)
    path = host_lib.host_write_vtu_faces(tmp_path, dim, np.zeros((0, 2), np.int32), 4, z, z, z, z, z, [("div_v", 1, z)], z, 5, 1.5, rank=1, nranks=2)
    f = read_face_vtu(path, dim)
    assert f["npoints"] == 0 and f["ncells"] == 0
    for name, a in f["arrays"].items():
        assert a.size == (1 if name in ("TIME", "CYCLE") else 0), name
    assert "div_v" in f["arrays"] and f["arrays"]["TIME"][0] == 1.5


def test_face_writer_refuses_bad_input(tmp_path):
    from laghos_amd import host_lib
    faces, x, an = unit_box_faces(3, 2)
    NPt = len(faces) * 4
    z = np.zeros(NPt)
    bad = faces.copy()
    bad[2, 1] = 6
    with pytest.raises(RuntimeError):
        host_lib.host_write_vtu_faces(tmp_path, 3, bad, 2, x, x, z, z, z, [], an, 0, 0.0)
    with pytest.raises(RuntimeError):   # 1D has no face dumps
        host_lib.host_write_vtu_faces(tmp_path, 1, np.zeros((0, 2), np.int32), 2, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), [],
                                      np.zeros(0), 0, 0.0)
    assert not glob.glob(str(tmp_path / "*"))


# ---- the driver's refusals ------------------------------------------------------------------------------------------
BAD = {
    "axis": (["-pv-slice", "w", "1"], "cube01_hex", "-pv-slice", "x, y or z"),
    "K-negative": (["-pv-slice", "z", "-1"], "cube01_hex", "-pv-slice", "-1"),
    "K-word": (["-pv-slice", "z", "top"], "cube01_hex", "-pv-slice", "top"),
    "K-above": (["-pv-slice", "z", "5"], "cube01_hex", "-pv-slice z 5", "0..4"),
    "z-in-2D": (["-pv-slice", "z", "1"], "square01_quad", "-pv-slice z 1", "2 dimensions"),
    "ninth": (sum([["-pv-slice", "x", str(k)] for k in range(5)] + [["-pv-slice", "y", str(k)] for k in range(4)], []), "cube01_hex", "-pv-slice y 3",
              "ninth"),
    "twice": (["-pv-slice", "y", "2", "-pv-surface", "-pv-slice", "y", "2"], "cube01_hex", "-pv-slice y 2", "twice"),
    "no-K": (["-pv-slice", "y"], "cube01_hex", "-pv-slice", "missing value"),
    "surface-1D": (["-pv-surface"], "segment01", "-pv-surface", "1D"),
    "slice-1D": (["-pv-slice", "x", "1"], "segment01", "-pv-slice", "1D"),
    "fields-alone": (["-pv-fields", "all"], "cube01_hex", "-pv-fields", "-paraview"),
    "vr": (["-pv-surface", "-vr", "9"], "cube01_hex", "-vr", "between 1 and 8"),
}


def run_refused(case, tmp_path):
    extra, mesh_name, *words = BAD[case]
    base = str(tmp_path / "run")
    args = ["-p", "2" if mesh_name == "segment01" else "1", "-m", f"data/{mesh_name}.mesh", "-rs", "1", "-ms", "1", "-k", base, "-q"] + extra
    p = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert p.returncode != 0 and all(w in p.stderr for w in words), p.stderr
    assert not glob.glob(str(tmp_path / "*"))                         # nothing was set up, nothing written


@pytest.mark.parametrize("case", list(BAD))
def test_driver_refuses_bad_face_options_before_the_gpu(case, tmp_path):
    """(the refusal comes before the first call of the GPU runtime: the executable gives it on a machine without a GPU too)"""
    run_refused(case, tmp_path)
