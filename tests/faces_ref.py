"""numpy restatement of the face sampling (lgh_sample_faces) for the tests: where a face's lattice points sit in the volume
lattice, the boundary faces of a mesh by brute force over node sets, the outward area vector from the Jacobian of
tests/derived_ref.py in the dtype it is given, and a reader of the `-pv-surface` / `-pv-slice` files on top of
tests/vtu_reader.py.  Shares no code with the library."""
import re
from collections import Counter

import numpy as np

from derived_ref import _jacobian
from vtu_reader import read_vtu


def face_axes(dim, f):
    """(normal axis a, side s, the other axes ascending)"""
    a, s = f >> 1, f & 1
    return a, s, [b for b in range(dim) if b != a]


def face_volume_index(dim, R1, faces):
    """For faces (nfaces, 2) = (zone, local face): the index into a volume lattice array (zone * R1^dim + r_x + R1 (r_y + R1 r_z))
    of every face lattice point pt = k * R1^(dim-1) + r_b + R1 r_c (b < c the axes other than the normal one)"""
    faces = np.asarray(faces).reshape(-1, 2)
    NPF, NPZ = R1 ** (dim - 1), R1 ** dim
    p = np.arange(NPF)
    out = np.empty((faces.shape[0], NPF), np.int64)
    for k, (e, f) in enumerate(faces):
        a, s, other = face_axes(dim, int(f))
        r = [None] * dim
        r[a] = np.full(NPF, s * (R1 - 1))
        r[other[0]] = p % R1
        if dim == 3:
            r[other[1]] = p // R1
        idx = r[dim - 1]
        for b in range(dim - 2, -1, -1):
            idx = idx * R1 + r[b]
        out[k] = int(e) * NPZ + idx
    return out.reshape(-1)


def face_nodes(dim, D, f):
    """local dof indices dx + D (dy + D dz) of the D^(dim-1) nodes of local face f"""
    a, s, _ = face_axes(dim, f)
    d = np.arange(D ** dim)
    return d[(d // D ** a) % D == s * (D - 1)]


def brute_boundary_faces(dim, NE, D, h1map):
    """(nfaces, 2) in ascending (zone, face): the faces whose node set no other face of any zone has"""
    hm = np.asarray(h1map).reshape(NE, D ** dim)
    sets = {(e, f): frozenset(hm[e, face_nodes(dim, D, f)].tolist()) for e in range(NE) for f in range(2 * dim)}
    count = Counter(sets.values())
    return np.array([k for k in sorted(sets) if count[sets[k]] == 1], np.int32).reshape(-1, 2)


def adjugate(J):
    """adj of [pt, dim, dim] with J adj(J) = det J I, from cofactors (no division), in the dtype of J"""
    n = J.shape[-1]
    A = np.empty_like(J)
    if n == 2:
        A[:, 0, 0], A[:, 0, 1], A[:, 1, 0], A[:, 1, 1] = J[:, 1, 1], -J[:, 0, 1], -J[:, 1, 0], J[:, 0, 0]
        return A
    for i in range(3):
        for j in range(3):
            a, b = (j + 1) % 3, (j + 2) % 3
            c, d = (i + 1) % 3, (i + 2) % 3
            A[:, i, j] = J[:, a, c] * J[:, b, d] - J[:, a, d] * J[:, b, c]
    return A


def area_normal_reference(dim, NE, N, D, h1map, S, Bh, Gh, faces):
    """(dim, NPt): N_i = sgn adj(J)_{a i} at the face lattice points, J = dx/dxi from dense einsums; works in the dtype of Bh"""
    dt = Bh.dtype
    R1 = Bh.shape[0]
    faces = np.asarray(faces).reshape(-1, 2)
    hm = np.asarray(h1map).reshape(NE, *([D] * dim))
    X = np.asarray(S).astype(dt)[:dim * N].reshape(dim, N)
    A = adjugate(_jacobian(X, hm, Bh, Gh, dim)[face_volume_index(dim, R1, faces)])
    NPF = R1 ** (dim - 1)
    a = np.repeat(faces[:, 1] >> 1, NPF)
    sgn = np.repeat(np.where(faces[:, 1] & 1, 1, -1), NPF).astype(dt)
    return (sgn[:, None] * A[np.arange(A.shape[0]), a, :]).T.copy()


def read_face_vtu(path, dim):
    """read_vtu of a face piece, checked for what every such file holds; adds conn (ncells, corners), cell_faces (ncells, 2) =
    (zone, face) from the cell data and cell_normals (ncells, 3): the normal of every cell by the right-hand rule over its
    corners (3D), the tangent turned clockwise (2D)"""
    f = read_vtu(path)
    A = f["arrays"]
    pd = [n for n, s in f["section"].items() if s == "PointData"]
    assert pd[:4] == ["density", "velocity", "specific_internal_energy", "pressure"] and pd[-1] == "area_normal", pd
    assert [n for n, s in f["section"].items() if s == "CellData"] == ["zone", "face", "rank"]
    assert f["ncomp"]["area_normal"] == 3 and f["ncomp"]["Points"] == 3
    nv = 4 if dim == 3 else 2
    assert np.all(A["types"] == (9 if dim == 3 else 3))
    assert np.array_equal(A["offsets"], nv * np.arange(1, f["ncells"] + 1))
    conn = A["connectivity"].reshape(-1, nv)
    assert conn.size == 0 or (conn.min() >= 0 and conn.max() < f["npoints"])
    zf = np.stack([A["zone"], A["face"]], 1)
    P = A["Points"].reshape(-1, 3)
    f["conn"] = conn
    if f["ncells"]:
        c = P[conn]
        if dim == 3:
            f["cell_normals"] = np.cross(c[:, 1] - c[:, 0], c[:, 3] - c[:, 0])
        else:
            t = c[:, 1] - c[:, 0]
            f["cell_normals"] = np.stack([t[:, 1], -t[:, 0], np.zeros(len(t))], 1)
    else:
        f["cell_normals"] = np.zeros((0, 3))
    f["cell_faces"] = zf
    return f


def read_pvd(path):
    """[(timestep string, file)] of a collection"""
    return re.findall(r'<DataSet timestep="([^"]+)" group="" part="0" file="([^"]+)"/>', open(path).read())
