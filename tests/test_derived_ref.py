"""The derived lattice fields without a GPU: the numpy reference (tests/derived_ref.py) against closed-form fields and
against itself in long double, the host library's derivative table against the formula, the VTK writer's entry points
with extra arrays read back with tests/vtu_reader.py, and the driver's refusals of bad `-pv-fields` values (all decided
while the command line is read or right after the mesh is known: before anything touches the GPU).

Closed form: the space is isoparametric, so a velocity v = A x + b set at the nodes of a curved mesh has dv/dx = A at
every point up to rounding, whatever the mesh: this pins the signs and the (i, j) order of every output independently
of the einsums of the reference."""
import glob
import os
import subprocess

import numpy as np
import pytest

from derived_ref import TOL, affine_velocity, curved_state, derived_reference, lagrange_grad_table, lattice_tables3
from lattice_ref import gll_nodes
from vtu_reader import read_vtu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

ZONES = {"1D-1": (1,), "1D-3": (3,), "1D-257": (257,), "2D-3x2": (3, 2), "3D-3x2x2": (3, 2, 2), "3D-5x5x3": (5, 5, 3)}
ORDERS = [(1, 0), (2, 1), (3, 2)]
CASES = [(z, o) for z in ZONES for o in ORDERS] + [("2D-3x2", (4, 3))]   # those of tests/test_gpu_derived.py
R1S = [2, 3, 6, 9]


def reference(c, R1, S=None, dtype=np.float64):
    T = lattice_tables3(c["ok"], c["ot"], R1 - 1, dtype)
    return derived_reference(c["dim"], c["NE"], c["N"], c["D"], c["L"], c["h1map"], c["S"] if S is None else S, c["gamma"], *T)


def affine_fields(dim):
    """name -> (A, expected vorticity (scalar in 2D, 3-vector in 3D, None in 1D), expected divergence)"""
    rng = np.random.default_rng(40 + dim)
    out = {}
    if dim == 1:
        out["expansion"] = (np.array([[0.7]]), None, 0.7)
        out["random"] = (np.array([[-1.3]]), None, -1.3)
        return out
    if dim == 2:
        Om = 0.9
        out["rotation"] = (np.array([[0.0, -Om], [Om, 0.0]]), 2 * Om, 0.0)            # v = Omega z x r
    else:
        w = np.array([0.3, -0.8, 0.5])                                                 # v = w x r: curl v = 2 w
        out["rotation"] = (np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]), 2 * w, 0.0)
    out["expansion"] = (0.7 * np.eye(dim), 0.0 if dim == 2 else np.zeros(3), dim * 0.7)
    A = rng.uniform(-1, 1, (dim, dim))
    curl = A[1, 0] - A[0, 1] if dim == 2 else np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]])
    out["random"] = (A, curl, np.trace(A))
    return out


@pytest.mark.parametrize("zones_id,order,R1", [("1D-3", (2, 1), 3), ("2D-3x2", (3, 2), 6), ("2D-3x2", (4, 3), 3), ("3D-3x2x2", (2, 1), 3),
                                               ("3D-3x2x2", (3, 2), 6)])
def test_affine_velocity_has_its_matrix_as_gradient(zones_id, order, R1):
    c = curved_state(ZONES[zones_id], *order)
    dim = c["dim"]
    for name, (A, curl, div) in affine_fields(dim).items():
        S = affine_velocity(c["S"], dim, c["N"], A, np.arange(1.0, dim + 1))
        ref = reference(c, R1, S)
        L = ref["grad_v"].T.reshape(-1, dim, dim)                     # entry (i, j) at row i*dim + j
        err = np.sqrt(((L - A) ** 2).sum((1, 2)))
        print(f"{zones_id} Q{order[0]}Q{order[1]} R1={R1} {name}: max |L - A|_F / bound {np.max(err / (TOL * ref['bound_L'])):.3f}")
        assert np.all(err <= TOL * ref["bound_L"]), name
        assert np.all(np.abs(ref["div_v"] - div) <= dim * TOL * ref["bound_L"]), name
        if dim > 1:
            want = np.broadcast_to(np.reshape(curl, (-1, 1)), (np.size(curl), L.shape[0])).reshape(ref["vorticity"].shape)
            assert np.all(np.abs(ref["vorticity"] - want) <= 2 * TOL * ref["bound_L"]), name
        assert "vorticity" in ref or dim == 1
    # the curved mesh is curved: J is not constant in a zone
    assert np.ptp(ref["detj"].reshape(c["NE"], -1), axis=1).max() > 1e-3 * np.abs(ref["detj"]).max() or order[0] == 1


@pytest.mark.parametrize("zones_id,order", CASES, ids=[f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES])
def test_reference_in_long_double_against_itself(zones_id, order):
    """The float64 reference carries its own rounding: against the same formulas in long double it must stay within a quarter
    of the bound the GPU is held to, on every case of the GPU test."""
    c = curved_state(ZONES[zones_id], *order)
    for R1 in R1S:
        a, b = reference(c, R1), reference(c, R1, dtype=np.longdouble)
        assert b["grad_v"].dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
        eL = np.sqrt(((a["grad_v"] - b["grad_v"]).astype(np.float64) ** 2).sum(0))
        eD = np.abs(a["detj"] - b["detj"]).astype(np.float64)
        rL, rD = np.max(eL / (TOL * a["bound_L"])), np.max(eD / (TOL * a["bound_det"]))
        print(f"{zones_id} Q{order[0]}Q{order[1]} R1={R1}: reference error / bound: L {rL:.4f}, detJ {rD:.4f}")
        assert rL <= 0.25 and rD <= 0.25


@pytest.mark.parametrize("order_v", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_host_lattice_grad_table(order_v, R):
    from laghos_amd import host_lib
    G = host_lib.host_lattice_grad_table(order_v, R)
    want = lagrange_grad_table(gll_nodes(order_v + 1), np.arange(R + 1) / R)
    assert G.shape == (R + 1, order_v + 1)
    # entries up to O(order^2), sums of order_v products of order_v - 1 factors each; the two sides take other nodes (Newton
    # against numpy's roots) that agree to a few ulp, and the derivative's condition in the nodes is O(order^2) as well
    assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(G.sum(1)).max() <= 1e-12 * np.abs(want).max()      # the basis sums to one: its derivatives to zero
    # and it differentiates: d/dx of x^k, k <= order_v, interpolated at the nodes
    x, pts = gll_nodes(order_v + 1), np.arange(R + 1) / R
    for k in range(1, order_v + 1):
        assert np.abs(G @ x ** k - k * pts ** (k - 1)).max() <= 1e-12 * k * order_v ** 2


def sampled(dim, NE, R1, seed=0):
    rng = np.random.default_rng(seed)
    NP = NE * R1 ** dim
    return [rng.uniform(-1, 1, n) for n in (dim * NP, dim * NP, NP, NP, NP)], NP


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_writer_with_extra_arrays(dim, tmp_path):
    from laghos_amd import host_lib
    NE, R1 = 3, 3
    base, NP = sampled(dim, NE, R1)
    rng = np.random.default_rng(7)
    extra = [("div_v", 1, rng.uniform(-1, 1, NP)), ("vorticity", 3, rng.uniform(-1, 1, (NP, 3))),
             ("velocity_gradient", 9, rng.uniform(-1, 1, (NP, 9))), ("detJ", 1, rng.uniform(-1, 1, NP)), ("sound_speed", 1, rng.uniform(0, 1, NP))]
    for sel in (extra, extra[3:], extra[1:2], [extra[2], extra[0]]):      # (the writer keeps the order it is given)
        d = tmp_path / f"d{len(sel)}{sel[0][0]}"
        path = host_lib.host_write_vtu_fields(d, dim, NE, R1, *base, sel, 12, 0.25)
        f = read_vtu(path)
        names = [n for n, s in f["section"].items() if s == "PointData"]
        assert names == ["density", "velocity", "specific_internal_energy", "pressure"] + [n for n, _, _ in sel]
        for n, c, a in sel:
            assert f["ncomp"][n] == c and f["types"][n] == "Float64"
            assert np.array_equal(f["arrays"][n], a), n               # the bits
        # the standing arrays and the rest of the file are those of the plain writer
        plain = read_vtu(host_lib.host_write_vtu(tmp_path / "plain", dim, NE, R1, *base, 12, 0.25))
        for n, a in plain["arrays"].items():
            assert np.array_equal(f["arrays"][n], a), n
    # no extras: the bytes of the plain writer
    p0 = host_lib.host_write_vtu_fields(tmp_path / "none", dim, NE, R1, *base, [], 12, 0.25)
    assert open(p0, "rb").read() == open(tmp_path / "plain" / "cycle_000012.vtu", "rb").read()


def test_pvtu_with_extra_arrays(tmp_path):
    import re
    from laghos_amd import host_lib
    extra = [("div_v", 1), ("vorticity", 3), ("velocity_gradient", 9)]
    txt = open(host_lib.host_write_pvtu_fields(tmp_path / "a", 4, 0.5, 2, extra)).read()
    ppd = re.search(r"<PPointData.*?</PPointData>", txt, flags=re.S).group(0)
    got = re.findall(r'<PDataArray type="Float64" Name="([^"]+)" NumberOfComponents="(\d+)"/>', ppd)
    assert got == [("density", "1"), ("velocity", "3"), ("specific_internal_energy", "1"), ("pressure", "1")] + [(n, str(c)) for n, c in extra]
    assert re.findall(r'<Piece Source="([^"]+)"/>', txt) == ["cycle_000004.0.vtu", "cycle_000004.1.vtu"]
    plain = open(host_lib.host_write_pvtu(tmp_path / "b", 4, 0.5, 2)).read()
    assert open(host_lib.host_write_pvtu_fields(tmp_path / "c", 4, 0.5, 2, [])).read() == plain


def test_writer_refuses_a_bad_extra_array(tmp_path):
    from laghos_amd import host_lib
    base, NP = sampled(2, 2, 2)
    L = host_lib.load()
    import ctypes
    names = (ctypes.c_char_p * 1)(b"div_v")
    comps = (ctypes.c_int * 1)(0)                                     # no components
    a = np.zeros(NP)
    data = (ctypes.c_void_p * 1)(a.ctypes.data)
    rc = L.laghos_host_write_vtu_fields(str(tmp_path).encode(), 2, 2, 2, *[b.ctypes.data for b in base], 1, names, comps, data, 0, 0.0, 0, 1)
    assert rc != 0 and not glob.glob(str(tmp_path / "*"))
    comps[0], data[0] = 1, None                                       # no data
    rc = L.laghos_host_write_vtu_fields(str(tmp_path).encode(), 2, 2, 2, *[b.ctypes.data for b in base], 1, names, comps, data, 0, 0.0, 0, 1)
    assert rc != 0 and not glob.glob(str(tmp_path / "*"))


BAD = {
    "unknown": (["-paraview", "-pv-fields", "div_v,enstrophy"], "square01_quad", "enstrophy"),
    "empty": (["-paraview", "-pv-fields", ""], "square01_quad", "empty"),
    "commas": (["-paraview", "-pv-fields", ",,"], "square01_quad", "empty"),
    "no-paraview": (["-pv-fields", "all"], "square01_quad", "-paraview"),
    "1D-vorticity": (["-paraview", "-pv-fields", "detj,vorticity"], "segment01", "1D"),
    "1D-all-and-vorticity": (["-paraview", "-pv-fields", "all,vorticity"], "segment01", "1D"),
    "no-value": (["-paraview", "-pv-fields"], "square01_quad", "missing value"),
}


@pytest.mark.parametrize("case", list(BAD))
def test_driver_refuses_bad_pv_fields_before_the_gpu(case, tmp_path):
    """(the refusal comes before the first call of the GPU runtime: the executable gives it on a machine without a GPU too)"""
    extra, mesh, word = BAD[case]
    base = str(tmp_path / "run")
    args = ["-p", "2" if mesh == "segment01" else "1", "-m", f"data/{mesh}.mesh", "-rs", "1", "-ms", "1", "-k", base, "-q"] + extra
    p = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert p.returncode != 0 and "-pv-fields" in p.stderr and word in p.stderr, p.stderr
    assert not glob.glob(str(tmp_path / "*"))                         # nothing was set up, nothing written
