"""lgh_sample_faces (Context.sample_faces): the fields and derived fields of a state on the lattices of zone faces.

Definition under test: every output but the area vector has THE BITS lgh_sample_fields / lgh_sample_derived give at the same
lattice point of the volume lattice (tests/faces_ref.py face_volume_index says which point that is, from the definition in
include/laghos_hip.h).  The volume kernels are run once per (case, R1) on the curved-mesh random state of
tests/test_gpu_sample.py (its Case, built here on this file's zone grids) and shared, unchanged, by the tests.

Shapes: one zone and a few, unequal counts per axis, 75 zones; orders 1..3 and 4 on the small grids; lattices below and above
the dof grid and the workgroup (R1 = 2, 3, 6, 9).  Lists: all faces, the boundary, one face, the faces of one zone, a shuffled
list with repeats, and FPB - 1, FPB, FPB + 1 faces (FPB from lgh_sample_faces_fpb: the edges of a workgroup).  Outputs are
NaN-filled before a call and carry a guard word behind the last entry.

The area vector N_i = sgn adj(J)_{a i} is held to the bound tests/test_gpu_derived.py applies to det J - TOL |A_J|_F |J^-1|_F
|det J| per point, |N - N_ref|_2 on the left: the entries of adj(J) are sub-determinants of the same J, and |A_J|_F |adj J|_F
is that product - against tests/faces_ref.py in long double (tests/test_host_faces.py holds the float64 form of that reference
to a quarter of the bound on these cases), and on an affine mesh against the closed form.

Not covered: the two LGH_ERR_UNSUPPORTED refusals (tables above 81 entries, a face above 64 KB of LDS) need D1D = 10, for
which no context can be created."""
import ctypes

import numpy as np
import pytest

from derived_ref import TOL, derived_reference, lattice_tables3
from faces_ref import area_normal_reference, brute_boundary_faces, face_volume_index
from test_gpu_sample import Case

pytestmark = pytest.mark.gpu

ZONES = {"2D-1x1": (1, 1), "2D-3x2": (3, 2), "3D-1x1x1": (1, 1, 1), "3D-3x2x2": (3, 2, 2), "3D-5x5x3": (5, 5, 3)}
SMALL = ("2D-1x1", "2D-3x2", "3D-1x1x1")
CASES = [(z, o) for z in ZONES for o in [(1, 0), (2, 1), (3, 2)]] + [(z, (4, 3)) for z in SMALL]
R1S = [2, 3, 6, 9]
NAMES = ("x", "v", "e", "rho", "p", "detj", "grad_v", "div_v", "vorticity", "sound_speed", "area_normal")
GUARD = -1234.5


def ncomp(k, dim):
    return {"x": dim, "v": dim, "grad_v": dim * dim, "vorticity": 3 if dim == 3 else 1, "area_normal": dim}.get(k, 1)


class FaceCase(Case):
    def __init__(self, zones, ok, ot, renumber=None):
        super().__init__(zones, ok, ot, renumber)
        self._vol = {}

    def tables3(self, R1):
        return lattice_tables3(self.ok, self.ot, R1 - 1)

    def volume(self, R1):
        """the outputs of the two volume kernels, name -> (components, NP); computed once, shared, never written"""
        if R1 not in self._vol:
            dim, NP = self.dim, self.NE * R1 ** self.dim
            Bh, Gh, Bl = self.tables3(R1)
            out = {k: self.ctx.to_dev(np.full(ncomp(k, dim) * NP, np.nan)) for k in NAMES if k != "area_normal"}
            self.ctx.sample_fields(self.Sd, self.rhod, Bh, Bl, **{k: out[k] for k in ("x", "v", "e", "rho", "p")})
            self.ctx.sample_derived(self.Sd, Bh, Gh, Bl, detj=out["detj"], grad_v=out["grad_v"], div_v=out["div_v"], vorticity=out["vorticity"],
                                    sound_speed=out["sound_speed"])
            self.ctx.sync()
            vol = {k: t.cpu().numpy().reshape(ncomp(k, dim), NP) for k, t in out.items()}
            for a in vol.values():
                assert np.all(np.isfinite(a))
                a.setflags(write=False)
            self._vol[R1] = vol
        return self._vol[R1]

    def faces_run(self, R1, faces, want=NAMES, Sd=None, rho_l2=True):
        """name -> (components, NPt) of the outputs asked for (the others are NULL); NaN-filled, guard word checked"""
        dim = self.dim
        faces = np.asarray(faces, np.int32).reshape(-1, 2)
        NPt = len(faces) * R1 ** (dim - 1)
        Bh, Gh, Bl = self.tables3(R1)
        out = {k: self.ctx.to_dev(np.concatenate([np.full(ncomp(k, dim) * NPt, np.nan), [GUARD]])) for k in want}
        self.ctx.sample_faces(self.Sd if Sd is None else Sd, self.rhod if rho_l2 else None, Bh, Gh, Bl, faces, **out)
        self.ctx.sync()
        res = {}
        for k, t in out.items():
            a = t.cpu().numpy()
            assert a[-1] == GUARD, (k, "the word behind the array was written")
            res[k] = a[:-1].reshape(ncomp(k, dim), NPt)
        return res


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(zones_id, order, renumber=None):
        key = (zones_id, order, renumber)
        if key not in made:
            made[key] = FaceCase(ZONES[zones_id], order[0], order[1], renumber)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def all_faces(c):
    return np.stack([np.repeat(np.arange(c.NE), 2 * c.dim), np.tile(np.arange(2 * c.dim), c.NE)], 1).astype(np.int32)


def face_lists(c, R1):
    """name -> (nfaces, 2): the lists every (case, R1) is run on"""
    rng = np.random.default_rng(7 * c.NE + R1)
    every = all_faces(c)
    fpb = c.ctx.faces_per_block(R1)
    cyc = lambda n: every[(np.arange(n) * 5 + 1) % len(every)]      # n faces, zones not consecutive, repeats once n > len
    z = int(rng.integers(c.NE))
    lists = {"all": every, "boundary": c.ctx.boundary_faces(), "one": every[[int(rng.integers(len(every)))]],
             "zone": every[every[:, 0] == z], "shuffled": every[rng.integers(len(every), size=len(every) + 3)]}
    for n in (fpb - 1, fpb, fpb + 1):
        if n > 0:
            lists[f"fpb{n - fpb:+d}"] = cyc(n)
    return lists, fpb


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_bits(c, R1, faces, got, what):
    vol, idx = c.volume(R1), face_volume_index(c.dim, R1, faces)
    for k, a in got.items():
        assert np.all(np.isfinite(a)), (what, k, "an entry was not written")
        if k != "area_normal":
            bad = np.argwhere(bits(a) != bits(vol[k][:, idx]))
            assert bad.size == 0, (what, k, f"{len(bad)} entries differ from the volume lattice, first at {bad[0]}")


def expected_fpb(dim, D, L, R1):
    """the documented rule (include/laghos_hip.h)"""
    h1 = D ** dim + 2 * R1 * D ** (dim - 1) + (3 * R1 * R1 * D if dim == 3 else 0)
    l2 = L ** dim + R1 * L ** (dim - 1) + (R1 * R1 * L if dim == 3 else 0)
    tab, face = 8 * (R1 + 2) * (2 * D + L), 8 * (1 + max(h1, l2))
    return max(1, min(256 // R1 ** (dim - 1), (48 * 1024 - tab) // face))


@pytest.mark.parametrize("R1", R1S)
@pytest.mark.parametrize("zones_id,order", CASES, ids=[f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES])
def test_faces_have_the_bits_of_the_volume_lattice(cases, zones_id, order, R1):
    c = cases(zones_id, order)
    lists, fpb = face_lists(c, R1)
    assert fpb == expected_fpb(c.dim, c.D, c.L, R1)
    assert np.array_equal(lists["boundary"], brute_boundary_faces(c.dim, c.NE, c.D, c.h1map))
    assert len(lists) >= 7
    S_before, gen = c.S.copy(), c.ctx.quadrature_generation()
    for name, faces in lists.items():
        what = f"{zones_id} Q{order[0]}Q{order[1]} R1={R1} {name} ({len(faces)} faces, FPB {fpb})"
        check_bits(c, R1, faces, c.faces_run(R1, faces), what)
    # read-only inputs
    assert np.array_equal(c.Sd.cpu().numpy(), S_before) and c.ctx.quadrature_generation() == gen
    if c.NE >= 12:   # the clamps of pressure and sound speed are in play on the faces too
        got = c.faces_run(R1, lists["all"], want=("e", "p", "sound_speed"))
        assert (got["e"] < 0).any() and (got["p"] == 0).any() and (got["sound_speed"] == 0).any() and (got["p"] > 0).any()


@pytest.mark.parametrize("zones_id,order,R1", [("2D-3x2", (4, 3), 6), ("3D-5x5x3", (3, 2), 3), ("3D-3x2x2", (3, 2), 9), ("3D-1x1x1", (1, 0), 2)])
def test_every_output_alone_gives_the_same_bits(cases, zones_id, order, R1):
    c = cases(zones_id, order)
    faces = face_lists(c, R1)[0]["shuffled"]
    full = c.faces_run(R1, faces)
    for k in NAMES:
        alone = c.faces_run(R1, faces, want=(k,), rho_l2=k in ("rho", "p"))   # (without density dofs where none are needed)
        assert np.array_equal(bits(alone[k]), bits(full[k])), k
    # the tables an output does not need may be NULL
    dim, NPt = c.dim, len(faces) * R1 ** (c.dim - 1)
    Bh, Gh, Bl = c.tables3(R1)
    e = c.ctx.to_dev(np.full(NPt, np.nan))
    c.ctx.sample_faces(c.Sd, None, None, None, Bl, faces, e=e)
    x = c.ctx.to_dev(np.full(dim * NPt, np.nan))
    c.ctx.sample_faces(c.Sd, None, Bh, None, None, faces, x=x)
    c.ctx.sync()
    assert np.array_equal(bits(e.cpu().numpy()), bits(full["e"][0])) and np.array_equal(bits(x.cpu().numpy().reshape(dim, NPt)), bits(full["x"]))


def test_two_calls_give_identical_bits(cases):
    for zones_id, order, R1 in (("3D-5x5x3", (3, 2), 6), ("2D-3x2", (3, 2), 9), ("3D-3x2x2", (2, 1), 2)):
        c = cases(zones_id, order)
        faces = face_lists(c, R1)[0]["all"]
        a, b = c.faces_run(R1, faces), c.faces_run(R1, faces)
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), (zones_id, k)
        # a shorter list after a longer one (the context's device copy is reused), then the longer one again
        short = c.faces_run(R1, faces[:3])
        for k in a:
            assert np.array_equal(bits(short[k]), bits(a[k][:, :3 * R1 ** (c.dim - 1)])), (zones_id, k)


@pytest.mark.parametrize("zones_id", ["3D-3x2x2", "2D-3x2"])
def test_renumbered_mesh(cases, zones_id):
    """another numbering of nodes and zones (Discretization::Renumber): faces name the caller's zone ids, the values are those of
    that mesh's own volume lattice, and the boundary found from the map is the boundary of the box"""
    c = cases(zones_id, (3, 2), "random")
    assert not np.array_equal(c.elem_perm, np.arange(c.NE)) and not np.array_equal(c.node_perm, np.arange(c.N))
    for R1 in (3, 6):
        lists, _ = face_lists(c, R1)
        for name, faces in lists.items():
            check_bits(c, R1, faces, c.faces_run(R1, faces), f"{zones_id} random R1={R1} {name}")
        zones = ZONES[zones_id]
        assert len(lists["boundary"]) == 2 * sum(c.NE // n for n in zones)


def affine_mesh_state(c, zones, A, b):
    """S of the case with x = A X0 + b at the nodes, X0 the undisplaced nodes of the unit box"""
    from oracle.fem import Problem
    p = Problem(breaks=[np.linspace(0.0, 1.0, n + 1) for n in zones], order_v=c.ok, order_e=c.ot, problem=1)
    X0 = p.initial_state()[0][:p.H1V].reshape(c.dim, c.N)
    S = c.S.copy()
    S[:c.dim * c.N] = (A @ X0 + b[:, None]).reshape(-1)
    return S


@pytest.mark.parametrize("zones_id,order,R1", [("2D-3x2", (3, 2), 3), ("3D-3x2x2", (2, 1), 3), ("3D-5x5x3", (3, 2), 6), ("3D-1x1x1", (1, 0), 2)])
def test_area_normal_on_an_affine_mesh(cases, zones_id, order, R1):
    """x = A xi + b: J = A / n in every zone, and N is the constant sgn times row a of adj(J) - signs and the (a, i) order,
    independently of the einsums of the reference"""
    c = cases(zones_id, order)
    dim, zones = c.dim, ZONES[zones_id]
    rng = np.random.default_rng(80 + dim)
    A, b = rng.uniform(-1, 1, (dim, dim)) + 2 * np.eye(dim), rng.uniform(-1, 1, dim)
    S = affine_mesh_state(c, zones, A, b)
    J = A / np.array(zones, float)[None, :]
    adj = np.linalg.det(J) * np.linalg.inv(J)
    assert np.linalg.det(J) > 0
    faces = all_faces(c)
    got = c.faces_run(R1, faces, want=("area_normal", "detj"), Sd=c.ctx.to_dev(S))
    NPF = R1 ** (dim - 1)
    a, sgn = np.repeat(faces[:, 1] >> 1, NPF), np.repeat(np.where(faces[:, 1] & 1, 1.0, -1.0), NPF)
    want = (sgn[:, None] * adj[a, :]).T
    T = c.tables3(R1)
    ref = derived_reference(dim, c.NE, c.N, c.D, c.L, c.h1map, S, c.gamma, *T)
    bound = TOL * ref["bound_det"][face_volume_index(dim, R1, faces)]
    err = np.sqrt(((got["area_normal"] - want) ** 2).sum(0))
    print(f"{zones_id} R1={R1}: max |N - sgn adj(J)_a| / bound {np.max(err / bound):.4f}")
    assert np.all(err <= bound)
    # outward: on side 1 of axis a, N . (column a of J) = det J > 0
    assert np.all((got["area_normal"] * (sgn[None, :] * J[:, a])).sum(0) > 0)


@pytest.mark.parametrize("R1", R1S)
@pytest.mark.parametrize("zones_id,order", CASES, ids=[f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES])
def test_area_normal_on_the_curved_mesh(cases, zones_id, order, R1):
    c = cases(zones_id, order)
    dim, faces = c.dim, all_faces(c)
    got = c.faces_run(R1, faces, want=("area_normal",))["area_normal"]
    Bq, Gq, _ = lattice_tables3(c.ok, c.ot, R1 - 1, np.longdouble)
    want = area_normal_reference(dim, c.NE, c.N, c.D, c.h1map, c.S, Bq, Gq, faces)
    assert want.dtype == np.longdouble
    ref = derived_reference(dim, c.NE, c.N, c.D, c.L, c.h1map, c.S, c.gamma, *c.tables3(R1))
    bound = TOL * ref["bound_det"][face_volume_index(dim, R1, faces)]
    err = np.sqrt(((got - want).astype(np.float64) ** 2).sum(0))
    print(f"{zones_id} Q{order[0]}Q{order[1]} R1={R1}: max |N - N_ref| / bound {np.max(err / bound):.4f}")
    assert np.all(err <= bound)
    assert np.abs(want).max() > 0


def test_refused_calls_set_the_error_and_run_no_kernel(cases):
    from laghos_amd import _lib
    from laghos_amd._lib import LghError
    c = cases("3D-3x2x2", (2, 1))
    L = _lib.load()
    R1, dim = 3, 3
    faces = all_faces(c)[:5]
    NPt = len(faces) * R1 ** 2
    Bh, Gh, Bl = c.tables3(R1)
    outs = lambda *names: {k: c.ctx.to_dev(np.full(ncomp(k, dim) * NPt, np.nan)) for k in names}

    def refused(match, tables=(Bh, Gh, Bl), fc=faces, with_rho=True, **out):
        with pytest.raises(LghError, match=match) as ei:
            c.ctx.sample_faces(c.Sd, c.rhod if with_rho else None, *tables, fc, **out)
        assert str(ei.value).split(": ", 1)[1] == L.lgh_last_error().decode()      # the last error is set
        c.ctx.sync()
        for k, t in out.items():
            assert np.all(np.isnan(t.cpu().numpy())), (match, k, "a kernel ran")

    for bad in (1, 10):
        refused(f"R1 = {bad}", tables=(np.ones((bad, c.D)), np.ones((bad, c.D)), np.ones((bad, c.L))), **outs("e", "detj"))
    refused("B_h1_lat", tables=(None, Gh, Bl), **outs("x"))
    refused("B_h1_lat", tables=(None, Gh, Bl), **outs("detj"))
    refused("G_h1_lat", tables=(Bh, None, Bl), **outs("x", "area_normal"))
    refused("G_h1_lat", tables=(Bh, None, Bl), **outs("div_v"))
    refused("B_l2_lat", tables=(Bh, Gh, None), **outs("sound_speed"))
    refused("rho_l2", with_rho=False, **outs("rho"))
    refused("rho_l2", with_rho=False, **outs("x", "p"))
    bad = faces.copy()
    bad[3, 0] = c.NE
    refused(f"zone {c.NE} ", fc=bad, **outs("x"))
    bad[3, 0] = -1
    refused("zone -1 ", fc=bad, **outs("x"))
    bad = faces.copy()
    bad[4, 1] = 6
    refused("local face 6 ", fc=bad, **outs("x"))
    bad[4, 1] = -2
    refused("local face -2 ", fc=bad, **outs("x"))
    # nfaces < 0: through the library itself
    out = outs("e")["e"]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    tab = lambda T: np.ascontiguousarray(T.T.reshape(-1)).ctypes.data_as(dp)
    nul = [None] * 11
    args = lambda n, o: [c.ctx.h, c.Sd.data_ptr(), c.rhod.data_ptr(), R1, tab(Bh), tab(Gh), tab(Bl), n, faces.ctypes.data_as(ip)] + nul[:2] + [o] + nul[3:]
    assert L.lgh_sample_faces(*args(-1, out.data_ptr())) == 1 and b"nfaces = -1" in L.lgh_last_error()
    # no faces, or no output: fine, nothing runs
    assert L.lgh_sample_faces(*args(0, out.data_ptr())) == 0
    assert L.lgh_sample_faces(*args(5, None)) == 0
    c.ctx.sample_faces(c.Sd, c.rhod, Bh, Gh, Bl, np.zeros((0, 2), np.int32), e=out)
    c.ctx.sync()
    assert np.all(np.isnan(out.cpu().numpy()))
    # 1D: refused whatever is asked (and so is the vorticity, as the derived kernel refuses it there)
    c1 = Case((3,), 2, 1)
    try:
        T1 = lattice_tables3(2, 1, 2)
        for name in ("x", "vorticity"):
            o1 = c1.ctx.to_dev(np.full(9, np.nan))
            with pytest.raises(LghError, match="dim = 1"):
                c1.ctx.sample_faces(c1.Sd, c1.rhod, *T1, np.array([[0, 0]], np.int32), **{name: o1})
            c1.ctx.sync()
            assert np.all(np.isnan(o1.cpu().numpy()))
        with pytest.raises(LghError):
            c1.ctx.faces_per_block(3)
    finally:
        c1.close()


def test_face_fields_of_the_operator():
    """HydroOperator.face_fields is the call of the tests above with the host library's tables and its own density projection:
    the bits of derived_fields / the sampler at the matching lattice points; and the operator is left alone"""
    from helpers import deformed_state, make_gpu
    from lattice_ref import lattice_tables
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1)
    g = make_gpu(prob, cg_tol=1e-12)
    try:
        S = deformed_state(prob, seed=5)
        Sd = g.ctx.to_dev(S)
        g.update_quadrature_data(Sd)
        g.ctx.sync()
        triple = g.ctx.quadrature_generation()
        R = 3
        faces = g.ctx.boundary_faces()
        assert len(faces) == 6 * 16
        d = g.face_fields(Sd, R, faces)
        assert set(d) == set(NAMES) | {"faces"} and all(np.isfinite(a).all() for a in d.values())
        assert g.ctx.quadrature_generation() == triple and np.array_equal(Sd.cpu().numpy(), S)
        vol = g.derived_fields(Sd, R)
        idx = face_volume_index(3, R + 1, faces)
        for k in ("detj", "div_v", "sound_speed"):
            assert np.array_equal(bits(d[k]), bits(vol[k][idx])), k
        for k in ("grad_v", "vorticity"):
            assert np.array_equal(bits(d[k]), bits(vol[k][:, idx])), k
        only = g.face_fields(Sd, R, faces[:7], fields=("p", "area_normal"))
        assert set(only) == {"p", "area_normal", "faces"} and np.array_equal(bits(only["p"]), bits(d["p"][:7 * 16]))
        with pytest.raises(ValueError):
            g.face_fields(Sd, R, faces, fields=("enstrophy",))
    finally:
        g.close()
