"""lgh_contour and its companions (Context.contour, contour_gather, contour_scalar, contour_zpb; HydroOperator.contour) against
tests/contour_ref.py, the numpy restatement of the definition in include/laghos_hip.h (tests/test_contour_ref.py holds that
reference to facts of its own).

Bars: the number of primitives, their lattice edges and zones equal to the reference in its order; the weights t bit-equal (one
IEEE division of two IEEE differences; the file is built without contraction); a second call gives the same bytes; a gathered
value within 2 eps max(|a|, |b|) of a + t (b - a) and exactly a where t == 0.

Set-up: the curved-mesh random state of tests/test_gpu_sample.py (its Case, on this file's zone grids); the scalars are the
sampling kernels' own lattice output - rho at its median, p, |v|, an oblique plane through the curved mesh, a scalar of small
integers with a third of the points on the value, all inside / all outside, one NaN.  Grids: one zone and a few, 75 zones, and
the grids of tests/shape_cases.py with ZPB - 1, ZPB or ZPB + 1 zones (ZPB = Context.contour_zpb: the zones of a workgroup); R1
below and above the workgroup size.  Outputs are filled before a call and carry a guard word behind the last entry."""
import ctypes

import numpy as np
import pytest

from contour_ref import contour_reference, gather_reference, measure, simplex_points
from shape_cases import SHAPES_2D, SHAPES_3D
from test_gpu_sample import Case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ZONES = {"2D-1x1": (1, 1), "2D-3x2": (3, 2), "3D-1x1x1": (1, 1, 1), "3D-3x2x2": (3, 2, 2), "3D-5x5x3": (5, 5, 3)}
ORDERS = [(1, 0), (2, 1), (3, 2)]
R1S = [2, 3, 6, 9]
GUARD_I, GUARD_D, FILL_I = -77, -1234.5, -5


def documented_zpb(dim, R1):
    """include/laghos_hip.h: min(16, 1024 / R1^dim), at least 1"""
    return max(1, min(16, 1024 // R1 ** dim))


def edge_grids():
    """(zones, R1) of tests/shape_cases.py with ZPB - 1, ZPB or ZPB + 1 zones"""
    out = []
    for shapes in (SHAPES_2D, SHAPES_3D):
        for R1 in R1S:
            seen = set()
            for zones in shapes:
                NE, zpb = int(np.prod(zones)), documented_zpb(len(zones), R1)
                if abs(NE - zpb) <= 1 and NE not in seen:
                    seen.add(NE)
                    out.append((zones, R1))
    return out


EDGES = edge_grids()
RUNS = [(ZONES[z], o, R1) for z in ZONES for o in ORDERS for R1 in R1S] + [(zones, (3, 2), R1) for zones, R1 in EDGES]
run_id = lambda r: f"{'x'.join(map(str, r[0]))}-Q{r[1][0]}Q{r[1][1]}-R1={r[2]}"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class ContourCase(Case):
    def __init__(self, zones, ok, ot, renumber=None):
        super().__init__(zones, ok, ot, renumber)
        self._lat = {}

    def lattice(self, R1):
        """the lattice arrays of lgh_sample_fields and the scalars formed from them, on the device; made once, never written"""
        if R1 not in self._lat:
            ctx, dim, NP = self.ctx, self.dim, self.NE * R1 ** self.dim
            Bh, Bl = self.tables(R1)
            d = dict(x=ctx.empty(dim * NP), v=ctx.empty(dim * NP), e=ctx.empty(NP), rho=ctx.empty(NP), p=ctx.empty(NP))
            ctx.sample_fields(self.Sd, self.rhod, Bh, Bl, **d)
            self.normal = np.array([0.6, -0.3, 0.74][:dim])
            d["speed"] = ctx.contour_scalar("norm", d["v"])
            d["plane"] = ctx.contour_scalar("plane", d["x"], self.normal)
            ctx.sync()
            h = {k: t.cpu().numpy() for k, t in d.items()}
            d["ties"] = ctx.to_dev(np.floor(2.0 * h["rho"]))        # 1, 2 or 3: about a third of the points at 2
            h["ties"] = d["ties"].cpu().numpy()
            for a in h.values():
                assert np.all(np.isfinite(a))
                a.setflags(write=False)
            self._lat[R1] = (d, h)
        return self._lat[R1]

    def scalars(self, R1):
        """name -> (device scalar, host copy, iso)"""
        d, h = self.lattice(R1)
        mid = lambda a, q=0.5: float(np.quantile(a, q))
        return {"rho": (d["rho"], h["rho"], mid(h["rho"])), "p": (d["p"], h["p"], mid(h["p"], 0.6)), "speed": (d["speed"], h["speed"], mid(h["speed"])),
                "plane": (d["plane"], h["plane"], mid(h["plane"], 0.45)), "ties": (d["ties"], h["ties"], 2.0)}

    def run(self, R1, sd, iso, capacity=None, zone=True):
        """One call with buffers for `capacity` primitives (None: as many as the counting call names), filled and guarded:
        (n_prims, n_skipped, edges, t, zone, written) - `written` False when every entry still holds its fill"""
        import torch
        ctx, dim = self.ctx, self.dim
        need, ns0 = ctx.contour_into(sd, iso, R1, 0)
        cap = need if capacity is None else capacity
        mk = lambda n, fill, guard, dt: torch.as_tensor(np.concatenate([np.full(n, fill), [guard]]).astype(dt)).to(ctx.device)
        e, t, z = mk(2 * dim * cap, FILL_I, GUARD_I, np.int32), mk(dim * cap, np.nan, GUARD_D, np.float64), mk(cap, FILL_I, GUARD_I, np.int32)
        ctx._torch_done()
        n, ns = ctx.contour_into(sd, iso, R1, cap, e if cap else None, t if cap else None, z if (zone and cap) else None)
        ctx.sync()
        assert (n, ns) == (need, ns0), "the counting call and the emitting call disagree"
        e, t, z = e.cpu().numpy(), t.cpu().numpy(), z.cpu().numpy()
        assert e[-1] == GUARD_I and t[-1] == GUARD_D and z[-1] == GUARD_I, "the word behind an array was written"
        written = not (np.all(e[:-1] == FILL_I) and np.all(np.isnan(t[:-1])) and np.all(z[:-1] == FILL_I))
        return n, ns, e[:-1].reshape(cap, dim, 2), t[:-1].reshape(cap, dim), z[:-1], written


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(zones, order, renumber=None):
        key = (tuple(zones), order, renumber)
        if key not in made:
            made[key] = ContourCase(zones, order[0], order[1], renumber)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def check_against_reference(c, R1, name, sd, sh, iso, what):
    n, ns, e, t, z, _ = c.run(R1, sd, iso)
    re, rt, rz, rns = contour_reference(c.dim, c.NE, R1, sh, iso)
    print(f"{what} {name}: {n} primitives, {ns} skipped")
    assert (n, ns) == (len(rt), rns), (what, name)
    assert np.array_equal(e, re) and np.array_equal(z, rz), (what, name)
    assert np.array_equal(bits(t), bits(rt)), (what, name, "t differs in bits", int((bits(t) != bits(rt)).sum()))
    return n, e, t, z


@pytest.mark.parametrize("zones,order,R1", RUNS, ids=[run_id(r) for r in RUNS])
def test_contour_equals_the_reference(cases, zones, order, R1):
    c = cases(zones, order)
    assert c.ctx.contour_zpb(R1) == documented_zpb(c.dim, R1)
    what = run_id((zones, order, R1))
    S_before, gen = c.S.copy(), c.ctx.quadrature_generation()
    total = 0
    for name, (sd, sh, iso) in c.scalars(R1).items():
        n, e, t, z = check_against_reference(c, R1, name, sd, sh, iso, what)
        total += n
        if name in ("rho", "ties"):
            # a second call gives the same bytes; the zone array may be left out
            n2, _, e2, t2, z2, _ = c.run(R1, sd, iso, zone=False)
            assert n2 == n and np.array_equal(e2, e) and np.array_equal(bits(t2), bits(t)) and (n == 0 or np.all(z2 == FILL_I))
        assert np.all(np.isfinite(t))
    assert total > 0
    # all inside, all outside: nothing, outputs untouched
    sd, sh, _ = c.scalars(R1)["rho"]
    for iso in (sh.min() - 1.0, sh.max() + 1.0):
        n, ns, _, _, _, written = c.run(R1, sd, iso, capacity=3)
        assert (n, ns) == (0, 0) and not written
    assert np.array_equal(c.Sd.cpu().numpy(), S_before) and c.ctx.quadrature_generation() == gen
    assert np.array_equal(sd.cpu().numpy(), sh), "the scalar was written"


NAN_RUNS = [((3, 2), (2, 1), 3), ((3, 2), (3, 2), 9), ((3, 2, 2), (3, 2), 6), ((1, 1, 1), (1, 0), 2), ((5, 5, 3), (2, 1), 3)]


@pytest.mark.parametrize("zones,order,R1", NAN_RUNS, ids=[run_id(r) for r in NAN_RUNS])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_a_value_that_is_not_finite(cases, zones, order, R1, bad):
    c = cases(zones, order)
    _, sh, iso = c.scalars(R1)["rho"]
    s = sh.copy()
    hole = (7 * len(s)) // 11
    s[hole] = bad
    sd = c.ctx.to_dev(s)
    n, e, t, z = check_against_reference(c, R1, "rho with a hole", sd, s, iso, run_id((zones, order, R1)))
    touched = (simplex_points(c.dim, c.NE, R1).reshape(-1, c.dim + 1) == hole).any(1)
    _, ns, _, _, _, _ = c.run(R1, sd, iso)
    assert ns == touched.sum() > 0 and np.all(np.isfinite(t)) and not (e == hole).any()


@pytest.mark.parametrize("zones,order,R1", [((3, 2), (3, 2), 6), ((3, 2, 2), (2, 1), 3), ((5, 5, 3), (3, 2), 6), ((17, 1, 1), (3, 2), 2)])
def test_capacity(cases, zones, order, R1):
    c = cases(zones, order)
    sd, sh, iso = c.scalars(R1)["rho"]
    need = len(contour_reference(c.dim, c.NE, R1, sh, iso)[1])
    assert need > 1
    for cap in (need - 1, 1):
        n, ns, e, t, z, written = c.run(R1, sd, iso, capacity=cap)
        assert n == need and ns == 0 and not written, cap
    n, ns, e, t, z, written = c.run(R1, sd, iso, capacity=need)          # (run checks the guard words)
    assert n == need and written and np.all(np.isfinite(t)) and np.all(e >= 0) and np.all(z >= 0)
    n, ns, e2, t2, z2, written = c.run(R1, sd, iso, capacity=need + 5)
    assert np.array_equal(e2[:need], e) and np.all(e2[need:] == FILL_I) and np.all(np.isnan(t2[need:])) and np.all(z2[need:] == FILL_I)


@pytest.mark.parametrize("zones", [(3, 2, 2), (3, 2)])
def test_renumbered_mesh(cases, zones):
    c = cases(zones, (3, 2), "random")
    assert not np.array_equal(c.elem_perm, np.arange(c.NE))
    for R1 in (3, 6):
        for name, (sd, sh, iso) in c.scalars(R1).items():
            check_against_reference(c, R1, name, sd, sh, iso, f"random {zones} R1={R1}")


@pytest.mark.parametrize("zones,order,R1", [((3, 2), (3, 2), 9), ((3, 2, 2), (3, 2), 3), ((5, 5, 3), (2, 1), 6), ((1, 1, 1), (1, 0), 2)])
def test_gather_and_scalars(cases, zones, order, R1):
    c = cases(zones, order)
    d, h = c.lattice(R1)
    dim, NP = c.dim, c.NE * R1 ** c.dim
    # the two scalars: the plane in the bits of its definition, |v| within its rounding (three roundings under the root)
    x, v = h["x"].reshape(dim, NP), h["v"].reshape(dim, NP)
    plane = c.normal[0] * x[0] + c.normal[1] * x[1]
    speed2 = v[0] * v[0] + v[1] * v[1]
    if dim == 3:
        plane, speed2 = plane + c.normal[2] * x[2], speed2 + v[2] * v[2]
    assert np.array_equal(bits(h["plane"]), bits(plane))
    assert np.all(np.abs(h["speed"] - np.sqrt(speed2)) <= 2 * EPS * np.sqrt(speed2))
    for name in ("rho", "ties"):
        sd, sh, iso = c.scalars(R1)[name]
        edges, t, zone, ns = c.ctx.contour(sd, iso, R1)
        re, rt, rz, _ = contour_reference(dim, c.NE, R1, sh, iso)
        assert np.array_equal(edges.cpu().numpy(), re) and np.array_equal(bits(t.cpu().numpy()), bits(rt)) and np.array_equal(zone.cpu().numpy(), rz)
        for k, nc in (("x", dim), ("v", dim), ("e", 1), ("p", 1)):
            got = c.ctx.contour_gather(edges, t, d[k], nc)
            c.ctx.sync()
            got = got.cpu().numpy().reshape(nc, len(rt), dim)
            f = h[k].reshape(nc, NP)
            a, b = f[:, re[..., 0]], f[:, re[..., 1]]
            assert np.all(np.abs(got - gather_reference(re, rt, f)) <= 2 * EPS * np.maximum(np.abs(a), np.abs(b))), (name, k)
            at0 = np.broadcast_to(rt == 0.0, a.shape)
            assert np.array_equal(bits(got[at0]), bits(a[at0])), (name, k, "t == 0 is not the end point")
        if name == "ties" and c.NE > 1:
            assert (rt == 0.0).any() and (rt == 1.0).any()
        # the gathered scalar is the value
        g = c.ctx.contour_gather(edges, t, sd)
        c.ctx.sync()
        s0, s1 = sh[re[..., 0]], sh[re[..., 1]]
        assert np.all(np.abs(g.cpu().numpy().reshape(-1, dim) - iso) <= 4 * EPS * np.maximum(np.maximum(np.abs(s0), np.abs(s1)), abs(iso)))


def test_refused_calls_set_the_error_and_run_no_kernel(cases):
    from laghos_amd import _lib
    from laghos_amd._lib import LghError
    L = _lib.load()
    c = cases((3, 2, 2), (2, 1))
    R1 = 3
    sd, sh, iso = c.scalars(R1)["rho"]
    need = c.ctx.contour_into(sd, iso, R1, 0)[0]

    def buffers(n, dim):
        import torch
        e = torch.full((2 * dim * n,), FILL_I, dtype=torch.int32, device=c.ctx.device)
        t = c.ctx.to_dev(np.full(dim * n, np.nan))
        return e, t

    def refused(ctx, match, R1_, scalar, cap, e, t):
        with pytest.raises(LghError, match=match) as ei:
            ctx.contour_into(scalar, iso, R1_, cap, e, t)
        assert str(ei.value).split(": ", 1)[1] == L.lgh_last_error().decode()
        ctx.sync()
        assert np.all(e.cpu().numpy() == FILL_I) and np.all(np.isnan(t.cpu().numpy())), (match, "a kernel ran")

    e, t = buffers(need, 3)
    refused(c.ctx, "R1 = 1 ", 1, sd, need, e, t)
    refused(c.ctx, "R1 = 10 ", 10, sd, need, e, t)
    refused(c.ctx, "scalar is NULL", R1, None, need, e, t)
    refused(c.ctx, "capacity = -1", R1, sd, -1, e, t)
    with pytest.raises(LghError, match="edges_out NULL"):
        c.ctx.contour_into(sd, iso, R1, need, None, t)
    for bad in (1, 10):
        with pytest.raises(LghError, match=f"R1 = {bad} "):
            c.ctx.contour_zpb(bad)
    c1 = Case((3,), 2, 1)
    try:
        e1, t1 = buffers(4, 1)
        s1 = c1.ctx.to_dev(np.arange(9.0))
        refused(c1.ctx, "dim = 1", 3, s1, 4, e1, t1)
        with pytest.raises(LghError, match="dim = 1"):
            c1.ctx.contour_zpb(3)
    finally:
        c1.close()


@pytest.mark.parametrize("mesh,normal,d,want", [("cube01_hex", (1.0, 1.0, 1.0), 1.5, 0.75 * np.sqrt(3.0)), ("square01_quad", (1.0, 2.0), 1.0, 0.5 * np.sqrt(5.0))])
def test_closed_form_surfaces_through_the_operator(mesh, normal, d, want):
    """the hexagon x + y + z = 1.5 of the unit cube and the segment x + 2 y = 1 of the unit square on the undeformed mesh:
    a linear scalar on an affine lattice is contoured exactly, 1e-12 relative"""
    from helpers import make_gpu
    from oracle.fem import Problem
    prob = Problem(mesh=mesh, rs=1, order_v=3, order_e=2, problem=1)
    g = make_gpu(prob, cg_tol=1e-12)
    try:
        S = prob.initial_state()[0]
        Sd = g.ctx.to_dev(S)
        triple = g.ctx.quadrature_generation()
        for R in (1, 3, 5):
            res = g.contour(Sd, R, ("plane", normal, d), fields=("div_v",))
            dim = len(normal)
            nprim = len(res["zone"])
            P = res["points"].reshape(dim, nprim, dim)
            got = measure(P)
            print(f"{mesh} R={R}: {nprim} primitives, measure {got:.16g}, relative error {abs(got / want - 1):.2e}")
            assert res["n_skipped"] == 0 and nprim > 0 and res["cells"].shape == (nprim, dim)
            assert abs(got - want) <= 1e-12 * want
            assert set(res) >= {"points", "cells", "zone", "v", "e", "rho", "p", "div_v", "n_skipped"}
            assert res["v"].shape == (dim, dim * nprim) and res["rho"].shape == (dim * nprim,) and np.all(np.isfinite(res["rho"]))
            # every point lies on the plane.  In units of eps |n|_1 (coordinates in [0, 1]): 3 for the rounded weight (1.5 eps of
            # |iso - s0| <= 2 |n|_1), 1.5 for the rounded lattice scalar, 1.5 for the gather, 1.5 for the sum below
            on = sum(normal[a] * res["points"][a] for a in range(dim))
            assert np.all(np.abs(on - d) <= 8 * EPS * sum(abs(n) for n in normal))
        # an iso-surface of a field: the same route
        cut = g.contour(Sd, 2, "x", 0.3)
        assert len(cut["zone"]) > 0 and np.all(np.abs(cut["points"][0] - 0.3) <= 4 * EPS)
        with pytest.raises(ValueError):
            g.contour(Sd, 2, "enstrophy", 1.0)
        with pytest.raises(ValueError):
            g.contour(Sd, 2, "density", float("nan"))
        with pytest.raises(ValueError):
            g.contour(Sd, 2, ("plane", (0.0,) * len(normal), 1.0))
        assert g.ctx.quadrature_generation() == triple and np.array_equal(Sd.cpu().numpy(), S)
    finally:
        g.close()
