"""lgh_sample_fields (Context.sample_fields): the fields of a state on the visualisation lattice against a numpy einsum of
the test's own tables over the element -> node map (tests/lattice_ref.py).  Curved mesh (x is not affine), random v, e
(negative values included: the max(e, 0) of the pressure shows), random density dofs, a random gamma per zone.

Shapes: the smallest at which the kernel can go wrong - one zone, a few, more than one workgroup's worth in 1D (257),
unequal zone counts per axis (an axis mix-up shows), 75 zones (no multiple of any zones-per-workgroup); lattices smaller
and larger than the dof grid (R1 < D1D, R1 > D1D), R1^dim below and above the workgroup size.

Tolerance 1e-13 * max|field| per field: at most D1D^dim <= 125 products of O(1) basis values with O(1) data, summed in
fp64 in another order than numpy's (125 * 2^-53 = 1.4e-14 of the largest term)."""
import numpy as np
import pytest

from lattice_ref import lattice_tables, sample_reference

pytestmark = pytest.mark.gpu

TOL = 1e-13
ZONES = {"1D-1": (1,), "1D-3": (3,), "1D-257": (257,), "2D-3x2": (3, 2), "3D-3x2x2": (3, 2, 2), "3D-5x5x3": (5, 5, 3)}
ORDERS = [(1, 0), (2, 1), (3, 2)]
CASES = [(z, o) for z in ZONES for o in ORDERS] + [("2D-3x2", (4, 3))]
R1S = [2, 3, 6, 9]


class Case:
    """One discretisation with a context on the GPU and a random state on a curved mesh."""

    def __init__(self, zones, ok, ot, renumber=None):
        from laghos_amd import host_lib
        from laghos_amd.context import Context
        dim = len(zones)
        if renumber is None:
            from oracle.fem import Problem
            p = Problem(breaks=[np.linspace(0.0, 1.0, n + 1) for n in zones], order_v=ok, order_e=ot, problem=1)
            x0 = p.initial_state()[0][:p.H1V]
            h1map, N, W, ess, B, G, Bl = np.asarray(p.h1map).reshape(-1), p.N, p.W, p.ess, p.B, p.G, p.Bl
        else:
            d = host_lib.host_disc("cartesian", 0, ok, ot, 1, zones=zones, renumber=renumber, seed=5)
            t = host_lib.host_tables(ok, ot)
            h1map, W, ess, B, G, Bl = d["h1map"], d["W"], d["ess"], t["B"], t["G"], t["Bl"]
            N = int(h1map.max()) + 1
            x0 = d["S0"][:dim * N]
            self.elem_perm, self.node_perm = d["elem_perm"], d["node_perm"]
        self.dim, self.NE, self.N, self.D, self.L = dim, int(np.prod(zones)), N, ok + 1, ot + 1
        self.ok, self.ot, self.h1map = ok, ot, h1map
        NE, NL, H1V = self.NE, self.L ** dim, dim * N
        rng = np.random.default_rng(1000 * dim + 10 * ok + NE)
        hmin = 1.0 / (max(zones) * ok)
        self.S = np.concatenate([x0 + 0.2 * hmin * rng.uniform(-1, 1, H1V),      # curved zones
                                 rng.uniform(-1, 1, H1V), rng.uniform(-0.5, 1.0, NE * NL)])
        self.rho = rng.uniform(0.5, 2.0, NE * NL)
        self.gamma = rng.uniform(1.2, 1.8, NE)
        Q = B.shape[0]
        self.ctx = Context(dim, NE, self.D, Q, self.L, N, h1map, B, G, Bl, W, self.gamma, ess, order_v=ok)
        self.Sd, self.rhod = self.ctx.to_dev(self.S), self.ctx.to_dev(self.rho)
        self._ref = {}

    def tables(self, R1):
        return lattice_tables(self.ok, self.ot, R1 - 1)

    def reference(self, R1):
        if R1 not in self._ref:   # computed once, shared, never written
            Bh, Bl = self.tables(R1)
            ref = sample_reference(self.dim, self.NE, self.N, self.D, self.L, self.h1map, self.S, self.rho, self.gamma, Bh, Bl)
            for a in ref.values():
                a.setflags(write=False)
            self._ref[R1] = ref
        return self._ref[R1]

    def sample(self, R1, want=("x", "v", "e", "rho", "p"), rho_l2=True):
        """dict name -> numpy array of the outputs asked for (the others are passed as NULL)"""
        NP = self.NE * R1 ** self.dim
        Bh, Bl = self.tables(R1)
        # NaN-filled: an entry the kernel does not write shows
        out = {k: self.ctx.to_dev(np.full((self.dim if k in "xv" else 1) * NP, np.nan)) for k in want}
        self.ctx.sample_fields(self.Sd, self.rhod if rho_l2 else None, Bh, Bl, **out)
        self.ctx.sync()
        return {k: (t.cpu().numpy().reshape(self.dim, NP) if k in "xv" else t.cpu().numpy()) for k, t in out.items()}

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(zones_id, order, renumber=None):
        key = (zones_id, order, renumber)
        if key not in made:
            made[key] = Case(ZONES[zones_id], order[0], order[1], renumber)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def check_fields(got, ref, what=""):
    for k, a in got.items():
        err, scale = np.abs(a - ref[k]).max(), np.abs(ref[k]).max()
        print(f"{what} {k}: max err {err:.3e}, max|field| {scale:.3e}")
        assert np.all(np.isfinite(a)), (what, k, "an entry was not written")
        assert err <= TOL * scale, (what, k, err, scale)


@pytest.mark.parametrize("R1", R1S)
@pytest.mark.parametrize("zones_id,order", CASES, ids=[f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES])
def test_sample_matches_numpy(cases, zones_id, order, R1):
    c = cases(zones_id, order)
    ref = c.reference(R1)
    if c.NE >= 12:   # the clamp of the pressure is in play
        assert (ref["e"] < 0).any() and (ref["p"] == 0).any() and (ref["p"] > 0).any()
    check_fields(c.sample(R1), ref, f"{zones_id} Q{order[0]}Q{order[1]} R1={R1}")


@pytest.mark.parametrize("zones_id,order,R1", [("1D-3", (2, 1), 3), ("2D-3x2", (3, 2), 6), ("3D-3x2x2", (3, 2), 3), ("3D-3x2x2", (2, 1), 6)])
def test_shared_faces_carry_the_same_x_and_v(cases, zones_id, order, R1):
    """x and v are continuous: the lattice points of a face two zones share have the same values from both sides
    (a transposed lattice index would pair the wrong points)."""
    c = cases(zones_id, order)
    got = c.sample(R1, want=("x", "v"))
    zones, dim = ZONES[zones_id], c.dim
    nz = list(zones) + [1] * (3 - dim)
    R1s = [R1 if a < dim else 1 for a in range(3)]
    pairs = 0
    for name in ("x", "v"):
        F = got[name].reshape(dim, nz[2], nz[1], nz[0], R1s[2], R1s[1], R1s[0])   # [c, ez, ey, ex, rz, ry, rx]
        scale = np.abs(F).max()
        for a in range(dim):   # neighbours along axis a: upper face of the lower zone = lower face of the upper zone
            lo = np.take(np.take(F, range(nz[a] - 1), axis=3 - a), R1 - 1, axis=6 - a)
            hi = np.take(np.take(F, range(1, nz[a]), axis=3 - a), 0, axis=6 - a)
            pairs += lo.size
            assert np.abs(lo - hi).max() <= TOL * scale if lo.size else True, (name, a)
    assert pairs > 0


@pytest.mark.parametrize("renumber", ["random", "mfem"])
def test_outputs_sit_at_the_callers_zone_ids(cases, renumber):
    """3 x 2 x 2 zones under another numbering of nodes and zones (Discretization::Renumber): the library may walk the zones
    in an order of its own, the outputs are indexed by the caller's zone ids"""
    c = cases("3D-3x2x2", (3, 2), renumber)
    if renumber == "random":
        assert not np.array_equal(c.elem_perm, np.arange(c.NE))
    assert not np.array_equal(c.node_perm, np.arange(c.N))
    for R1 in (3, 6):
        check_fields(c.sample(R1), c.reference(R1), f"{renumber} R1={R1}")
    # and they are the values of the same zones of the mesh in its lexicographic numbering: zone j is the structured zone
    # elem_perm[j], structured node i is node node_perm[i]
    lex = cases("3D-3x2x2", (3, 2))
    H1V, NL = 3 * c.N, c.L ** 3
    S_lex = np.concatenate([c.S[k * c.N:(k + 1) * c.N][c.node_perm] for k in range(6)]
                           + [c.S[2 * H1V:].reshape(c.NE, NL)[np.argsort(c.elem_perm)].reshape(-1)])
    rho_lex = c.rho.reshape(c.NE, NL)[np.argsort(c.elem_perm)].reshape(-1)
    Bh, Bl = lex.tables(3)
    ref = sample_reference(3, lex.NE, lex.N, lex.D, lex.L, lex.h1map, S_lex, rho_lex, c.gamma[np.argsort(c.elem_perm)], Bh, Bl)
    got = c.sample(3)
    for k in ("x", "v", "e", "rho", "p"):
        a_ren = got[k].reshape(-1, c.NE, 27)
        a_lex = ref[k].reshape(-1, c.NE, 27)[:, c.elem_perm]
        assert np.abs(a_ren - a_lex).max() <= TOL * np.abs(a_lex).max(), k


@pytest.mark.parametrize("zones_id,order,R1", [("1D-257", (3, 2), 3), ("2D-3x2", (4, 3), 6), ("3D-5x5x3", (3, 2), 3), ("3D-3x2x2", (3, 2), 9)])
def test_every_output_alone_gives_the_same_bits(cases, zones_id, order, R1):
    c = cases(zones_id, order)
    full = c.sample(R1)
    for k in ("x", "v", "e", "rho", "p"):
        alone = c.sample(R1, want=(k,))
        assert np.array_equal(alone[k], full[k]), k
    e_only = c.sample(R1, want=("e",), rho_l2=False)   # without density dofs: x, v, e are still served
    assert np.array_equal(e_only["e"], full["e"])


def test_two_calls_give_identical_bits(cases):
    for zones_id, order, R1 in (("3D-5x5x3", (3, 2), 6), ("1D-257", (2, 1), 2), ("2D-3x2", (3, 2), 9)):
        c = cases(zones_id, order)
        a, b = c.sample(R1), c.sample(R1)
        for k in a:
            assert np.array_equal(a[k], b[k]), (zones_id, k)


def test_refused_calls_name_the_argument(cases):
    from laghos_amd._lib import LghError
    c = cases("3D-3x2x2", (2, 1))
    with pytest.raises(LghError, match="rho_l2"):
        c.sample(3, want=("rho",), rho_l2=False)
    with pytest.raises(LghError, match="rho_l2"):
        c.sample(3, want=("x", "p"), rho_l2=False)
    for R1 in (1, 10):
        NP = c.NE * R1 ** 3
        out = c.ctx.zeros(NP)
        Bh, Bl = np.ones((R1, c.D)), np.ones((R1, c.L))
        with pytest.raises(LghError, match="R1"):
            c.ctx.sample_fields(c.Sd, c.rhod, Bh, Bl, e=out)
        c.ctx.sync()
        assert not out.cpu().numpy().any()   # no kernel ran


def test_sampling_leaves_the_operator_alone():
    """The quadrature data, its generation counter and the fused force products are untouched: dS/dt of a state is the same
    bits before and after a sample, lgh_quadrature_generation returns the same triple around it, S is unchanged."""
    from helpers import deformed_state, make_gpu
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1)
    g = make_gpu(prob, cg_tol=1e-12)
    try:
        S = deformed_state(prob, seed=5)
        Sd = g.ctx.to_dev(S)

        def rhs():
            dS = g.ctx.zeros(S.size)
            g.reset_quadrature_data()
            g.mult(Sd, dS)
            g.ctx.sync()
            return dS.cpu().numpy()

        before = rhs()
        g.update_quadrature_data(Sd)              # quadrature data and fused products of S on hand
        g.ctx.sync()
        triple = g.ctx.quadrature_generation()
        rho = g.compute_density(Sd)
        R1 = 4
        NP = prob.NE * R1 ** 3
        Bh, Bl = lattice_tables(3, 2, R1 - 1)
        out = dict(x=g.ctx.zeros(3 * NP), v=g.ctx.zeros(3 * NP), e=g.ctx.zeros(NP), rho=g.ctx.zeros(NP), p=g.ctx.zeros(NP))
        t0 = g.ctx.quadrature_generation()
        g.ctx.sample_fields(Sd, rho, Bh, Bl, **out)
        g.ctx.sync()
        assert g.ctx.quadrature_generation() == t0 == triple
        assert np.abs(out["x"].cpu().numpy()).max() > 0
        assert np.array_equal(Sd.cpu().numpy(), S)
        # the data the sample must not have touched is used as it stands: no reset in between
        dS = g.ctx.zeros(S.size)
        g.mult(Sd, dS)
        g.ctx.sync()
        assert np.array_equal(dS.cpu().numpy(), before)
        assert np.array_equal(rhs(), before)
    finally:
        g.close()
